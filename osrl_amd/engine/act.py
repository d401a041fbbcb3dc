"""Host side of the B = 1 (.. 4) ``act()`` latency path (csrc/act.hip, include/osrl_amd.h ``osrl_policy_*``).

The reference's evaluation loop calls ``model.act(obs)`` once per environment step (cpq.py:330-347 ->
cpq.py:240-252; bcql.py:236-243; bc.py:57-64): a host->device copy of one observation, a handful of aten kernels and
two ``.cpu().numpy()`` syncs.  ``FastPolicy`` keeps ONE pinned, device-mapped I/O block per model: ``act()`` writes
the observation into it through a numpy view, makes one C call (one kernel launch + a spin on the published sequence
number) and reads the action back through another numpy view -- no torch tensor is created on this path.

The kernel reads the packed forward weight copies of the flat optimizer groups -- the ones the fused optimizer kernel
and ``load_state_dict`` keep in step with the parameters -- and the canonical biases; the flat buffers never move, so a
``FastPolicy`` built once stays valid for the model's lifetime (in-place edits of parameters from outside the trainer
need ``model.repack()``, as for training).

``VecFastPolicy`` is the same for ``num_envs`` episodes on as many host environments, advanced in lockstep by one C call
per environment step (csrc/act_vec.hip, ``osrl_policy_*_n``): the slots are rows of 16-row fp32-MFMA tiles, and a
slot's action does not depend on how many ran beside it.

``rollout_refill`` is the host-side scheduler both trainer families use for ``schedule="refill"``: a queue of jobs over
N environments, where a slot whose episode has ended takes the next job in the same policy call in which the others step
(``VecFastPolicy.step(restart=...)``, ``CDTVecFastPolicy.step(restart=...)``) instead of waiting for the longest episode
of its wave.  ``collect_refill`` is the same loop with a recorder: every job comes back as rows of a DSRL-layout
dataset (``Trainer.collect_jobs``), with the collectors' exploration noise added by the policy call itself
(``step(explore_std=...)``).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _lib as L
from .core import NetDesc, cur_stream, require_cuda


def _gemv_net(dst: "L.GemvNetT", desc: NetDesc) -> None:
    if desc.E != 1:
        raise ValueError("the latency path runs one policy network per stage")
    dst.n_layers = desc.nl
    for i, v in enumerate(desc.dims):
        dst.dims[i] = v
    for i, a in enumerate(desc.acts):
        dst.acts[i] = a
    dst.out_scale = desc.out_scale
    for l, r in enumerate(desc.nets[0]):
        if r.target:
            raise ValueError("policies act with their online parameters")
        dst.Wf[l], dst.b[l] = r.wf_ptr, r.b.data_ptr()


KINDS = {"mlp": L.POLICY_MLP, "gauss": L.POLICY_GAUSS, "bcq": L.POLICY_BCQ}
MAX_ENVS = L.POLICY_MAX_ENVS


def _policy_desc(kind: str, obs_dim: int, act_dim: int, net0: NetDesc, max_action: float, net1: Optional[NetDesc],
                 latent_dim: int, phi: float) -> "L.PolicyT":
    d = L.PolicyT()
    d.kind, d.obs_dim, d.act_dim, d.latent_dim = KINDS[kind], obs_dim, act_dim, latent_dim
    d.max_action, d.phi = float(max_action), float(phi)
    _gemv_net(d.net[0], net0)
    if net1 is not None:
        _gemv_net(d.net[1], net1)
    return d


def _vec_args(num_envs, limit: int, limit_name: str) -> int:
    if isinstance(num_envs, bool) or not isinstance(num_envs, (int, np.integer)):
        raise ValueError(f"num_envs must be an integer from 1 to {limit}, got {num_envs!r}")
    if not 1 <= int(num_envs) <= limit:
        raise ValueError(f"num_envs {int(num_envs)} is outside 1 .. {limit} ({limit_name})")
    return int(num_envs)


class PinnedHandle:
    """A handle to a pinned, device-mapped I/O block behind a ctypes pointer; ``DESTROY`` names the C call that frees
    it.  It cannot be copied or pickled: a copied / unpickled model simply has no fast policy yet and builds its own on
    first use (the models test ``_fast is None``)."""

    DESTROY = ""

    def _open(self, device, entry: str, *args):
        """Creates the handle on ``device`` by ``entry(*args, &handle)``; returns the library."""
        self.device = torch.device(device)
        lib = L.load()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(getattr(lib, entry)(*args, C.byref(h)), entry)
        self._h, self._lib = h, lib
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        return lib

    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (type(None), ())

    def _stream(self):
        return self._raw_stream(self._dev_index) if self._raw_stream is not None else cur_stream()

    def _rows(self, name, x, tail, dtype=None) -> np.ndarray:
        """``x`` as an array of shape ``(num_envs,) + tail``: for the lockstep handles, which set ``num_envs``."""
        want = (self.num_envs,) + tail
        if np.shape(x) != want:  # numpy would broadcast silently
            raise ValueError(f"expected {name} of shape {want}, got {np.shape(x)}")
        return np.asarray(x, dtype=dtype)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            getattr(self._lib, self.DESTROY)(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass


class FastPolicy(PinnedHandle):
    """``kind``: "mlp" (BC), "gauss" (squashed-Gaussian actor), "bcq" (VAE decoder + perturbation actor)."""

    KINDS = KINDS
    DESTROY = "osrl_policy_destroy"

    def __init__(self, kind: str, device, obs_dim: int, act_dim: int, net0: NetDesc, max_action: float = 1.0,
                 net1: Optional[NetDesc] = None, latent_dim: int = 0, phi: float = 0.0, seed: int = 0):
        require_cuda(device)
        d = _policy_desc(kind, obs_dim, act_dim, net0, max_action, net1, latent_dim, phi)
        self._keep = (net0, net1)  # the descriptors hold the parameter views alive
        self.kind, self.obs_dim, self.act_dim, self.seed = kind, obs_dim, act_dim, int(seed)
        self.noise_dim = {"mlp": 0, "gauss": act_dim, "bcq": latent_dim}[kind]
        lib = self._open(device, "osrl_policy_create", C.byref(d))
        ptrs = [C.POINTER(C.c_float)() for _ in range(4)]
        L.check(lib.osrl_policy_io(self._h, *[C.byref(p) for p in ptrs]), "osrl_policy_io")
        R = L.POLICY_MAX_ROWS
        view = lambda p, shape: np.ctypeslib.as_array(p, shape=shape)  # noqa: E731  numpy views of PINNED memory
        self.obs = view(ptrs[0], (R, obs_dim))
        self.noise = view(ptrs[1], (R, max(self.noise_dim, 1)))
        self.act_out = view(ptrs[2], (R, act_dim))
        self.logp_out = view(ptrs[3], (R,))
        self._act1, self._obs1, self._lp1 = self.act_out[0], self.obs[0], self.logp_out[0:1].reshape(())
        self._fn = lib.osrl_policy_act
        self._gauss = kind == "gauss"

    def act1(self, obs, deterministic: bool = True):
        """The hot call of the episode loop: ONE observation [obs_dim], no explicit noise.  Everything a call does on
        the host: one numpy copy into pinned memory, one C call, one or two copies out."""
        if np.shape(obs) != self._obs1.shape:  # numpy would broadcast a scalar / length-1 observation silently
            raise ValueError(f"expected one observation of shape {self._obs1.shape}, got {np.shape(obs)}")
        self._obs1[:] = obs  # converts dtype
        st = self._raw_stream(self._dev_index) if self._raw_stream is not None else cur_stream()
        rc = self._fn(self._h, 1, 1 if deterministic else 0, 0, self.seed, st)
        if rc != 0:
            L.check(rc, "osrl_policy_act")
        return self._act1.copy(), (self._lp1.copy() if self._gauss else None)

    def act(self, obs, deterministic: bool = True, noise=None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """``obs``: [obs_dim] or [rows <= 4, obs_dim].  Returns copies (action[, log-prob]) with the input's leading
        shape.  ``noise``: explicit standard-normal draws ([.., act_dim] eps for "gauss", [.., latent_dim] z for
        "bcq"); omitted = drawn in the kernel (Philox) when the policy is stochastic."""
        if noise is None and np.ndim(obs) == 1:
            return self.act1(obs, deterministic)
        o = np.asarray(obs, dtype=np.float32)
        single = o.ndim == 1
        rows = 1 if single else o.shape[0]
        if rows > L.POLICY_MAX_ROWS or o.shape[-1] != self.obs_dim:
            raise ValueError(f"expected [<= {L.POLICY_MAX_ROWS}, {self.obs_dim}] observations, got {o.shape}")
        if single:
            self._obs1[:] = o
        else:
            self.obs[:rows] = o
        host_noise = 0
        if noise is not None and self.noise_dim:
            self.noise[:rows, :self.noise_dim] = np.asarray(noise, np.float32).reshape(rows, self.noise_dim)
            host_noise = 1
        rc = self._fn(self._h, rows, 1 if deterministic else 0, host_noise, self.seed, cur_stream())
        if rc != 0:
            L.check(rc, "osrl_policy_act")
        if single:
            return self._act1.copy(), (self.logp_out[0].copy() if self.kind == "gauss" else None)
        return self.act_out[:rows].copy(), (self.logp_out[:rows].copy() if self.kind == "gauss" else None)


class VecFastPolicy(PinnedHandle):
    """``num_envs`` episodes of one policy on as many host environments, in lockstep: ``reset`` starts episodes and
    ``step`` advances them, one C call each for all slots.  Same kinds and descriptors as ``FastPolicy``.  A slot's
    action is the same bits whatever ``num_envs`` is, whichever slot it is and whatever the other slots hold.

    A slot passed as inactive (``active[e] = False``) idles: its row of ``obs`` / ``noise`` is not read, its step does
    not advance and its rows of the results keep the values of its last active call.

    Noise the kernel draws itself (no ``noise`` argument: z of "bcq", eps of a stochastic "gauss") is keyed by the
    policy's seed, the slot's episode id and its step within the episode only, so an episode replays identically in any
    slot of a policy of any width."""

    KINDS = KINDS
    DESTROY = "osrl_policy_destroy_n"
    LIMIT = (MAX_ENVS, "OSRL_POLICY_MAX_ENVS")

    def __init__(self, kind: str, device, obs_dim: int, act_dim: int, net0: NetDesc, max_action: float = 1.0,
                 net1: Optional[NetDesc] = None, latent_dim: int = 0, phi: float = 0.0, seed: int = 0,
                 num_envs: int = 1):
        N = self.num_envs = _vec_args(num_envs, *self.LIMIT)
        require_cuda(device)
        d = _policy_desc(kind, obs_dim, act_dim, net0, max_action, net1, latent_dim, phi)
        self._keep = (net0, net1)  # the descriptors hold the parameter views alive
        self.kind, self.obs_dim, self.act_dim, self.seed = kind, obs_dim, act_dim, int(seed)
        self.noise_dim = {"mlp": 0, "gauss": act_dim, "bcq": latent_dim}[kind]
        lib = self._open(device, "osrl_policy_create_n", C.byref(d), N)
        h = self._h
        fp = [C.POINTER(C.c_float)() for _ in range(4)]
        ip = [C.POINTER(C.c_int32)() for _ in range(2)]
        L.check(lib.osrl_policy_io_n(h, *[C.byref(p) for p in fp + ip]), "osrl_policy_io_n")
        view = lambda p, shape: np.ctypeslib.as_array(p, shape=shape)  # noqa: E731  numpy views of PINNED memory
        self.obs = view(fp[0], (N, obs_dim))
        self.noise = view(fp[1], (N, max(self.noise_dim, 1)))
        self.act_out = view(fp[2], (N, act_dim))
        self.logp_out = view(fp[3], (N,))
        self._active = view(ip[0], (N,))
        self._meta = view(ip[1], (N, 2))  # (episode id, step) of each slot
        xp = [C.POINTER(C.c_float)() for _ in range(2)]
        L.check(lib.osrl_policy_explore_io_n(h, *[C.byref(p) for p in xp]), "osrl_policy_explore_io_n")
        self._sigma = view(xp[0], (N,))        # exploration scale of each slot
        self._eps = view(xp[1], (N, act_dim))  # injected exploration noise
        self._started = False

    def _checked(self, obs, active, noise):
        obs = self._rows("obs", obs, (self.obs_dim,))
        if active is not None:
            active = self._rows("active", active, ())
            if active.dtype != np.bool_:
                raise ValueError(f"expected active as booleans, got dtype {active.dtype}")
        if noise is not None:
            if not self.noise_dim:
                raise ValueError(f'a "{self.kind}" policy takes no noise')
            noise = self._rows("noise", noise, (self.noise_dim,), np.float32)
        return obs, active, noise

    def _ids(self, episode_ids) -> np.ndarray:
        if episode_ids is None:
            return np.arange(self.num_envs, dtype=np.int64)
        ids = self._rows("episode_ids", episode_ids, ())
        if ids.dtype.kind not in "iu" or (ids < 0).any() or (ids > 0x7FFFFFFF).any():
            raise ValueError("expected episode_ids as integers in 0 .. 2^31 - 1")
        return ids

    def _explore(self, explore_std, explore_seed, explore_noise):
        """The checked exploration arguments of a call: None, or (sigma [N] fp32, seed, eps [N, act_dim] fp32 or None)."""
        if explore_std is None:
            if explore_noise is not None:
                raise ValueError("explore_noise is the eps of explore_std: pass explore_std")
            return None
        sg = np.asarray(explore_std, dtype=np.float32)
        if sg.ndim != 0 and sg.shape != (self.num_envs,):
            raise ValueError(f"expected explore_std as a scalar or of shape ({self.num_envs},), got {sg.shape}")
        if explore_noise is not None:
            explore_noise = self._rows("explore_noise", explore_noise, (self.act_dim,), np.float32)
        return np.broadcast_to(sg, (self.num_envs,)), int(explore_seed) & 0xFFFFFFFFFFFFFFFF, explore_noise

    def _call(self, obs, active, noise, deterministic, explore=None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        if explore is not None:
            sel = slice(None) if active is None else active
            self._sigma[sel] = explore[0][sel]
            if explore[2] is not None:
                self._eps[sel] = explore[2][sel]
        if active is None:
            self.obs[:] = obs  # converts dtype
            self._active[:] = 1
            if noise is not None:
                self.noise[:, :self.noise_dim] = noise
        else:
            self.obs[active] = obs[active]
            self._active[:] = active
            if noise is not None:
                self.noise[active, :self.noise_dim] = noise[active]
        st = self._raw_stream(self._dev_index) if self._raw_stream is not None else cur_stream()
        if explore is None:
            rc = self._lib.osrl_policy_act_n(self._h, 1 if deterministic else 0, 0 if noise is None else 1, self.seed,
                                             st)
            if rc != 0:
                L.check(rc, "osrl_policy_act_n")
        else:
            rc = self._lib.osrl_policy_act_explore_n(self._h, 1 if deterministic else 0, 0 if noise is None else 1,
                                                     self.seed, explore[1], 0 if explore[2] is None else 1, st)
            if rc != 0:
                L.check(rc, "osrl_policy_act_explore_n")
        return self.act_out.copy(), (self.logp_out.copy() if self.kind == "gauss" else None)

    def reset(self, obs, episode_ids=None, active=None, noise=None, deterministic: bool = True, explore_std=None,
              explore_seed: int = 0, explore_noise=None):
        """Starts an episode in every active slot from ``obs [N, obs_dim]`` (``episode_ids``: ``[N]`` integers, default
        the slot numbers; ``active``: bool ``[N]``, default all) and returns the first ``(actions [N, act_dim],
        log-probs [N] or None)``.  ``explore_std`` / ``explore_seed`` / ``explore_noise``: as ``step`` takes them."""
        if self._h is None:
            raise RuntimeError("VecFastPolicy is closed")
        obs, active, noise = self._checked(obs, active, noise)
        explore = self._explore(explore_std, explore_seed, explore_noise)
        ids = self._ids(episode_ids)
        sel = slice(None) if active is None else active
        self._meta[sel, 0] = ids[sel]
        self._meta[sel, 1] = 0
        self._started = True
        return self._call(obs, active, noise, deterministic, explore)

    def step(self, obs, active=None, noise=None, deterministic: bool = True, restart=None, episode_ids=None,
             explore_std=None, explore_seed: int = 0, explore_noise=None):
        """The next ``(actions, log-probs or None)`` of every active slot from its new observation.  ``noise``:
        explicit standard-normal draws ``[N, act_dim]`` (eps of "gauss") or ``[N, latent_dim]`` (z of "bcq").
        ``restart`` (bool ``[N]``): the masked slots start a new episode from ``obs[e]`` instead of stepping -- they
        count as active and take ``episode_ids[e]`` (``[N]`` integers, default the slot numbers) at step 0, as ``reset``
        gives them -- while the other active slots step.
        ``explore_std`` (None: off, the call is the one without these arguments): the collectors' exploration tail on
        the returned action, ``clip(a + explore_std[e] * eps, +-max_action)`` with one sigma or ``[N]`` of them; a slot
        whose sigma is 0 returns its action's bits unchanged.  ``eps`` is ``explore_noise [N, act_dim]`` when given,
        else drawn in the kernel keyed by ``(explore_seed, the slot's episode id, its step, column)`` -- the device
        collectors' draw (``Trainer.collect``), apart from the policy's own noise.  The log-probs stay those of the
        policy's own action."""
        if self._h is None:
            raise RuntimeError("VecFastPolicy is closed")
        if restart is not None:
            restart = self._rows("restart", restart, ())
            if restart.dtype != np.bool_:
                raise ValueError(f"expected restart as booleans, got dtype {restart.dtype}")
            ids = self._ids(episode_ids)
            if not restart.any():
                restart = None
        elif episode_ids is not None:
            raise ValueError("episode_ids belong to the slots that restart: pass restart")
        if not self._started and restart is None:
            raise RuntimeError("call reset() before step()")
        obs, active, noise = self._checked(obs, active, noise)
        explore = self._explore(explore_std, explore_seed, explore_noise)
        if restart is None:
            self._meta[slice(None) if active is None else active, 1] += 1
            return self._call(obs, active, noise, deterministic, explore)
        stepping = ~restart if active is None else active & ~restart
        self._meta[stepping, 1] += 1
        self._meta[restart, 0] = ids[restart]
        self._meta[restart, 1] = 0
        self._started = True
        return self._call(obs, None if active is None else active | restart, noise, deterministic, explore)


def cached_vec_policy(model, num_envs, make, limit=VecFastPolicy.LIMIT):
    """``model``'s lockstep policy of width ``num_envs`` (one per width, built by ``make(num_envs)`` on first use);
    ``limit``: the policy class's ``LIMIT``."""
    N = _vec_args(num_envs, *limit)
    cache = model.__dict__.setdefault("_fast_vec", {})
    if cache.get(N) is None:  # (None: the slot of a copied / unpickled model)
        cache[N] = make(N)
    return cache[N]


def rollout_lockstep(model, envs, num_slots=None, episode_ids=None, cost_scale=None, append=None):
    """The MLP trainers' ``rollout()`` on each of the host environments ``envs`` at once, through
    ``model.fast_policy(num_envs)``: one C call per environment step for all of them.  Returns three arrays (return,
    length, cost sum), one entry per environment.  A slot leaves the loop when its environment terminates, truncates or
    reaches ``model.episode_len``; the slots past ``len(envs)`` idle.  ``cost_scale``: factor on ``info["cost"]`` (None:
    summed as it is); ``append``: a value appended to every observation (BC's multi-task cost limit); ``episode_ids``
    (default 0 .. len(envs) - 1) key the noise the policy draws on the device."""
    envs = list(envs)
    n = len(envs)
    N = n if num_slots is None else int(num_slots)
    if N < n:
        raise ValueError(f"{n} environments do not fit {N} slots")
    ep_ret, ep_len, ep_cost = [0.0] * n, np.zeros(n, np.int64), [0.0] * n
    if episode_ids is not None and np.shape(episode_ids) != (n,):
        raise ValueError(f"expected episode_ids of shape ({n},), got {np.shape(episode_ids)}")
    if n == 0:
        return np.asarray(ep_ret), ep_len, np.asarray(ep_cost)
    ids = np.zeros(N, np.int64)
    ids[:n] = np.arange(n) if episode_ids is None else episode_ids
    pol = model.fast_policy(num_envs=N)
    obs = np.zeros((N, pol.obs_dim), np.float32)
    active = np.zeros(N, bool)
    active[:n] = True
    put = (lambda o: o) if append is None else (lambda o: np.append(o, append))  # noqa: E731
    for e, env in enumerate(envs):
        o, _ = env.reset()
        obs[e] = put(o)
    act, _ = pol.reset(obs, episode_ids=ids, active=active)
    EL = model.episode_len
    for step in range(EL):
        for e in np.flatnonzero(active):
            o, r, terminated, truncated, info = envs[e].step(act[e])
            ep_ret[e] += r
            ep_len[e] += 1
            ep_cost[e] += info["cost"] if cost_scale is None else info["cost"] * cost_scale
            if terminated or truncated or step + 1 == EL:
                active[e] = False
                continue
            obs[e] = put(o)
        if not active.any():
            break
        act, _ = pol.step(obs, active=active)
    return np.asarray(ep_ret), ep_len, np.asarray(ep_cost)


def evaluate_lockstep(trainer, eval_episodes):
    """``eval_episodes`` rollouts over the list of host environments ``trainer.env``: episode ``q`` runs in wave
    ``q // N`` on environment ``q % N`` with episode id ``q``.  Returns the means (return, cost sum, length), not
    rescaled."""
    envs = list(trainer.env)
    N = len(envs)
    if N == 0:
        raise ValueError("evaluate over an empty list of environments")
    trainer.model.eval()
    rets, lens, costs = [], [], []
    for q0 in range(0, int(eval_episodes), N):
        k = min(N, int(eval_episodes) - q0)
        r, l, c = trainer.rollout_many(envs[:k], num_slots=N, episode_ids=np.arange(q0, q0 + k))
        rets += list(r)
        lens += list(l)
        costs += list(c)
    trainer.model.train()
    return np.mean(rets), np.mean(costs), np.mean(lens)


SCHEDULES = ("waves", "refill")


def check_schedule(schedule) -> str:
    if schedule not in SCHEDULES:
        raise ValueError(f'schedule must be "waves" or "refill", got {schedule!r}')
    return schedule


RefillResult = namedtuple("RefillResult", "returns lengths costs slots calls")
RefillResult.__doc__ = """What ``rollout_refill`` returns: per job its return, length and cost sum (arrays, job order) and
the slot (= index of the environment) it ran in; ``calls``: the policy calls the schedule took."""


def rollout_refill(adapter, envs, jobs, episode_len) -> RefillResult:
    """Runs every job of the queue ``jobs`` to completion on the host environments ``envs``, one slot per environment
    and ONE policy call per loop iteration for all slots.  Job ``e`` starts in slot ``e``; after every iteration the
    slots are scanned in ascending order and each slot whose episode ended (its environment terminated or truncated, or
    the episode reached ``episode_len`` steps) takes the next queued job: it is reset and passed as ``restart`` in the
    next iteration's policy call, in which the other slots step.  With the queue empty a finished slot idles.  The
    number of policy calls is the makespan of that list schedule, not the sum over waves of the longest episode.

    ``adapter`` ties the loop to a policy: ``obs_dim``; ``observe(o)`` -> the policy's observation row; ``costs(info)``
    -> (the cost the policy is told, the cost summed into the result); ``act(obs, reward, cost, step, restart, jobs)``
    -> actions ``[N, ..]``, where ``step`` / ``restart`` are bool ``[N]`` masks and ``jobs[e]`` is the queue entry of a
    restarting slot (None elsewhere)."""
    return _refill(adapter, envs, jobs, episode_len, None)


def _refill(adapter, envs, jobs, episode_len, rec) -> RefillResult:
    """``rollout_refill``'s loop; ``rec`` (None, or a ``JobRecorder``) is shown every transition."""
    envs, jobs = list(envs), list(jobs)
    N, J, EL = len(envs), len(jobs), int(episode_len)
    if J and N == 0:
        raise ValueError("jobs over an empty list of environments")
    ep_ret, ep_len, ep_cost = [0.0] * J, np.zeros(J, np.int64), [0.0] * J
    slot_of = np.full(J, -1, np.int64)
    if J == 0:
        return RefillResult(np.asarray(ep_ret), ep_len, np.asarray(ep_cost), slot_of, 0)
    obs = np.zeros((N, adapter.obs_dim), np.float32)
    reward, cost = np.zeros(N, np.float64), np.zeros(N, np.float64)
    active, restart = np.zeros(N, bool), np.zeros(N, bool)
    job_in = [-1] * N
    queued = 0

    def take(e):
        nonlocal queued
        q, queued = queued, queued + 1
        job_in[e], slot_of[q] = q, e
        o, _ = envs[e].reset()
        obs[e] = adapter.observe(o)
        active[e] = restart[e] = True
        if rec is not None:
            rec.start(q, o)

    for e in range(min(N, J)):
        take(e)
    calls = 0
    while active.any():
        act = adapter.act(obs, reward, cost, active & ~restart, restart.copy(),
                          [jobs[job_in[e]] if restart[e] else None for e in range(N)])
        calls += 1
        restart[:] = False
        for e in np.flatnonzero(active):
            q = job_in[e]
            o, r, terminated, truncated, info = envs[e].step(act[e])
            told, summed = adapter.costs(info)
            ep_ret[q] += r
            ep_len[q] += 1
            ep_cost[q] += summed
            if rec is not None:
                rec.add(q, act[e], o, r, info["cost"], terminated, truncated or ep_len[q] == EL)
            if terminated or truncated or ep_len[q] == EL:
                active[e] = False
                continue
            obs[e], reward[e], cost[e] = adapter.observe(o), r, told
        for e in range(N):  # ascending: the lowest finished slot takes the earliest queued job
            if not active[e] and queued < J:
                take(e)
    return RefillResult(np.asarray(ep_ret), ep_len, np.asarray(ep_cost), slot_of, calls)


class JobRecorder:
    """What ``collect_refill`` keeps of every job: its transitions under the seven DSRL keys (host lists, one entry per
    step) and its sums.  ``cost_scale`` multiplies the raw cost in the two cost sums only; the recorded costs are raw."""

    def __init__(self, num_jobs: int, gamma: Optional[float] = None, cost_scale: Optional[float] = None):
        J = int(num_jobs)
        self.gamma = 1.0 if gamma is None else float(gamma)
        self.cost_scale = 1.0 if cost_scale is None else cost_scale
        self.rows = [[] for _ in range(J)]  # per job: (obs, action, next obs, reward, cost, terminal, timeout)
        self.cur = [None] * J               # the observation the job's next action answers
        self.ret, self.cret, self.dret, self.dcret = [0.0] * J, [0.0] * J, [0.0] * J, [0.0] * J

    def start(self, q: int, o) -> None:
        self.cur[q] = np.array(o, dtype=np.float32)

    def add(self, q: int, a, o_next, r, cost, terminated, timeout) -> None:
        t = len(self.rows[q])
        o_next = np.array(o_next, dtype=np.float32)
        self.rows[q].append((self.cur[q], np.array(a, dtype=np.float32), o_next, r, cost, bool(terminated), bool(timeout)))
        self.cur[q] = o_next
        pw, c = self.gamma ** t, cost * self.cost_scale
        self.ret[q] += r
        self.cret[q] += c
        self.dret[q] += pw * float(r)
        self.dcret[q] += pw * float(c)

    def dataset(self):
        """The rows job-major (job 0's, then job 1's, ..., each with its true length) as fp32 numpy arrays."""
        rows = [x for job in self.rows for x in job]
        n = len(rows)
        col = lambda i, w: (np.stack([x[i] for x in rows]).astype(np.float32).reshape((n,) + w) if n  # noqa: E731
                            else np.zeros((0,) + w, np.float32))
        od = () if not n else rows[0][0].shape
        ad = () if not n else rows[0][1].shape
        return {"observations": col(0, od), "actions": col(1, ad), "next_observations": col(2, od),
                "rewards": col(3, ()), "costs": col(4, ()), "terminals": col(5, ()), "timeouts": col(6, ())}


CollectedJobs = namedtuple("CollectedJobs", "dataset returns cost_returns lengths disc_returns disc_cost_returns refill")
CollectedJobs.__doc__ = """What ``collect_refill`` returns: ``dataset`` (numpy, on the host, job-major), the per-job sums in
fp64 (``Collected``'s fields) and the ``RefillResult`` of the schedule."""


def collect_refill(adapter, envs, jobs, episode_len, gamma: Optional[float] = None, cost_scale=None) -> CollectedJobs:
    """``rollout_refill`` recorded: the same schedule, the same calls of ``adapter`` (which adds whatever noise it is
    built to add), and of every job its transitions under the seven DSRL keys -- ``observations`` /
    ``next_observations`` are the environment's own (not ``adapter.observe``'s row), ``actions`` the bits the policy
    call returned, ``costs`` the raw ``info["cost"]``, ``terminals`` 1 where the environment terminated, ``timeouts`` 1
    where it truncated or the episode reached ``episode_len`` -- plus return, cost return (times ``cost_scale``), length
    and the two sums weighted by ``gamma ** t`` in fp64.  The rows are job-major with each job's true length: the layout
    depends neither on ``len(envs)`` nor on the slot a job ran in."""
    jobs = list(jobs)
    rec = JobRecorder(len(jobs), gamma, cost_scale)
    res = _refill(adapter, envs, jobs, episode_len, rec)
    f = lambda x: np.asarray(x, dtype=np.float64)  # noqa: E731
    return CollectedJobs(rec.dataset(), f(rec.ret), f(rec.cret), res.lengths.astype(np.float64), f(rec.dret),
                         f(rec.dcret), res)


def check_job_noise(num_jobs, episode_len, action_dim, noise_std, noise, episode_ids):
    """``collect_jobs``'s per-job arguments, checked on the host: sigma ``[J]`` fp32 (one value or one per job), the
    injected noise ``[J, episode_len, action_dim]`` fp32 or None, the episode ids ``[J]`` (default ``0 .. J - 1``)."""
    J = int(num_jobs)
    if J < 0:
        raise ValueError(f"num_jobs must not be negative, got {J}")
    if torch.is_tensor(noise_std):
        noise_std = noise_std.detach().cpu().numpy()
    sg = np.asarray(noise_std, dtype=np.float32)
    if sg.ndim != 0 and sg.shape != (J,):
        raise ValueError(f"noise_std holds {sg.size} values, the queue {J} jobs")
    sg = np.ascontiguousarray(np.broadcast_to(sg, (J,)))
    if noise is not None:
        if torch.is_tensor(noise):
            noise = noise.detach().cpu().numpy()
        noise = np.asarray(noise, dtype=np.float32)
        if noise.shape != (J, int(episode_len), int(action_dim)):
            raise ValueError(f"noise must be [{J}, {int(episode_len)}, {int(action_dim)}] (jobs, episode_len, "
                             f"action_dim), got {noise.shape}")
    if episode_ids is None:
        ids = np.arange(J, dtype=np.int64)
    else:
        if np.shape(episode_ids) != (J,):
            raise ValueError(f"expected episode_ids of shape ({J},), got {np.shape(episode_ids)}")
        ids = np.asarray(episode_ids)
        if ids.dtype.kind not in "iu" or (ids < 0).any() or (ids > 0x7FFFFFFF).any():
            raise ValueError("expected episode_ids as integers in 0 .. 2^31 - 1")
    return sg, noise, ids


def check_jobs_store(into, num_jobs, episode_len, state_dim, action_dim) -> None:
    """``collect_jobs(into=)``, before the run: a ``SequenceStore`` must have room for ``num_jobs`` trajectories of
    ``episode_len`` rows (the lengths are not known in advance, and the run must not be lost); a ``ReplayStore`` under
    ``collect``'s rules."""
    from ..common.replay import SequenceStore
    from .collect import _check_replay_store
    if isinstance(into, SequenceStore):
        into.check_append(int(num_jobs), int(num_jobs) * int(episode_len), observations=state_dim, actions=action_dim)
    else:
        _check_replay_store(into, state_dim, action_dim)


def finish_jobs(got: CollectedJobs, device, into):
    """The host rows as a ``Collected``: ONE upload of all seven tables, then views of it as the dataset, or the store's
    ``append``."""
    from .collect import KEYS, Collected
    d = got.dataset
    flat = np.concatenate([d[k].reshape(-1) for k in KEYS]) if d["rewards"].size else np.zeros(0, np.float32)
    dev = torch.from_numpy(flat).to(device)
    data, off = {}, 0
    for k in KEYS:
        data[k] = dev[off:off + d[k].size].view(d[k].shape)
        off += d[k].size
    if into is not None:
        into.append(data)
        data = None
    return Collected(data, got.returns, got.cost_returns, got.lengths, got.disc_returns, got.disc_cost_returns)


class MLPRefillAdapter:
    """``rollout_refill`` over ``model.fast_policy(num_envs)`` of an MLP model: a job is an episode id (the key, with
    the step, of the noise the policy draws on the device)."""

    def __init__(self, model, num_envs, cost_scale=None, append=None):
        self.pol = model.fast_policy(num_envs=num_envs)
        self.obs_dim, self.cost_scale, self.append = self.pol.obs_dim, cost_scale, append

    def observe(self, o):
        return o if self.append is None else np.append(o, self.append)

    def costs(self, info):
        return 0.0, info["cost"] if self.cost_scale is None else info["cost"] * self.cost_scale

    def act(self, obs, reward, cost, step, restart, jobs):
        ids = np.asarray([0 if j is None else j for j in jobs], dtype=np.int64)
        return self.pol.step(obs, active=step, restart=restart, episode_ids=ids)[0]


class PlanRefillAdapter:
    """``rollout_refill`` over a ``ModelPlanner`` (engine/mpc.py): every policy call is one ``planner.act`` on the slots'
    current states, each slot with the budget its episode has left -- ``max(cost_limit * cost_scale - cost so far, 0)``,
    the cost so far accumulated here in the planner's ``cost_scale`` units.  A slot that idles is fed its last state and
    its action is ignored.  ``budgets`` / ``restarts``: per call the ``[N]`` budgets passed and the slots that started an
    episode in it (host copies, for inspection)."""

    def __init__(self, planner, cost_limit, cost_scale=None):
        self.planner, self.obs_dim, self.cost_scale = planner, planner.venv.state_dim, cost_scale
        self.limit = float(cost_limit) * (1.0 if cost_scale is None else float(cost_scale))
        self.so_far = np.zeros(planner.num_envs, np.float64)
        self.budgets, self.restarts = [], []

    def observe(self, o):
        return o

    def costs(self, info):
        c = info["cost"] if self.cost_scale is None else info["cost"] * self.cost_scale
        return c, c

    def act(self, obs, reward, cost, step, restart, jobs):
        self.so_far[restart] = 0.0
        self.so_far[step] += cost[step]
        budget = np.maximum(self.limit - self.so_far, 0.0).astype(np.float32)
        self.budgets.append(budget.copy())
        self.restarts.append(restart.copy())
        return self.planner.act(obs, budget)


def evaluate_planned(planner, envs, eval_episodes, cost_limit, episode_len, cost_scale=None):
    """``eval_episodes`` episodes over the host environments ``envs`` on the refill schedule, every action planned
    (``PlanRefillAdapter``).  Returns the means (return, cost sum, length), not rescaled, and the adapter."""
    envs = list(envs)
    if len(envs) != planner.num_envs:
        raise ValueError(f"the planner holds {planner.num_envs} slots, evaluate_planned was given {len(envs)} environments")
    if int(eval_episodes) < 1:
        raise ValueError(f"eval_episodes {eval_episodes}: at least one episode")
    adapter = PlanRefillAdapter(planner, cost_limit, cost_scale)
    res = _refill(adapter, envs, list(range(int(eval_episodes))), episode_len, None)
    return (np.mean(res.returns), np.mean(res.costs), np.mean(res.lengths)), adapter


class MLPCollectAdapter(MLPRefillAdapter):
    """``MLPRefillAdapter`` with the exploration tail: a job is ``(q, episode id, sigma)``; ``noise`` (None, or ``[J,
    episode_len, act_dim]``) is injected instead of the draw keyed by ``(seed, episode id, step, column)``."""

    def __init__(self, model, num_envs, cost_scale=None, append=None, seed: int = 0, noise=None):
        super().__init__(model, num_envs, cost_scale, append)
        N = self.pol.num_envs
        self.seed, self.noise = int(seed), noise
        self.ids, self.sigma = np.zeros(N, np.int64), np.zeros(N, np.float32)
        self.job, self.t = np.zeros(N, np.int64), np.zeros(N, np.int64)
        self.eps = None if noise is None else np.zeros((N, self.pol.act_dim), np.float32)

    def act(self, obs, reward, cost, step, restart, jobs):
        for e, j in enumerate(jobs):
            if j is not None:
                self.job[e], self.ids[e], self.sigma[e] = j
                self.t[e] = -1
        run = step | restart
        self.t[run] += 1
        if self.eps is not None:
            self.eps[run] = self.noise[self.job[run], self.t[run]]
        return self.pol.step(obs, active=step, restart=restart, episode_ids=self.ids, explore_std=self.sigma,
                             explore_seed=self.seed, explore_noise=self.eps)[0]


def collect_jobs_mlp(model, envs, num_jobs, noise_std=0.0, gamma=None, seed: int = 0, noise=None, episode_ids=None,
                     into=None, cost_scale=None, append=None):
    """``RolloutMixin.collect_jobs``: ``rollout_jobs_mlp``'s queue through ``collect_refill`` with the exploration tail of
    ``VecFastPolicy.step``.  Returns a ``Collected``."""
    envs = list(envs)
    J = int(num_jobs)
    kind, obs_dim, _, _ = model._policy_spec()
    state_dim = obs_dim - (0 if append is None else 1)
    sg, noise, ids = check_job_noise(J, model.episode_len, model.action_dim, noise_std, noise, episode_ids)
    check_jobs_store(into, J, model.episode_len, state_dim, model.action_dim)
    if J and not envs:
        raise ValueError("jobs over an empty list of environments")
    if J == 0:
        got = collect_refill(None, envs, [], model.episode_len, gamma, cost_scale)
        d = got.dataset
        d["observations"] = d["next_observations"] = np.zeros((0, state_dim), np.float32)
        d["actions"] = np.zeros((0, model.action_dim), np.float32)
    else:
        adapter = MLPCollectAdapter(model, len(envs), cost_scale, append, seed, noise)
        got = collect_refill(adapter, envs, [(q, int(ids[q]), float(sg[q])) for q in range(J)], model.episode_len,
                             gamma, cost_scale)
    return finish_jobs(got, model.device, into)


def rollout_jobs_mlp(model, envs, num_jobs, episode_ids=None, cost_scale=None, append=None) -> RefillResult:
    """``num_jobs`` episodes over the host environments ``envs`` on the refill schedule (``rollout_refill``); job ``q``
    carries episode id ``episode_ids[q]`` (default ``q``)."""
    J = int(num_jobs)
    if episode_ids is None:
        ids = np.arange(J, dtype=np.int64)
    else:
        if np.shape(episode_ids) != (J,):
            raise ValueError(f"expected episode_ids of shape ({J},), got {np.shape(episode_ids)}")
        ids = np.asarray(episode_ids)
        if ids.dtype.kind not in "iu" or (ids < 0).any() or (ids > 0x7FFFFFFF).any():
            raise ValueError("expected episode_ids as integers in 0 .. 2^31 - 1")
    envs = list(envs)
    if J and not envs:
        raise ValueError("jobs over an empty list of environments")
    if J == 0:
        return rollout_refill(None, envs, [], model.episode_len)
    return rollout_refill(MLPRefillAdapter(model, len(envs), cost_scale, append), envs, [int(i) for i in ids],
                          model.episode_len)


def evaluate_refill(trainer, eval_episodes):
    """``evaluate_lockstep`` on the refill schedule: episode ``q`` (episode id ``q``) is job ``q`` of one queue over the
    environments ``trainer.env``.  Returns the means (return, cost sum, length), not rescaled."""
    if len(list(trainer.env)) == 0:
        raise ValueError("evaluate over an empty list of environments")
    trainer.model.eval()
    res = trainer.rollout_jobs(list(trainer.env), int(eval_episodes))
    trainer.model.train()
    return np.mean(res.returns), np.mean(res.costs), np.mean(res.lengths)
