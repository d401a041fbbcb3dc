"""Host side of the CDT act latency path (csrc/cdt_act.hip, include/osrl_amd.h ``osrl_cdt_policy_*``).

``CDTTrainer.rollout`` (cdt.py:436-518) on a host environment asks for one action per env step over the window of the
last ``seq_len`` timesteps.  ``CDTFastPolicy`` keeps that window on the device, with every token's cached hidden state:
``reset`` / ``step`` write the observation into a pinned, device-mapped block through a numpy view, make one C call
(the step's launch chain + a spin on the published sequence number) and read the action back through another view.
Window updates use the existing loop's fp32 expressions (``returns - float(reward)``, ``costs - cost``), on device.

The kernels read the packed forward weight copies and the biases of the model's flat group -- the buffers the fused
AdamW step, ``load_state_dict`` and ``repack()`` keep current -- so training between evaluations needs no rebuild.

``CDTVecFastPolicy`` is the same for ``num_envs`` episodes on as many host environments, advanced by one C call per env
step (``osrl_cdt_policy_*_n``): the step's launches run over the rows of all the episodes, and an episode's actions do
not depend on how many ran beside it.  The slots run in lockstep (``reset`` starts all of them) or, once a slot has been
restarted on its own (``step(..., restart=mask)``, ``osrl_cdt_policy_step_slots``), each at its own timestep: a finished
slot takes a new episode while the others go on, and an inactive slot costs no device rows.  ``step(explore_std=...)`` /
``step(sample=True)`` end the head launch in the collectors' exploration tail (``CDTTrainer.collect_jobs``).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np

from .. import _lib as L
from .act import PinnedHandle, _vec_args

MAX_TOKENS, MAX_E, MAX_HEAD_DIM = 256, 512, 128
MAX_ENVS = L.CDT_POLICY_MAX_ENVS


def unsupported(model) -> Optional[str]:
    """Why ``model`` is outside the fast path's domain (None: inside)."""
    S = model.seq_repeat * model.seq_len + int(model.cost_prefix)
    if S > MAX_TOKENS:
        return f"{S} tokens per sequence > {MAX_TOKENS} (seq_repeat * seq_len + cost_prefix)"
    if model.embedding_dim > MAX_E:
        return f"embedding_dim {model.embedding_dim} > {MAX_E}"
    if model.embedding_dim // model.num_heads > MAX_HEAD_DIM:
        return f"head_dim {model.embedding_dim // model.num_heads} > {MAX_HEAD_DIM}"
    if model.action_head_layers > L.MAX_LAYERS:
        return f"action_head_layers {model.action_head_layers} > {L.MAX_LAYERS}"
    if 2 * model.action_dim > 1024:
        return f"action_dim {model.action_dim} > 512"
    return None


def _descriptor(m) -> Tuple["L.CdtPolicyT", object]:
    """The C descriptor of ``m`` and its per-layer array: device pointers into the model's flat group."""
    g = m.groups["cdt"]
    pk = lambda key: g.pf.data_ptr() + 4 * g.f_off[key]  # noqa: E731  packed forward copy
    cv = lambda key: g.view(key).data_ptr()  # noqa: E731  canonical tensor
    d = L.CdtPolicyT()
    d.state_dim, d.action_dim, d.seq_len = m.state_dim, m.action_dim, m.seq_len
    d.embedding_dim, d.num_layers, d.num_heads = m.embedding_dim, m.num_layers, m.num_heads
    d.use_rew, d.use_cost, d.cost_prefix = int(m.use_rew), int(m.use_cost), int(m.cost_prefix)
    d.cost_transform = int(m.cost_transform_on)
    d.add_cost_feat, d.mul_cost_feat, d.cat_cost_feat = int(m.add_cost_feat), int(m.mul_cost_feat), int(m.cat_cost_feat)
    chain = list(m.head_hidden_keys) + [m.head_out_key]
    d.head_layers = len(chain)
    d.head_out_width = 2 * m.action_dim if m.stochastic else m.action_dim
    d.max_action = float(m.max_action)
    if m.time_emb:
        d.te = cv("cdt.timestep_emb.weight")
        d.te_rows = g.layout["cdt.timestep_emb.weight"][1][0]
    d.state_w, d.state_b = cv("cdt.state_emb.weight"), cv("cdt.state_emb.bias")
    d.action_w, d.action_b = cv("cdt.action_emb.weight"), cv("cdt.action_emb.bias")
    if m.use_rew:
        d.return_w, d.return_b = cv("cdt.return_emb.weight"), cv("cdt.return_emb.bias")
    if m.use_cost:
        d.cost_w, d.cost_b = cv("cdt.cost_emb.weight"), cv("cdt.cost_emb.bias")
    if m.cost_prefix:
        d.prefix_w, d.prefix_b = cv("cdt.prefix_emb.weight"), cv("cdt.prefix_emb.bias")
    d.emb_g, d.emb_b = cv("cdt.emb_norm.weight"), cv("cdt.emb_norm.bias")
    d.out_g, d.out_b = cv("cdt.out_norm.weight"), cv("cdt.out_norm.bias")
    for i, key in enumerate(chain):
        d.head_w[i], d.head_b[i] = pk(key), cv(key[:-len("weight")] + "bias")
    layers = (L.CdtLayerT * m.num_layers)()
    for l in range(m.num_layers):
        p, y = f"cdt.blocks.{l}.", layers[l]
        y.ln1_g, y.ln1_b = cv(p + "norm1.weight"), cv(p + "norm1.bias")
        y.w_qkv, y.b_qkv = pk(p + "attention.in_proj_weight"), cv(p + "attention.in_proj_bias")
        y.w_o, y.b_o = pk(p + "attention.out_proj.weight"), cv(p + "attention.out_proj.bias")
        y.ln2_g, y.ln2_b = cv(p + "norm2.weight"), cv(p + "norm2.bias")
        y.w_1, y.b_1 = pk(p + "mlp.0.weight"), cv(p + "mlp.0.bias")
        y.w_2, y.b_2 = pk(p + "mlp.2.weight"), cv(p + "mlp.2.bias")
    return d, layers


class _CDTHandle(PinnedHandle):
    """What the one-episode and the lockstep policy share: the handle of ``model`` and the window read-back."""

    DESTROY = "osrl_cdt_policy_destroy"

    def _create(self, model, entry: str, *width):
        why = unsupported(model)
        if why is not None:
            raise NotImplementedError("the CDT act latency path does not support: " + why)
        m = self.model = model
        d, layers = _descriptor(m)
        lib = self._open(m.device, entry, C.byref(d), layers, *width)
        self.od, self.ad, self.T = m.state_dim, m.action_dim, m.seq_len
        self._t, self._episode_len = -1, 0
        self._te_rows = int(d.te_rows) if m.time_emb else None
        return lib

    def _window(self, entry: str, *env) -> Dict[str, np.ndarray]:
        T, od, ad = self.T, self.od, self.ad
        s, a = np.zeros((T, od), np.float32), np.zeros((T, ad), np.float32)
        r, c, ts = np.zeros(T, np.float32), np.zeros(T, np.float32), np.zeros(T, np.int64)
        n = C.c_int32(0)
        f = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
        L.check(getattr(self._lib, entry)(self._h, *env, f(s), f(a), f(r), f(c), f(ts), C.byref(n), self._stream()),
                entry)
        k = n.value
        return dict(states=s[:k].copy(), actions=a[:k].copy(), returns=r[:k].copy(), costs=c[:k].copy(),
                    time_steps=ts[:k].copy())


class CDTFastPolicy(_CDTHandle):
    def __init__(self, model):
        lib = self._create(model, "osrl_cdt_policy_create")
        ptrs = [C.POINTER(C.c_float)() for _ in range(3)]
        L.check(lib.osrl_cdt_policy_io(self._h, *[C.byref(p) for p in ptrs]), "osrl_cdt_policy_io")
        od, ad = self.od, self.ad
        self._obs = np.ctypeslib.as_array(ptrs[0], shape=(od,))  # numpy views of PINNED memory
        self._act_in = np.ctypeslib.as_array(ptrs[1], shape=(ad,))
        self._act_out = np.ctypeslib.as_array(ptrs[2], shape=(ad,))

    def _put_obs(self, obs) -> None:
        if np.shape(obs) != self._obs.shape:  # numpy would broadcast a scalar silently
            raise ValueError(f"expected one observation of shape {self._obs.shape}, got {np.shape(obs)}")
        self._obs[:] = obs  # float32 (round to nearest), as torch.as_tensor(obs) written into the fp32 window

    def reset(self, obs, target_return: float, target_cost: float) -> np.ndarray:
        """Starts an episode (cdt.py:470-478) and returns the first action."""
        if self._h is None:
            raise RuntimeError("CDTFastPolicy is closed")
        self._episode_len = int(self.model.episode_len)
        self.model.repack()  # in-place edits of the parameters since the last step (CDT.forward does the same)
        self._put_obs(obs)
        self._t = 0
        rc = self._lib.osrl_cdt_policy_reset(self._h, float(target_return), float(target_cost), self._stream())
        if rc != 0:
            self._t = -1
            L.check(rc, "osrl_cdt_policy_reset")
        return self._act_out.copy()

    def step(self, obs, reward, cost, action=None) -> np.ndarray:
        """Records the action taken at the previous step (``action``, default: the one returned), the new observation
        and that step's reward and cost (``info["cost"] * cost_scale``, or its cost_reverse form); returns the next
        action."""
        if self._t < 0:
            raise RuntimeError("call reset() before step()")
        if self._t + 1 >= self._episode_len:
            raise RuntimeError(f"the episode is over: {self._episode_len} steps (model.episode_len)")
        self._put_obs(obs)
        host = 0
        if action is not None:
            if np.shape(action) != self._act_in.shape:
                raise ValueError(f"expected one action of shape {self._act_in.shape}, got {np.shape(action)}")
            self._act_in[:] = action
            host = 1
        rc = self._lib.osrl_cdt_policy_step(self._h, float(reward), float(cost), host, self._stream())
        if rc != 0:
            L.check(rc, "osrl_cdt_policy_step")
        self._t += 1
        return self._act_out.copy()

    def window(self) -> Dict[str, np.ndarray]:
        """numpy copies of the current window (oldest timestep first), as the model saw it for the last action."""
        return self._window("osrl_cdt_policy_window")


class CDTVecFastPolicy(_CDTHandle):
    """``num_envs`` episodes on as many host environments, one C call per env step for all of them.  A slot's actions
    are those a ``CDTFastPolicy`` returns for the same inputs, bit for bit, whatever ``num_envs`` is and whatever the
    other slots are doing.

    Lockstep (the default): ``reset`` starts all slots and ``step`` advances all of them, so they share the timestep.
    A slot whose episode has ended is passed as inactive (``active[e] = False``): its rows of ``obs / reward / cost /
    action`` are not read and its row of the result is zero.  Its device rows keep running on the stale inputs of its
    last active step (the launches cover every slot); nothing of that reaches the other slots.

    Independent slots: ``step(..., restart=mask)`` starts a new episode in the masked slots, at timestep 0, while the
    others step.  From the first such call until the next ``reset`` every slot has its own timestep (``timesteps``) and
    episode length, and an inactive slot is FROZEN: it runs no device rows, its timestep does not advance, and a later
    call continues it where it stood."""

    LIMIT = (MAX_ENVS, "OSRL_CDT_POLICY_MAX_ENVS")

    def __init__(self, model, num_envs: int):
        N = self.num_envs = _vec_args(num_envs, *self.LIMIT)
        lib = self._create(model, "osrl_cdt_policy_create_n", N)
        ptrs = [C.POINTER(C.c_float)() for _ in range(4)]
        L.check(lib.osrl_cdt_policy_io_n(self._h, *[C.byref(p) for p in ptrs]), "osrl_cdt_policy_io_n")
        od, ad = self.od, self.ad
        self._obs = np.ctypeslib.as_array(ptrs[0], shape=(N, od))  # numpy views of PINNED memory
        self._act_in = np.ctypeslib.as_array(ptrs[1], shape=(N, ad))
        self._act_out = np.ctypeslib.as_array(ptrs[2], shape=(N, ad))
        self._scalars = np.ctypeslib.as_array(ptrs[3], shape=(N, 4))  # reward, cost, target_return, target_cost
        xp = [C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_float)()]
        L.check(lib.osrl_cdt_policy_explore_io(self._h, *[C.byref(p) for p in xp]), "osrl_cdt_policy_explore_io")
        self._sigma = np.ctypeslib.as_array(xp[0], shape=(N,))       # exploration scale of each slot
        self._eps = np.ctypeslib.as_array(xp[1], shape=(N, ad))      # injected exploration noise
        self._episode_id = np.ctypeslib.as_array(xp[2], shape=(N,))  # the episode word of the noise key
        self._head = np.ctypeslib.as_array(xp[3], shape=(N, 2 * ad))  # (mu | log_std) of a sampling call
        self.last_head = None

    # Per-slot state lives beside the scalars ``_t`` / ``_episode_len``: ``_ts`` / ``_els`` ([N] arrays) and ``_slots``
    # (True once a slot has been restarted on its own).  In lockstep the scalars are every slot's; with independent
    # slots ``_t`` is the furthest slot's timestep and ``_episode_len`` the length read at the latest (re)start.
    def _slot_state(self) -> Tuple[np.ndarray, np.ndarray]:
        if not self.__dict__.get("_slots", False):
            N = self.num_envs
            return np.full(N, self._t, np.int64), np.full(N, self._episode_len, np.int64)
        return self._ts, self._els

    @property
    def timesteps(self) -> np.ndarray:
        """``[N]`` integers: the timestep of each slot's newest window entry, -1 for a slot never started."""
        return self._slot_state()[0].copy()

    def _target(self, name, x) -> np.ndarray:
        if np.ndim(x) != 0 and np.shape(x) != (self.num_envs,):
            raise ValueError(f"expected {name} as a scalar or of shape ({self.num_envs},), got shape {np.shape(x)}")
        return np.broadcast_to(np.asarray(x, dtype=np.float64), (self.num_envs,))

    def _mask(self, name, x) -> np.ndarray:
        x = self._rows(name, x, ())
        if x.dtype != np.bool_:
            raise ValueError(f"expected {name} as booleans, got dtype {x.dtype}")
        return x

    def reset(self, obs, target_return, target_cost) -> np.ndarray:
        """Starts ``num_envs`` episodes from ``obs [N, state_dim]``; the targets are scalars or one per slot.  Returns
        the first actions ``[N, action_dim]``.  The slots are in lockstep again from here."""
        if self._h is None:
            raise RuntimeError("CDTVecFastPolicy is closed")
        obs = self._rows("obs", obs, (self.od,))
        tr, tc = self._target("target_return", target_return), self._target("target_cost", target_cost)
        self._episode_len = int(self.model.episode_len)
        self.model.repack()  # in-place edits of the parameters since the last step (CDT.forward does the same)
        self._obs[:] = obs  # float32 (round to nearest), as torch.as_tensor(obs) written into the fp32 window
        self._scalars[:, 2] = tr  # float(target) -> fp32, as the one-episode call's float arguments
        self._scalars[:, 3] = tc
        self._t, self._slots = 0, False
        rc = self._lib.osrl_cdt_policy_reset_n(self._h, self._stream())
        if rc != 0:
            self._t = -1
            L.check(rc, "osrl_cdt_policy_reset_n")
        return self._act_out.copy()

    def step(self, obs, reward, cost, action=None, active=None, restart=None, target_return=None,
             target_cost=None, explore_std=None, sample: bool = False, explore_seed: int = 0, explore_noise=None,
             episode_ids=None) -> np.ndarray:
        """Per slot as ``CDTFastPolicy.step``: ``obs [N, state_dim]``, ``reward [N]``, ``cost [N]``, the actions taken at
        the previous step (``action [N, action_dim]``, default: the ones returned) and ``active`` (bool ``[N]``, default:
        all).  Returns the next actions ``[N, action_dim]``, zero in the rows of inactive slots.

        ``restart`` (bool ``[N]``): the masked slots begin a new episode at timestep 0 from ``obs[e]`` with
        ``target_return`` / ``target_cost`` (scalars or ``[N]``; required when any slot restarts) instead of stepping:
        their ``reward / cost / action`` rows are not read, they count as active, and their row of the result is the
        new episode's first action (what ``reset`` returns for it).

        ``explore_std`` (None: off) or ``sample=True``: the collectors' exploration tail on the returned action,
        ``clip(mu + s * eps)`` with ``s = explore_std`` (one sigma or ``[N]``) or, sampling, the Gaussian head's own
        ``exp(log_std)``; ``s == 0`` returns the evaluating call's bits.  ``eps`` is ``explore_noise [N, action_dim]``
        when given, else drawn in the kernel keyed by ``(explore_seed, the slot's episode id, its timestep, column)`` --
        ``collect_targets``' draw; ``episode_ids`` (``[N]`` integers) gives the restarting slots theirs.  The window
        records the action taken.  After a sampling call ``last_head`` holds ``(mu | log_std) [N, 2 * action_dim]`` (rows
        of slots that did not run are stale).  An exploring call runs the slots independently, as ``restart`` does."""
        N = self.num_envs
        explore = explore_std is not None or bool(sample)
        if not explore and (explore_noise is not None or episode_ids is not None):
            raise ValueError("explore_noise and episode_ids belong to an exploring call: pass explore_std or sample=True")
        if explore:
            sg = np.asarray(0.0 if explore_std is None else explore_std, dtype=np.float32)
            if sg.ndim != 0 and sg.shape != (N,):
                raise ValueError(f"expected explore_std as a scalar or of shape ({N},), got {sg.shape}")
            sg = np.broadcast_to(sg, (N,))
            if explore_noise is not None:
                explore_noise = self._rows("explore_noise", explore_noise, (self.ad,), np.float32)
            if episode_ids is not None:
                episode_ids = self._rows("episode_ids", episode_ids, ())
                if episode_ids.dtype.kind not in "iu" or (episode_ids < 0).any() or (episode_ids > 0x7FFFFFFF).any():
                    raise ValueError("expected episode_ids as integers in 0 .. 2^31 - 1")
            if sample and not self.model.stochastic:
                raise ValueError("sample=True draws from the Gaussian head's own standard deviation: the model was built "
                                 "with stochastic=False")
        if restart is not None:
            restart = self._mask("restart", restart)
            if not restart.any():
                restart = None
        if self._t < 0 and restart is None:
            raise RuntimeError("call reset() before step()")
        slots = restart is not None or explore or self.__dict__.get("_slots", False)
        if not slots and self._t + 1 >= self._episode_len:
            raise RuntimeError(f"the episode is over: {self._episode_len} steps (model.episode_len)")
        obs = self._rows("obs", obs, (self.od,))
        reward, cost = self._rows("reward", reward, ()), self._rows("cost", cost, ())
        if action is not None:
            action = self._rows("action", action, (self.ad,))
        if active is not None:
            active = self._mask("active", active)
        if not slots:
            if active is None:
                self._obs[:] = obs
                self._scalars[:, 0] = reward  # float(reward) -> fp32, as the one-episode call's float arguments
                self._scalars[:, 1] = cost
                if action is not None:
                    self._act_in[:] = action
            else:
                self._obs[active] = obs[active]
                self._scalars[active, 0] = reward[active]
                self._scalars[active, 1] = cost[active]
                if action is not None:
                    self._act_in[active] = action[active]
            rc = self._lib.osrl_cdt_policy_step_n(self._h, 0 if action is None else 1, self._stream())
            if rc != 0:
                L.check(rc, "osrl_cdt_policy_step_n")
            self._t += 1
            out = self._act_out.copy()
            if active is not None:
                out[~active] = 0.0
            return out
        # independent slots
        rs = np.zeros(N, bool) if restart is None else restart
        if rs.any():
            if target_return is None or target_cost is None:
                raise ValueError("target_return and target_cost are required when a slot restarts")
            tr, tc = self._target("target_return", target_return), self._target("target_cost", target_cost)
        st = (np.ones(N, bool) if active is None else active) & ~rs
        ts, els = self._slot_state()
        te = self.__dict__.get("_te_rows")
        for e in np.flatnonzero(st):
            if ts[e] < 0:
                raise RuntimeError(f"slot {e}: no episode was started (call reset(), or restart the slot)")
            if ts[e] + 1 >= els[e]:
                raise RuntimeError(f"slot {e}: the episode is over: {els[e]} steps (model.episode_len)")
            if te is not None and ts[e] + 1 >= te:
                raise RuntimeError(f"slot {e}: timestep {ts[e] + 1} is past the timestep embedding table ({te} rows)")
        if self._h is None:
            raise RuntimeError("CDTVecFastPolicy is closed")
        ts, els = ts.copy(), els.copy()
        if rs.any():
            els[rs] = self._episode_len = int(self.model.episode_len)
            self.model.repack()  # as reset()
            self._scalars[rs, 2] = tr[rs]
            self._scalars[rs, 3] = tc[rs]
        run = st | rs
        self._obs[run] = obs[run]
        self._scalars[st, 0] = reward[st]
        self._scalars[st, 1] = cost[st]
        if action is not None:
            self._act_in[st] = action[st]
        mode = np.where(rs, 2, np.where(st, 1, 0)).astype(np.int32)
        if explore:
            self._sigma[run] = sg[run]
            if explore_noise is not None:
                self._eps[run] = explore_noise[run]
            if episode_ids is not None:
                self._episode_id[rs] = episode_ids[rs]
            rc = self._lib.osrl_cdt_policy_step_slots_explore(
                self._h, mode.ctypes.data_as(C.POINTER(C.c_int32)), 0 if action is None else 1, 1 if sample else 0,
                int(explore_seed) & 0xFFFFFFFFFFFFFFFF, 0 if explore_noise is None else 1, self._stream())
            if rc != 0:
                L.check(rc, "osrl_cdt_policy_step_slots_explore")
            if sample:
                self.last_head = self._head.copy()
        else:
            rc = self._lib.osrl_cdt_policy_step_slots(self._h, mode.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      0 if action is None else 1, self._stream())
            if rc != 0:
                L.check(rc, "osrl_cdt_policy_step_slots")
        ts[st] += 1
        ts[rs] = 0
        self._ts, self._els, self._slots = ts, els, True
        self._t = int(ts.max())
        out = self._act_out.copy()
        out[~run] = 0.0
        return out

    def window(self, env: int) -> Dict[str, np.ndarray]:
        """numpy copies of slot ``env``'s current window (oldest timestep first)."""
        if not 0 <= int(env) < self.num_envs:
            raise ValueError(f"env {env} is outside 0 .. {self.num_envs - 1}")
        return self._window("osrl_cdt_policy_window_n", int(env))
