"""A fitted ensemble dynamics model (algorithms/dynamics.py) stepped on device as a vector environment.

``ModelVecEnv`` has ``VecSyntheticSafeEnv``'s interface -- ``E``, ``state_dim``, ``episode_len``, ``state``, ``acc``,
``desc``, ``reset``, ``step`` -- so ``BatchedRollout`` and ``CDTBatchedRollout`` (engine/rollout.py) drive it unchanged:
``evaluate`` of all six trainers, CDT's ``evaluate_targets`` grid included, on the dynamics a dataset describes.  One HIP
launch per environment step for all episodes (csrc/model_env.hip); the model's packed weights are read in place, so the
environment follows ``DynamicsTrainer`` steps as rollouts follow a policy.

What comes out is a model's opinion: its error grows with the rollout length and with the shift between the policy and the
data.  ``disagreement()`` -- how far the members' predictions lie apart along each episode -- is the trust signal.

Recording: ``collect`` / ``collect_targets`` refuse a ``ModelVecEnv``; ``Trainer.collect_model(menv, ...)`` (engine/collect.py
``ModelCollector``, csrc/model_env.hip ``osrl_model_env_collect``) records the policy's rollouts on it, k steps from the
initial states or from rows of a store, with the penalised reward.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from .synthetic_env import DeviceVecEnv


class ModelVecEnv(DeviceVecEnv):
    """``episodes`` episodes of ``model`` in HBM: ``state [E, od]``, ``acc [E, 4] = (return, cost * cost_scale, length,
    done)`` and ``unc [E, 2] = (max, sum over the steps taken)`` of the members' disagreement.

    ``init_states``: ``[n, od]`` rows (tensor or array) or a ``ReplayStore(state_init=True)``, whose initial observations
    are taken; episode ``e`` starts at row ``(base_seed + e) % n``.  ``mode``: "mean" follows the ensemble mean, "member"
    follows member ``member``, "random" a member drawn per episode and step from ``seed`` (Philox keyed by the episode id
    ``base_seed + e`` and the episode's own step).  ``reward_penalty`` lambda: ``r -= lambda * disagreement`` (MOPO).
    ``clip_states``: next states are clamped to the model's ``s_lo`` / ``s_hi``.  ``seed`` lives in device memory and
    may be set between runs; ``mode``, ``member`` and ``reward_penalty`` are launch arguments: changing them moves
    ``launch_epoch``, on which a rollout drops its captured graph.

    On a ``Dynamics(probabilistic=True)`` the step is ``osrl_model_env_step_gauss``.  ``sample``: the next state and the
    reward are drawn from the followed member's Gaussian (mode "mean": the mean of the members' variances), the noise a
    function of (``seed``, episode id, step, column) -- Philox stream 16 -- or ``set_noise_in``'s.  ``uncertainty``:
    "disagreement" (the spread of the means) or "max_std", MOPO's ``max_m sqrt(mean_k sigma_m[k]^2)``; the one in use is
    what ``reward_penalty`` weighs and what ``unc`` / ``disagreement()`` report.  Both are launch arguments too; on a
    deterministic model either raises a ``ValueError``.  With the defaults such a model steps bit for bit like a
    deterministic one that holds its members' first ``od + 2`` output rows.

    Pessimism beyond the reward (the ``_halt`` entry points; DESIGN.md "Halting on uncertainty").  ``halt_threshold``
    (None: never): where the signal in use exceeds it the episode ends at that step -- MOReL's absorbing "unknown" -- with
    ``halt_reward`` in the reward's place and ``halt_cost`` (0 or 1) as the cost; ``halt_step`` (int32 ``[E]`` on the
    device, -1: not halted; ``halted()``) keeps the step.  ``cost_penalty`` kappa: the cost bit is
    ``c + kappa * u > 0.5`` (CAP's inflation).  All four are launch arguments.  With the defaults ``desc()`` hands out the
    plain descriptors and the plain entry points run.

    Elites.  On a ``Dynamics(num_elites=k)`` the environment steps the model's elite members only
    (``model.elite_members()``, ascending): the descriptor holds those k nets and ``n_models = k``, so the mean, the spread,
    ``max_std``, mode "random"'s draw (mod k) and the halting range over the elites.  ``member`` stays a MODEL index and
    must be an elite in mode "member" (ValueError when the descriptor is built); ``set_member_in`` takes POSITIONS in
    ``[0, k)``.  ``model.set_elites`` moves ``launch_epoch`` like a launch argument does."""

    def __init__(self, model, init_states, episodes: int, episode_len: int, max_action: float = 1.0, base_seed: int = 0,
                 mode: str = "mean", member: int = 0, reward_penalty: float = 0.0, clip_states: bool = True,
                 seed: int = 0, sample: bool = False, uncertainty: str = "disagreement",
                 halt_threshold: Optional[float] = None, halt_reward: float = 0.0, halt_cost: float = 1.0,
                 cost_penalty: float = 0.0):
        import torch

        from .. import _lib as L
        from ..engine.core import require_cuda
        self.model, self.E, self.base_seed = model, int(episodes), int(base_seed)
        self.device = require_cuda(model.device)
        L.load()
        self.state_dim, self.action_dim, self.episode_len = model.state_dim, model.action_dim, int(episode_len)
        self.max_action, self.clip_states = float(max_action), bool(clip_states)
        if self.E < 1 or self.episode_len < 1:
            raise ValueError("ModelVecEnv needs episodes >= 1 and episode_len >= 1")
        rows = self._init_rows(init_states)
        if rows.dim() != 2 or rows.shape[1] != self.state_dim or rows.shape[0] < 1:
            raise ValueError(f"init_states must be [n >= 1, {self.state_dim}], got {tuple(rows.shape)}")
        idx = (self.base_seed + torch.arange(self.E, device=self.device)) % rows.shape[0]
        # the initial states are a function of (init_states, base_seed) only: kept in HBM, reset() is a device copy
        self.state0 = rows.index_select(0, idx).contiguous()
        f = dict(dtype=torch.float32, device=self.device)
        self.state = torch.zeros(self.E, self.state_dim, **f)
        self.acc = torch.zeros(self.E, 4, **f)
        self.unc = torch.zeros(self.E, 2, **f)
        self.halt_step = torch.full((self.E,), -1, dtype=torch.int32, device=self.device)
        self.extra_state = (self.unc, self.halt_step)  # what a step changes beside state / acc (BatchedRollout._snapshot)
        self._seed = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.member_in = None  # int32 [E] on the device: injected member choices of mode "random" (tests)
        self.noise_in = None  # float32 [E, od + 1] on the device: injected draws of ``sample`` (tests)
        self._own_epoch = 0
        self._mode, self._member, self._penalty = "mean", 0, 0.0
        self._sample, self._uncertainty = False, "disagreement"
        self._halt_thr, self._halt_reward, self._halt_cost, self._cost_penalty = None, 0.0, 1.0, 0.0
        self.seed = seed
        self.set_mode(mode, member)
        self.reward_penalty = reward_penalty
        self.sample = sample
        self.uncertainty = uncertainty
        self.halt_threshold, self.halt_reward, self.halt_cost = halt_threshold, halt_reward, halt_cost
        self.cost_penalty = cost_penalty
        model.repack()

    def _init_rows(self, init_states):
        import torch
        if hasattr(init_states, "tables"):  # a ReplayStore
            if not getattr(init_states, "state_init", False):
                raise ValueError("initial states from a store: build the ReplayStore with state_init=True")
            obs, init = init_states.live(0), init_states.live(6).reshape(-1)
            return obs[init == 1.0].to(self.device, torch.float32).contiguous()
        return torch.as_tensor(np.asarray(init_states) if not torch.is_tensor(init_states) else init_states).to(
            device=self.device, dtype=torch.float32).contiguous()

    # ---- what may change between runs ---------------------------------------------------------------------------------
    @property
    def launch_epoch(self) -> int:
        """Counts the changes of by-value launch arguments, the model's elite set among them (``Dynamics.elite_epoch``):
        a rollout compares it with its descriptor's and rebuilds that, dropping its captured graph."""
        return self._own_epoch + self._model_epoch()

    @launch_epoch.setter
    def launch_epoch(self, v: int) -> None:
        self._own_epoch = int(v) - self._model_epoch()

    def _model_epoch(self) -> int:
        return getattr(getattr(self, "model", None), "elite_epoch", 0)

    def _elites(self):
        f = getattr(self.model, "elite_members", None)
        return list(range(self.model.num_models)) if f is None else f()

    @property
    def seed(self) -> int:
        return int(self._seed.item())

    @seed.setter
    def seed(self, v: int) -> None:
        self._seed.fill_(int(v) & 0x7FFFFFFFFFFFFFFF)  # (device memory: a captured launch follows)

    @property
    def mode(self) -> str:
        return self._mode

    @property
    def member(self) -> int:
        return self._member

    def set_mode(self, mode: str, member: int = 0) -> None:
        from .. import _lib as L
        if mode not in L.MODEL_ENV_MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(L.MODEL_ENV_MODES)}")
        if not 0 <= int(member) < self.model.num_models:
            raise ValueError(f"member {member}: the model has {self.model.num_models} members")
        if mode == "member" and int(member) not in self._elites():
            raise ValueError(f"mode 'member' follows member {member}, which is not among the elites {self._elites()}")
        if (mode, int(member)) != (self._mode, self._member):
            self._mode, self._member = mode, int(member)
            self.launch_epoch += 1

    @property
    def reward_penalty(self) -> float:
        return self._penalty

    @reward_penalty.setter
    def reward_penalty(self, v: float) -> None:
        if float(v) != self._penalty:
            self._penalty = float(v)
            self.launch_epoch += 1

    def _needs_gauss(self, what: str) -> None:
        if not getattr(self.model, "probabilistic", False):
            raise ValueError(f"{what} reads the members' predicted variance: build the Dynamics with probabilistic=True")

    @property
    def sample(self) -> bool:
        return self._sample

    @sample.setter
    def sample(self, v: bool) -> None:
        if bool(v):
            self._needs_gauss("sample=True")
        if bool(v) != self._sample:
            self._sample = bool(v)
            self.launch_epoch += 1

    @property
    def uncertainty(self) -> str:
        return self._uncertainty

    @uncertainty.setter
    def uncertainty(self, v: str) -> None:
        from .. import _lib as L
        if v not in L.MODEL_ENV_UNC:
            raise ValueError(f"uncertainty {v!r}: one of {sorted(L.MODEL_ENV_UNC)}")
        if v != "disagreement":
            self._needs_gauss(f"uncertainty={v!r}")
        if v != self._uncertainty:
            self._uncertainty = v
            self.launch_epoch += 1

    # ---- halting and the pessimistic cost (launch arguments) -----------------------------------------------------------
    @property
    def halt_threshold(self) -> Optional[float]:
        return self._halt_thr

    @halt_threshold.setter
    def halt_threshold(self, v: Optional[float]) -> None:
        v = None if v is None else float(v)
        if v is not None and math.isnan(v):
            raise ValueError("halt_threshold is NaN: a number (u > threshold halts) or None")
        if v != self._halt_thr:
            if v is None:  # nothing writes halt_step from here on: reset() and the branch starts leave it alone
                self.halt_step.fill_(-1)
            self._halt_thr = v
            self.launch_epoch += 1

    @property
    def can_halt(self) -> bool:
        """Whether a step may end an episode early: recorded rollouts are then variable-length."""
        return self._halt_thr is not None

    @property
    def halt_reward(self) -> float:
        return self._halt_reward

    @halt_reward.setter
    def halt_reward(self, v: float) -> None:
        if math.isnan(float(v)):
            raise ValueError("halt_reward is NaN")
        if float(v) != self._halt_reward:
            self._halt_reward = float(v)
            self.launch_epoch += 1

    @property
    def halt_cost(self) -> float:
        return self._halt_cost

    @halt_cost.setter
    def halt_cost(self, v: float) -> None:
        if float(v) not in (0.0, 1.0):
            raise ValueError(f"halt_cost {v}: the raw cost of a halting step, 0 or 1")
        if float(v) != self._halt_cost:
            self._halt_cost = float(v)
            self.launch_epoch += 1

    @property
    def cost_penalty(self) -> float:
        return self._cost_penalty

    @cost_penalty.setter
    def cost_penalty(self, v: float) -> None:
        if not 0.0 <= float(v) < math.inf:
            raise ValueError(f"cost_penalty {v}: a finite value >= 0")
        if float(v) != self._cost_penalty:
            self._cost_penalty = float(v)
            self.launch_epoch += 1

    def halted(self) -> np.ndarray:
        """Per episode the step at which it halted, -1 where it did not (int32 numpy).  Synchronises."""
        return self.halt_step.cpu().numpy()

    def set_noise_in(self, eps) -> None:
        """Inject ``sample``'s draws: ``[E, od + 1]`` standard-normal values, one per episode and sampled column (the state
        delta's and the reward's), the same at every step (None: draw them from ``seed``, Philox stream 16)."""
        import torch
        had = self.noise_in is not None
        if eps is None:
            self.noise_in = None
        else:
            self._needs_gauss("noise_in")
            t = torch.as_tensor(np.asarray(eps.cpu() if torch.is_tensor(eps) else eps, np.float32)).to(self.device)
            if tuple(t.shape) != (self.E, self.state_dim + 1):
                raise ValueError(f"noise_in: [{self.E}, {self.state_dim + 1}] values, got {tuple(t.shape)}")
            t = t.contiguous()
            if had:
                self.noise_in.copy_(t)
            else:
                self.noise_in = t
        if had != (self.noise_in is not None):
            self.launch_epoch += 1

    def set_member_in(self, members) -> None:
        """Inject mode "random"'s choices: one member per episode, the same at every step (None: draw them).  The indices
        are POSITIONS among the members the environment steps, ``[0, k)`` on a model with k elites (position j is member
        ``model.elite_members()[j]``); on a model without elites positions and member indices coincide."""
        import torch
        had = self.member_in is not None
        if members is None:
            self.member_in = None
        else:
            t = torch.as_tensor(np.asarray(members, np.int32)).to(self.device).reshape(-1).contiguous()
            k = len(self._elites())
            if t.numel() != self.E or int(t.min()) < 0 or int(t.max()) >= k:
                raise ValueError(f"member_in: {self.E} indices below {k}")
            if had:
                self.member_in.copy_(t)
            else:
                self.member_in = t
        if had != (self.member_in is not None):
            self.launch_epoch += 1

    # ---- the vector-environment interface -----------------------------------------------------------------------------
    def desc(self, episode_len: int, cost_scale: float):
        """The by-value launch descriptor for the current mode / member / penalty, tagged with ``launch_epoch``."""
        from .. import _lib as L
        m = self.model
        d = L.ModelEnvT()
        elites, nets = self._elites(), m.member_descs()
        for i, e in enumerate(elites):  # (every member, in order, on a model without elites)
            d.net[i] = nets[e]
        member = self._member
        if self._mode == "member":  # a model index; the launch takes its position among the nets of the descriptor
            if member not in elites:
                raise ValueError(f"mode 'member' follows member {member}, which is not among the elites {elites}")
            member = elites.index(member)
        for k in ("mu_s", "sd_s", "mu_d", "sd_d", "mu_r", "sd_r"):
            setattr(d, k, getattr(m, k).data_ptr())
        if self.clip_states:
            d.s_lo, d.s_hi = m.s_lo.data_ptr(), m.s_hi.data_ptr()
        d.seed = self._seed.data_ptr()
        d.member_in = None if self.member_in is None else self.member_in.data_ptr()
        d.n_models, d.state_dim, d.action_dim, d.episode_len = len(elites), self.state_dim, self.action_dim, int(episode_len)
        d.mode, d.member, d.episode_base = L.MODEL_ENV_MODES[self._mode], member, self.base_seed & 0xFFFFFFFF
        d.max_action, d.cost_scale, d.reward_penalty = self.max_action, float(cost_scale), self._penalty
        if getattr(m, "probabilistic", False):  # osrl_model_env_gauss_t: the same descriptor, embedded
            g = L.ModelEnvGaussT()
            g.env = d
            g.noise_in = None if self.noise_in is None else self.noise_in.data_ptr()
            g.logvar_min, g.logvar_max = float(m.logvar_min.item()), float(m.logvar_max.item())
            g.sample, g.uncertainty = int(self._sample), L.MODEL_ENV_UNC[self._uncertainty]
            d = g
        if self._halt_thr is not None or self._cost_penalty != 0.0:  # the same descriptor beside osrl_model_env_pess_t
            p = L.ModelEnvPessT()
            p.halt_threshold = math.inf if self._halt_thr is None else self._halt_thr
            p.halt_reward, p.halt_cost, p.cost_penalty = self._halt_reward, self._halt_cost, self._cost_penalty
            p.halt_step = self.halt_step.data_ptr()
            d = (L.ModelEnvGaussHaltT if isinstance(d, L.ModelEnvGaussT) else L.ModelEnvHaltT)(d, p)
        d.launch_epoch = self.launch_epoch
        return d

    def reset(self, obs_out) -> None:
        """Initial states of episodes base_seed .. base_seed+E-1 -> ``state`` and ``obs_out[:, :od]``; zero totals."""
        self.state.copy_(self.state0)
        obs_out[:, :self.state_dim].copy_(self.state0)
        self.acc.zero_()
        self.unc.zero_()
        if self._halt_thr is not None:  # (otherwise it holds -1: nothing has written it since the threshold was None)
            self.halt_step.fill_(-1)

    def step(self, desc, actions, obs_out, step_out=None) -> None:
        """``step_out`` (optional [E,2]) receives this step's (reward, raw cost)."""
        import ctypes as C

        from .. import _lib as L
        from ..engine.core import cur_stream
        if isinstance(desc, L._HaltDesc):
            name, head = desc.step_fn, (C.byref(desc.env), C.byref(desc.pess))
        else:
            name = "osrl_model_env_step_gauss" if isinstance(desc, L.ModelEnvGaussT) else "osrl_model_env_step"
            head = (C.byref(desc),)
        L.check(getattr(L.load(), name)(*head, actions.data_ptr(), self.state.data_ptr(), obs_out.data_ptr(),
                                        obs_out.stride(0), self.acc.data_ptr(), self.unc.data_ptr(),
                                        None if step_out is None else step_out.data_ptr(), self.E, cur_stream()), name)

    def disagreement(self):
        """Per episode ``(max, mean over the steps taken)`` of the uncertainty signal in use (normalised units), two numpy
        arrays: the members' disagreement over their means, or with ``uncertainty="max_std"`` the largest predicted
        standard deviation.  Synchronises."""
        u, n = self.unc.cpu().numpy().astype(np.float64), self.acc[:, 2].cpu().numpy().astype(np.float64)
        return u[:, 0], u[:, 1] / np.maximum(n, 1.0)
