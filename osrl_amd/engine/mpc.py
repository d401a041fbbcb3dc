"""Planning at act time: policy-guided shooting on the learned model (MBOP's rule; DESIGN.md "Planning at act time").

``ModelPlanner`` is a ``ModelCollector`` (engine/collect.py) whose run starts at N REAL states instead of the environment's
own: every state ("slot") fans out into K imagined episodes (csrc/plan.hip ``osrl_plan_fanout``; episode ``n * K + k`` is
candidate k of slot n), the collector's recorded step runs H times -- the policy's launches, ``a = clip(pi(s) + sigma_e *
eps)``, ``osrl_model_env_collect*`` with whatever pessimism the environment carries (``reward_penalty``, ``cost_penalty``,
``halt_threshold``) -- and ``osrl_plan_select`` picks one candidate per slot from the discounted sums the recorder keeps:
the best penalised return among those whose discounted cost stays inside the slot's remaining budget, the cheapest one
when none does, or with ``temperature > 0`` the softmax average of the feasible first actions (MPPI).

Candidate 0 of every slot has sigma = 0: the policy's own proposal is always among the candidates.  The noise is the
collectors' (Philox stream 13, keyed by seed word, episode id ``base_seed + n * K + k``, the episode's step and the action
column) and the model's steps do not depend on their tile neighbours, so a slot's action is a function of its own state
and budget, the weights, the seed and the call number -- not of N, the slot's position aside, nor of the other slots.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from .. import _lib as L
from .collect import ModelCollector
from .core import cur_stream
from .rollout import _CHUNK


def check_plan(venv, num_envs, horizon, noise_std=0.0, temperature=0.0) -> int:
    """A planner's shape, judged on the host before anything is built or launched: the candidates per slot K.  TypeError
    for anything but a ``ModelVecEnv``; ValueError unless ``venv.E == num_envs * K`` with ``1 <= K <=
    PLAN_MAX_CANDIDATES``, ``horizon >= 1``, and ``noise_std`` / ``temperature`` are finite and not negative."""
    from ..common.model_env import ModelVecEnv
    if not isinstance(venv, ModelVecEnv):
        raise TypeError(f"a planner imagines on a learned model: a ModelVecEnv, not {type(venv).__name__}")
    N, H = int(num_envs), int(horizon)
    if N < 1:
        raise ValueError(f"num_envs {N}: at least one slot")
    if H < 1:
        raise ValueError(f"horizon {H}: at least one step")
    if venv.E % N != 0:
        raise ValueError(f"the model environment holds {venv.E} episodes, no multiple of num_envs = {N}: build it with "
                         f"episodes = num_envs * candidates")
    K = venv.E // N
    if K > L.PLAN_MAX_CANDIDATES:
        raise ValueError(f"{K} candidates per slot: at most {L.PLAN_MAX_CANDIDATES}")
    for name, x in (("noise_std", noise_std), ("temperature", temperature)):
        if not (0.0 <= float(x) < math.inf):
            raise ValueError(f"{name} {x}: a finite value >= 0")
    return K


def check_budget(cost_budget, num_envs: int) -> np.ndarray:
    """``act``'s ``cost_budget`` as fp32 ``[num_envs]``: one value for every slot or one per slot (ValueError for another
    length).  In the collector's ``cost_scale`` units, like the discounted cost it is compared with."""
    if torch.is_tensor(cost_budget):
        cost_budget = cost_budget.detach().cpu().numpy()
    b = np.asarray(cost_budget, dtype=np.float32)
    if b.ndim == 0:
        return np.full(int(num_envs), b, np.float32)
    b = b.reshape(-1)
    if b.size != int(num_envs):
        raise ValueError(f"cost_budget holds {b.size} values, the planner {int(num_envs)} slots")
    return b


def check_states(states, num_envs: int, state_dim: int) -> np.ndarray:
    """``act``'s ``states`` as fp32 ``[num_envs, state_dim]`` on the host; ValueError for another shape."""
    if torch.is_tensor(states):
        states = states.detach().cpu().numpy()
    s = np.asarray(states, dtype=np.float32)
    if s.shape != (int(num_envs), int(state_dim)):
        raise ValueError(f"states must be [{int(num_envs)}, {int(state_dim)}], got {s.shape}")
    return s


class ModelPlanner(ModelCollector):
    """``act(states [N, od], cost_budget)`` -> ``[N, ad]`` actions (numpy): upload, fan-out, H recorded model steps (one
    captured graph of ``min(H, _CHUNK)`` steps, replayed in chunks beyond that), select, one host sync.  Nothing is
    compacted and nothing appended to a store: on an environment that can halt, a halted candidate simply stops adding to
    its sums (and counts with ``halt_reward`` / ``halt_cost``).

    The seed word of call number c is ``seed + c`` -- device memory, so the graph is captured once; ``reset_calls()``
    starts the count again.  ``temperature`` is a device word too and may be set between calls.  BCQ-L with unfixed ``z``
    does what ``ModelCollector`` does today: its decode noise has the seed as a by-value launch argument, so every call
    (a new seed) drops the graph and captures again; pass ``z`` for a planner that keeps its graph.

    Of the last call, on the device: ``last_J`` / ``last_C`` ``[N, K]`` (discounted penalised return and discounted cost
    of every candidate, the latter in ``cost_scale`` units), ``last_first_actions`` ``[N, K, ad]``, ``chosen`` ``[N]``
    (int32: the arg-best candidate, under MPPI too) and ``n_feasible`` ``[N]``.  The first three are views of the
    planner's tables: the next call overwrites them."""

    def __init__(self, model, venv, kind: str, cost_scale: float = 1.0, extra_obs: Optional[float] = None,
                 num_envs: int = 1, horizon: int = 1, noise_std: float = 0.3, gamma: float = 1.0,
                 temperature: float = 0.0, seed: int = 0, z: Optional[torch.Tensor] = None, use_graph: bool = True):
        K = check_plan(venv, num_envs, horizon, noise_std, temperature)  # (before any device work)
        super().__init__(model, venv, kind, cost_scale, extra_obs, seed, z, use_graph)
        N, od, ad, dev = int(num_envs), venv.state_dim, model.action_dim, self.obs.device
        self.num_envs, self.candidates, self.horizon = N, K, int(horizon)
        self.noise_std, self.plan_gamma, self.base_plan_seed, self.calls = float(noise_std), float(gamma), int(seed), 0
        sg = torch.full((N, K), self.noise_std, dtype=torch.float32)
        sg[:, 0] = 0.0  # candidate 0: the policy's own proposal
        self._sigma_plan = sg.reshape(-1).to(dev)
        self._host_in = torch.zeros(N * (od + 1), dtype=torch.float32).pin_memory()  # states, then budgets: one upload
        self._dev_in = torch.zeros(N * (od + 1), dtype=torch.float32, device=dev)
        self._states, self._budget = self._dev_in[:N * od].view(N, od), self._dev_in[N * od:]
        self._temperature = torch.zeros(1, dtype=torch.float32, device=dev)
        self.temperature = temperature
        self.action = torch.zeros(N, ad, dtype=torch.float32, device=dev)
        self.chosen = torch.zeros(N, dtype=torch.int32, device=dev)
        self.n_feasible = torch.zeros(N, dtype=torch.int32, device=dev)

    @property
    def temperature(self) -> float:
        return self._temp_host

    @temperature.setter
    def temperature(self, v: float) -> None:
        if not (0.0 <= float(v) < math.inf):
            raise ValueError(f"temperature {v}: a finite value >= 0")
        self._temp_host = float(v)
        self._temperature.fill_(float(v))  # (device memory: a captured launch would follow)

    def reset_calls(self) -> None:
        """The next ``act`` is call number 0 again: it draws the first call's noise."""
        self.calls = 0

    @property
    def last_J(self) -> torch.Tensor:
        return self.disc[:, 0].view(self.num_envs, self.candidates)

    @property
    def last_C(self) -> torch.Tensor:
        return self.disc[:, 1].view(self.num_envs, self.candidates)

    @property
    def last_first_actions(self) -> torch.Tensor:
        ad = self.model.action_dim
        return self.tables["actions"].view(self.num_envs, self.candidates, self.horizon, ad)[:, :, 0]

    def run(self, *a, **kw):
        raise TypeError("a ModelPlanner plans (act); record rollouts with the trainer's collect_model")

    def _fanout(self) -> None:
        v = self.venv
        L.check(L.load().osrl_plan_fanout(
            self._states.data_ptr(), self.num_envs, self.candidates, v.state_dim, v.state.data_ptr(), self.obs.data_ptr(),
            self.obs.stride(0), v.acc.data_ptr(), v.unc.data_ptr(), self.disc.data_ptr(),
            v.halt_step.data_ptr() if v.can_halt else None, cur_stream()), "osrl_plan_fanout")

    def _select(self) -> None:
        L.check(L.load().osrl_plan_select(
            self.tables["actions"].data_ptr(), self.horizon, self.disc.data_ptr(), self._budget.data_ptr(),
            self._temperature.data_ptr(), self.num_envs, self.candidates, self.model.action_dim, self.action.data_ptr(),
            self.chosen.data_ptr(), self.n_feasible.data_ptr(), cur_stream()), "osrl_plan_select")

    @torch.no_grad()
    def act(self, states, cost_budget) -> np.ndarray:
        """``states``: ``[N, od]`` (array or tensor); ``cost_budget``: a float or ``[N]``, each slot's remaining budget in
        ``cost_scale`` units.  Every refusal comes before the first launch."""
        N, od, H = self.num_envs, self.venv.state_dim, self.horizon
        s, b = check_states(states, N, od), check_budget(cost_budget, N)
        host = self._host_in.numpy()
        host[:N * od], host[N * od:] = s.reshape(-1), b
        seed = (self.base_plan_seed + self.calls) & 0xFFFFFFFFFFFFFFFF
        self._begin(H, seed, self._sigma_plan, self.plan_gamma, None)
        self._dev_in.copy_(self._host_in, non_blocking=True)
        self._fanout()
        self._drive_recorded(H, min(H, _CHUNK), None)
        self._select()
        self.calls += 1
        return self.action.cpu().numpy()
