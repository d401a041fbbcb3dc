"""Fitted Q evaluation: the reward value and the cost value of a trained policy from the dataset alone.

The reference has no counterpart -- its only yardstick is ``evaluate()`` on an environment.  ``FQE`` fits an ensemble of
reward critics and an ensemble of cost critics for a frozen policy pi on the logged transitions (backup
``x + gamma (1 - done) Q_targ(s', pi(s'))``), ``FQETrainer.estimate`` reads ``Q(s0, pi(s0))`` at the dataset's initial
states.  The cost value is a discounted one: compare it with ``FQE.discounted_cost_limit`` (the ``q_thres`` of
cpq.py:102-105).  The arithmetic of the step is the HIP plan in ``osrl_amd/engine/fqe.py``.
"""
from __future__ import annotations

from copy import deepcopy
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from ..common.net import EnsembleQCritic, bind_group, check_mlp_limits, plan_group
from ..engine.core import FlatGroup, require_cuda
from ._base import FlatModel

MAX_NUM_Q = 4  # 2 * num_q nets share one launch (OSRL_MAX_NETS = 8); the seed reads <= 4 members per ensemble (kEns)


class FQEEstimate(NamedTuple):
    """Mean over the ensemble members of ``mean_s0 Q_e(s0, pi(s0))`` and the members' standard deviation, for the reward
    and the cost critics; ``n_init`` initial states.  Discounted values in the dataset's units (rescaled)."""
    value: float
    value_std: float
    cost_value: float
    cost_value_std: float
    n_init: int


def _device_key(device):
    d = torch.device(device)
    idx = d.index
    if d.type == "cuda" and idx is None:
        idx = torch.cuda.current_device() if torch.cuda.is_available() else 0
    return d.type, idx


class FQE(FlatModel):
    """``policy``: a trained BC / CPQ / BEARL / COptiDICE / BCQL model on ``device``; it is read in place (its packed
    forward weights, as ``BatchedRollout`` reads them) and never written, and it is NOT part of this model's
    ``state_dict``, which holds ``critic``, ``cost_critic`` and their targets in the reference's ``EnsembleQCritic`` layout."""

    ENGINE = "fqe.FQEEngine"

    def __init__(self, policy, c_hidden_sizes: list = [256, 256], gamma: float = 0.99, tau: float = 0.005,
                 num_q: int = 2, device: str = "cuda", state_dim: Optional[int] = None):
        """``state_dim``: the width of the dataset's observations, if the caller wants it checked here; a store whose
        observations are narrower than the policy's input is refused when it is attached or read in any case."""
        super().__init__()
        from ..engine.fqe import policy_kind
        self.kind = policy_kind(policy)  # TypeError: CDT, or not a policy of this package
        self.__dict__["policy"] = policy  # (not a submodule: its parameters stay out of state_dict and of .groups)
        self.state_dim, self.action_dim = int(policy.state_dim), int(policy.action_dim)
        if state_dim is not None and int(state_dim) != self.state_dim:
            raise ValueError(f"the policy's input is {self.state_dim} wide, the states are {int(state_dim)} wide (BC in "
                             "multi-task mode appends the cost limit to the state: FQE does not take such a policy)")
        self.c_hidden_sizes = list(c_hidden_sizes)
        self.gamma, self.tau, self.num_q = float(gamma), float(tau), int(num_q)
        if not 1 <= self.num_q <= MAX_NUM_Q:
            raise ValueError(f"num_q = {num_q}: FQE runs 2 * num_q nets per launch, 1 <= num_q <= {MAX_NUM_Q}")
        check_mlp_limits("FQE", critic=[self.state_dim + self.action_dim] + self.c_hidden_sizes + [1])
        self.device = str(device)
        if _device_key(policy.device) != _device_key(device):
            raise ValueError(f"the policy lives on {policy.device!r}, FQE was asked for {device!r}")
        dev = require_cuda(device)

        mk = lambda: EnsembleQCritic(self.state_dim, self.action_dim, self.c_hidden_sizes, nn.ReLU, num_q=self.num_q)  # noqa: E731
        self.critic, self.cost_critic = mk(), mk()
        self.critic_old, self.cost_critic_old = deepcopy(self.critic), deepcopy(self.cost_critic)
        for m in (self.critic_old, self.cost_critic_old):
            m.eval()
        # ONE optimizer group for both ensembles: one dW plan and one Adam + Polyak launch serve both
        g = FlatGroup("critic", dev, with_target=True)
        for name in ("critic", "cost_critic"):
            plan_group(g, name, getattr(self, name))
        g.finalize()
        for name in ("critic", "cost_critic"):
            bind_group(g, name, getattr(self, name), getattr(self, name + "_old"))
        self.groups: Dict[str, FlatGroup] = {"critic": g}
        self.seed = 0
        self._engine = None
        self._lrs: Optional[dict] = None
        self._readouts: dict = {}

    def setup_optimizers(self, critic_lr):
        self._lrs = dict(critic=critic_lr)

    def _engine_class(self):
        cls = super()._engine_class()
        return lambda model, batch_size, **kw: cls(model, batch_size, **{"seed": self.seed, **kw})

    @staticmethod
    def discounted_cost_limit(cost_limit: float, gamma: float, episode_len: int) -> float:
        """The per-state discounted threshold the algorithms compare a cost value with (cpq.py:102-105)."""
        return cost_limit * (1 - gamma ** episode_len) / (1 - gamma) / episode_len

    def check_store(self, store) -> None:
        if int(store.widths[0]) != self.state_dim or int(store.widths[2]) != self.action_dim:
            raise ValueError(f"the store holds ({store.widths[0]}, {store.widths[2]})-wide states and actions, the policy "
                             f"takes ({self.state_dim}, {self.action_dim}) (BC in multi-task mode is out of scope)")

    def readout(self, rows: int):
        from ..engine.fqe import ValueReadout
        r = self._readouts.get(rows)
        if r is None:
            r = self._readouts[rows] = ValueReadout(self, rows, torch.device(self.device))
        return r


class FQETrainer:
    """``train_one_step`` on the caller's batch (``StepEngine.BATCH`` order; rewards and costs as the dataset scales
    them), or ``model.engine(B)`` + ``attach_replay(store)`` + ``step_replay()`` with the minibatch drawn inside the step.
    ``reward_scale`` / ``cost_scale``: the dataset's scales, which ``estimate`` divides out again."""

    def __init__(self, model: FQE, logger=None, critic_lr: float = 1e-3, reward_scale: float = 1.0,
                 cost_scale: float = 1.0, seed: int = 0, stats_mode: str = "lazy", use_graph: bool = True) -> None:
        self.model = model
        if logger is None:
            from ..common.logger import DummyLogger
            logger = DummyLogger()
        self.logger = logger
        self.reward_scale, self.cost_scale = float(reward_scale), float(cost_scale)
        self.stats_mode, self.use_graph = stats_mode, use_graph
        model.seed = int(seed)
        model.setup_optimizers(critic_lr)
        self._init_idx: dict = {}

    def train_one_step(self, observations, next_observations, actions, rewards, costs, done, noise=None):
        """One FQE step.  ``noise``: ``{"z": [B, latent_dim]}``, the decode noise of a BCQ-Lag policy, injected (the step
        then runs eagerly); drawn on device when omitted."""
        eng = self.model.engine(observations.shape[0])
        eng.step(observations, next_observations, actions, rewards, costs, done, noise=noise,
                 use_graph=self.use_graph and noise is None)
        from ..common.logger import store_stats
        store_stats(self.logger, eng.st, self.stats_mode)

    def _initial_rows(self, store) -> torch.Tensor:
        if not getattr(store, "state_init", False):
            raise ValueError("estimate() reads the dataset's initial states: build the ReplayStore with state_init=True")
        hit = self._init_idx.get(id(store))
        version = getattr(store, "version", 0)  # (a store that grows: every append moves it)
        if hit is None or hit[0] is not store or hit[2] != version:
            idx = torch.nonzero(store.live(6).reshape(-1) == 1.0).reshape(-1).to(torch.int64).contiguous()
            hit = self._init_idx[id(store)] = (store, idx, version)
        return hit[1]

    @torch.no_grad()
    def estimate(self, store, rows: int = 1024, z=None) -> FQEEstimate:
        """The policy's value and cost value at the initial states of ``store`` (``ReplayStore(state_init=True)``), in
        chunks of ``rows`` states; the result does not depend on ``rows``, bit for bit.  ``z`` (BCQ-Lag policies):
        the decode noise [n_init, latent_dim], injected; by default drawn from the trainer's seed, the same every call.
        FQE's error grows with the shift between the policy and the data: a tool for ranking, not a certificate."""
        m = self.model
        idx = self._initial_rows(store)
        m.check_store(store)
        n = int(idx.numel())
        if n == 0:
            raise ValueError("the store has no initial state")
        dev = torch.device(m.device)
        zs = None
        if m.kind == "bcql":
            from ..engine import glue as G
            from ..engine.fqe import draw_decode_noise
            Lz = m.policy.latent_dim
            if z is None:
                zs = draw_decode_noise(n, Lz, m.seed, dev)
            else:
                zs = torch.as_tensor(z, dtype=torch.float32).to(dev).reshape(n, Lz).clone()
                G.clamp_(zs, -0.5, 0.5)
        acc = torch.zeros(2 * m.num_q, dtype=torch.float64, device=dev)
        rows = max(1, min(int(rows), n))
        for i0 in range(0, n, rows):
            i1 = min(i0 + rows, n)
            m.readout(i1 - i0).accumulate(store.tables[0], idx[i0:i1], None if zs is None else zs[i0:i1], acc)
        means = acc.cpu().numpy() / n  # the one host sync of the read-out
        E = m.num_q
        r, c = means[:E] / self.reward_scale, means[E:] / self.cost_scale
        return FQEEstimate(float(r.mean()), float(r.std()), float(c.mean()), float(c.std()), n)
