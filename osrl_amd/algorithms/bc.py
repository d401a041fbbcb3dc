"""Behaviour cloning on MI355X behind the reference's API (osrl/algorithms/bc.py)."""
from __future__ import annotations

from typing import Dict, Optional

import torch.nn as nn

from ..common.logger import store_stats
from ..common.net import MLPActor, bind_group, check_mlp_limits, plan_group
from ..engine.core import FlatGroup, require_cuda
from ._base import FlatModel, RolloutMixin


class BC(FlatModel):
    """bc.py:12-64."""

    ENGINE = "bc.BCEngine"

    def __init__(self, state_dim: int, action_dim: int, max_action: float, a_hidden_sizes: list = [128, 128],
                 episode_len: int = 300, device: str = "cuda"):
        super().__init__()
        self.state_dim, self.action_dim, self.max_action = state_dim, action_dim, max_action
        self.a_hidden_sizes = list(a_hidden_sizes)
        self.episode_len = episode_len
        self.device = str(device)
        check_mlp_limits("BC", actor=[state_dim] + self.a_hidden_sizes + [action_dim])
        dev = require_cuda(device)
        self.actor = MLPActor(state_dim, action_dim, self.a_hidden_sizes, nn.ReLU, max_action)
        g = FlatGroup("actor", dev)
        plan_group(g, "actor", self.actor)
        g.finalize()
        bind_group(g, "actor", self.actor)
        self.groups: Dict[str, FlatGroup] = {"actor": g}
        self._engine = None
        self._lrs: Optional[dict] = None

    def setup_optimizers(self, actor_lr):
        self._lrs = dict(actor=actor_lr)

    def _policy_spec(self):
        from ..common.net import net_desc_seq
        # (max_action: the clip of the exploration tail; the "mlp" kind's own action does not read it)
        return ("mlp", self.actor.pi[0].in_features, net_desc_seq([self.actor.pi], float(self.actor.act_limit)),
                dict(max_action=float(self.actor.act_limit)))

    def act(self, obs):
        """bc.py:57-64: single observation -> action (numpy)."""
        return self.fast_policy().act(obs)[0]


class BCTrainer(RolloutMixin):
    """bc.py:67-145."""

    def __init__(self, model: BC, env=None, logger=None, actor_lr: float = 1e-4, bc_mode: str = "all",
                 cost_limit: int = 10, device="cuda", stats_mode: str = "lazy", use_graph: bool = True):
        self.model, self.logger, self.env, self.device = model, logger, env, device
        self.bc_mode, self.cost_limit = bc_mode, cost_limit
        self.stats_mode, self.use_graph = stats_mode, use_graph
        self.model.setup_optimizers(actor_lr)

    def set_target_cost(self, target_cost):
        self.cost_limit = target_cost

    def train_one_step(self, observations, actions):
        eng = self.model.engine(observations.shape[0])
        eng.step(observations, actions, use_graph=self.use_graph)
        store_stats(self.logger, eng.st, self.stats_mode)

    # bc.py:111-149: evaluate() does not rescale, info["cost"] is summed as it is, and in ``multi-task`` mode the cost
    # limit is appended to every observation
    EVAL_KIND = "bc"

    def _before_evaluate(self) -> None:
        if getattr(self.model, "_engine", None) is not None:
            self.model._engine.check_health()  # never evaluate parameters a failed one-launch step left behind

    def _eval_extra(self):
        return float(self.cost_limit) if self.bc_mode == "multi-task" else None

    def _act_for_rollout(self, obs):
        return self.model.act(obs)

    def _cost_scale(self):
        return None

    def _scale_results(self, r, c, n):
        return r, c, n
