"""BCQ-Lagrangian on MI355X behind the reference's API (osrl/algorithms/bcql.py)."""
from __future__ import annotations

from copy import deepcopy
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from ..common.logger import store_stats
from ..common.net import (VAE, EnsembleDoubleQCritic, MLPGaussianPerturbationActor, bind_group, check_mlp_limits,
                          plan_group)
from ..engine.core import FlatGroup, require_cuda
from ._base import FlatModel, RolloutMixin


class LagrangianPIDController:
    """net.py:356-387 -- the integrator state lives in a 2-float device tensor ``state`` =
    [error_old, error_integral]; the update itself runs inside the actor-loss kernel
    (csrc/glue.hip bcq_actor_loss_kernel) so there is no host round trip."""

    def __init__(self, KP, KI, KD, thres, state: torch.Tensor) -> None:
        self.KP, self.KI, self.KD, self.thres = KP, KI, KD, thres
        self.state = state

    @property
    def error_old(self) -> float:
        return float(self.state[0].item())

    @property
    def error_integral(self) -> float:
        return float(self.state[1].item())


class BCQL(FlatModel):
    """bcql.py:15-112."""

    ENGINE = "bcql.BCQLEngine"

    def __init__(self, state_dim: int, action_dim: int, max_action: float, a_hidden_sizes: list = [128, 128],
                 c_hidden_sizes: list = [128, 128], vae_hidden_sizes: int = 64, sample_action_num: int = 10,
                 gamma: float = 0.99, tau: float = 0.005, phi: float = 0.05, lmbda: float = 0.75,
                 beta: float = 0.5, PID: list = [0.1, 0.003, 0.001], num_q: int = 1, num_qc: int = 1,
                 cost_limit: int = 10, episode_len: int = 300, device: str = "cuda"):
        super().__init__()
        self.state_dim, self.action_dim, self.max_action = state_dim, action_dim, max_action
        self.latent_dim = self.action_dim * 2
        self.a_hidden_sizes, self.c_hidden_sizes = list(a_hidden_sizes), list(c_hidden_sizes)
        self.vae_hidden_sizes = vae_hidden_sizes
        self.sample_action_num = sample_action_num
        self.gamma, self.tau, self.phi, self.lmbda, self.beta = gamma, tau, phi, lmbda, beta
        self.KP, self.KI, self.KD = PID
        self.num_q, self.num_qc = num_q, num_qc
        self.cost_limit, self.episode_len = cost_limit, episode_len
        self.device = str(device)
        check_mlp_limits("BCQL", actor=[state_dim + action_dim] + self.a_hidden_sizes + [action_dim],
                         critic=[state_dim + action_dim] + self.c_hidden_sizes + [1],
                         vae_encoder=[state_dim + action_dim, vae_hidden_sizes, vae_hidden_sizes, 2 * self.latent_dim],
                         vae_decoder=[state_dim + self.latent_dim, vae_hidden_sizes, vae_hidden_sizes, action_dim])
        dev = require_cuda(device)

        # creation order of bcql.py:86-100 (actor, critic, cost_critic, vae)
        self.actor = MLPGaussianPerturbationActor(state_dim, action_dim, self.a_hidden_sizes, nn.Tanh, phi,
                                                  max_action)
        self.critic = EnsembleDoubleQCritic(state_dim, action_dim, self.c_hidden_sizes, nn.ReLU, num_q=num_q)
        self.cost_critic = EnsembleDoubleQCritic(state_dim, action_dim, self.c_hidden_sizes, nn.ReLU, num_q=num_qc)
        self.vae = VAE(state_dim, action_dim, vae_hidden_sizes, self.latent_dim, max_action, self.device)
        self.actor_old = deepcopy(self.actor)
        self.critic_old = deepcopy(self.critic)
        self.cost_critic_old = deepcopy(self.cost_critic)
        for m in (self.actor_old, self.critic_old, self.cost_critic_old):
            m.eval()

        self.groups: Dict[str, FlatGroup] = {}
        for name, with_tgt in (("actor", True), ("critic", True), ("cost_critic", True), ("vae", False)):
            g = FlatGroup(name, dev, with_target=with_tgt)
            plan_group(g, name, getattr(self, name))
            g.finalize()
            bind_group(g, name, getattr(self, name), getattr(self, name + "_old") if with_tgt else None)
            self.groups[name] = g

        self.qc_thres = cost_limit * (1 - self.gamma ** self.episode_len) / (1 - self.gamma) / self.episode_len
        self.pid_state = torch.zeros(2, dtype=torch.float32, device=dev)
        self.controller = LagrangianPIDController(self.KP, self.KI, self.KD, self.qc_thres, self.pid_state)
        self._engine = None
        self._lrs: Optional[dict] = None

    def setup_optimizers(self, actor_lr, critic_lr, vae_lr):
        """bcql.py:218-226."""
        self._lrs = dict(actor=actor_lr, critic=critic_lr, cost_critic=critic_lr, vae=vae_lr)

    def sync_weight(self):
        """bcql.py:228-234 -- fused into the per-group optimizer kernels of train_one_step."""
        return None

    def _policy_spec(self):
        from ..common.net import net_desc_seq, vae_dec_desc
        return "bcq", self.state_dim, vae_dec_desc(self.vae), dict(
            max_action=float(self.actor.act_limit), net1=net_desc_seq([self.actor.pi], 1.0), latent_dim=self.latent_dim,
            phi=float(self.actor.phi))

    @torch.no_grad()
    def act(self, obs, deterministic=False, with_logprob=False, z=None):
        """bcql.py:236-243 (stochastic: decode draws z unless given)."""
        zz = None if z is None else (z.detach().cpu().numpy() if torch.is_tensor(z) else np.asarray(z))
        return self.fast_policy().act(obs, deterministic, noise=zz)[0], None


class BCQLTrainer(RolloutMixin):
    """bcql.py:246-340."""

    def __init__(self, model: BCQL, env=None, logger=None, actor_lr: float = 1e-4,
                 critic_lr: float = 1e-4, vae_lr: float = 1e-4, reward_scale: float = 1.0,
                 cost_scale: float = 1.0, device="cuda", stats_mode: str = "lazy", use_graph: bool = True):
        self.model, self.logger, self.env = model, logger, env
        self.reward_scale, self.cost_scale, self.device = reward_scale, cost_scale, device
        self.stats_mode, self.use_graph = stats_mode, use_graph
        self.model.setup_optimizers(actor_lr, critic_lr, vae_lr)

    def train_one_step(self, observations, next_observations, actions, rewards, costs, done, noise=None):
        eng = self.model.engine(observations.shape[0])
        eng.step(observations, next_observations, actions, rewards, costs, done, noise=noise,
                 use_graph=self.use_graph and noise is None)
        store_stats(self.logger, eng.st, self.stats_mode)

    # bcql.py:308-340: rollout() acts through the stochastic decode (z drawn per step; in the batched and lockstep forms
    # from the device Philox stream, keyed by the episode id and the step)
    EVAL_KIND = "bcql"

    def _act_for_rollout(self, obs):
        return self.model.act(obs)[0]
