"""An ensemble dynamics model fitted on the logged transitions: what ``common/model_env.py`` steps as a vector environment.

The reference has no counterpart -- it evaluates a policy on a simulator.  ``Dynamics`` holds ``num_models`` ReLU MLPs
``[state_dim + action_dim, *hidden, state_dim + 2]`` (the PETS / MOPO ensemble).  Member m maps the normalised input
``x = [(s - mu_s) / sd_s, a]`` to

    columns 0 .. od-1   the normalised state delta   (s' - s - mu_d) / sd_d
    column  od          the normalised reward        (r - mu_r) / sd_r
    column  od+1        the raw 0 / 1 cost, regressed by MSE (the environment thresholds it at 0.5)

``probabilistic=True`` makes every member a diagonal Gaussian (MOPO / MBPO / PETS): ``[od + ad, *hidden, 2 od + 3]``, the
first ``od + 2`` columns as above (the means, and the cost still regressed by MSE), then

    columns od+2 .. 2 od+2   the raw log-variance of columns 0 .. od; column od+2+k belongs to column k

bounded by PETS' soft clamp with the fixed bounds ``logvar_min`` / ``logvar_max`` (registered buffers of such a model only):
``lv = lo + softplus((hi - softplus(hi - raw)) - lo)``, ``sigma = exp(0.5 lv)``; fitted by negative log-likelihood.

All members see the same minibatches; their diversity comes from initialisation.  The six normaliser tables and the state
bounds ``s_lo`` / ``s_hi`` are registered buffers: ``state_dict`` and the checkpoints carry them.  The arithmetic of the train
step is the HIP plan in ``osrl_amd/engine/dynamics.py``.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn as nn

from .. import _lib as L
from ..common.net import bind_group, check_mlp_limits, mlp, plan_group
from ..engine.core import FlatGroup, require_cuda
from ._base import FlatModel

SIGMA_FLOOR = 1e-6
TABLES = ("mu_s", "sd_s", "mu_d", "sd_d", "mu_r", "sd_r", "s_lo", "s_hi")


class Dynamics(FlatModel):
    ENGINE = "dynamics.DynamicsEngine"

    def __init__(self, state_dim: int, action_dim: int, hidden_sizes: list = [200, 200, 200], num_models: int = 5,
                 device: str = "cuda", probabilistic: bool = False, logvar_min: float = -10.0, logvar_max: float = 0.5):
        super().__init__()
        self.state_dim, self.action_dim = int(state_dim), int(action_dim)
        self.hidden_sizes, self.num_models = list(hidden_sizes), int(num_models)
        self.probabilistic = bool(probabilistic)
        if not 1 <= self.num_models <= L.MAX_NETS:
            raise ValueError(f"num_models = {num_models}: the ensemble runs as one launch, 1 <= num_models <= {L.MAX_NETS}")
        if self.probabilistic and not float(logvar_min) < float(logvar_max):
            raise ValueError(f"Dynamics: logvar_min {logvar_min} must lie below logvar_max {logvar_max}")
        self.out_width = 2 * self.state_dim + 3 if self.probabilistic else self.state_dim + 2
        sizes = [self.state_dim + self.action_dim] + self.hidden_sizes + [self.out_width]
        check_mlp_limits("Dynamics", member=sizes)
        # the environment step keeps a 16-episode tile of every layer in LDS (csrc/model_env.hip)
        if max(sizes) > L.MODEL_ENV_MAX_WIDTH:
            raise ValueError(f"Dynamics: a layer {max(sizes)} wide; the environment step takes at most "
                             f"{L.MODEL_ENV_MAX_WIDTH} units per layer (sizes {sizes})")
        if self.state_dim > L.MODEL_ENV_MAX_STATE:
            raise ValueError(f"Dynamics: state_dim {self.state_dim}; the environment step takes at most "
                             f"{L.MODEL_ENV_MAX_STATE}")
        self.device = str(device)
        dev = require_cuda(device)

        self.members = nn.ModuleList([mlp(sizes, nn.ReLU) for _ in range(self.num_models)])
        # ONE optimizer group without a target copy: one dW plan and one Adam launch serve every member
        g = FlatGroup("dynamics", dev, with_target=False)
        plan_group(g, "members", self.members)
        g.finalize()
        bind_group(g, "members", self.members)
        self.groups: Dict[str, FlatGroup] = {"dynamics": g}
        od = self.state_dim
        f = dict(dtype=torch.float32, device=dev)
        for name, n, fill in (("mu_s", od, 0.0), ("sd_s", od, 1.0), ("mu_d", od, 0.0), ("sd_d", od, 1.0), ("mu_r", 1, 0.0),
                              ("sd_r", 1, 1.0), ("s_lo", od, -3.0e38), ("s_hi", od, 3.0e38)):
            self.register_buffer(name, torch.full((n,), fill, **f))
        if self.probabilistic:  # (a deterministic model's state_dict keeps its keys)
            self.register_buffer("logvar_min", torch.full((1,), float(logvar_min), **f))
            self.register_buffer("logvar_max", torch.full((1,), float(logvar_max), **f))
        self.seed = 0
        self._engine = None
        self._lrs: Optional[dict] = None

    def setup_optimizers(self, lr):
        self._lrs = dict(dynamics=lr)

    def _engine_class(self):
        cls = super()._engine_class()
        return lambda model, batch_size, **kw: cls(model, batch_size, **{"seed": self.seed, **kw})

    def check_store(self, store) -> None:
        if int(store.widths[0]) != self.state_dim or int(store.widths[2]) != self.action_dim:
            raise ValueError(f"the store holds ({store.widths[0]}, {store.widths[2]})-wide states and actions, the model "
                             f"takes ({self.state_dim}, {self.action_dim})")
        if float(store.scales[4]) != 1.0:
            raise ValueError(f"the store scales costs by {store.scales[4]}: the model regresses the raw 0 / 1 cost "
                             "(build the ReplayStore with cost_scale=1)")

    @torch.no_grad()
    def fit_normalizer(self, data) -> None:
        """The normaliser tables and the state bounds from ``data``: a ``ReplayStore`` (its live rows, rewards as the store
        scales them) or a DSRL-layout dataset (a mapping with observations, next_observations, actions, rewards).  torch on
        the device in fp64, rounded to fp32 (off the hot path); population statistics, every sigma at least 1e-6;
        ``s_lo`` / ``s_hi`` = min / max over observations and next observations.  Written in place: a captured train step
        and a captured rollout follow."""
        dev = self.mu_s.device
        if hasattr(data, "tables"):
            self.check_store(data)
            obs, nobs, rew = data.live(0), data.live(1), data.live(3) * float(data.scales[3])
        else:
            t = lambda k: torch.as_tensor(data[k]).to(dev)  # noqa: E731
            obs, nobs, rew = t("observations"), t("next_observations"), t("rewards")
        obs, nobs = obs.to(dev, torch.float64).reshape(-1, self.state_dim), nobs.to(dev, torch.float64).reshape(-1, self.state_dim)
        rew = rew.to(dev, torch.float64).reshape(-1, 1)
        if obs.shape[0] < 1 or obs.shape != nobs.shape or rew.shape[0] != obs.shape[0]:
            raise ValueError("fit_normalizer: observations, next_observations and rewards must hold the same rows (>= 1)")
        sd = lambda x: x.std(0, unbiased=False).clamp_min(SIGMA_FLOOR)  # noqa: E731
        dl = nobs - obs
        both = torch.cat([obs, nobs], 0)
        for name, v in (("mu_s", obs.mean(0)), ("sd_s", sd(obs)), ("mu_d", dl.mean(0)), ("sd_d", sd(dl)),
                        ("mu_r", rew.mean(0)), ("sd_r", sd(rew)), ("s_lo", both.min(0).values), ("s_hi", both.max(0).values)):
            getattr(self, name).copy_(v.to(torch.float32))

    def member_descs(self):
        """One ``osrl_gemv_net_t`` per member over the group's packed forward weights (what the environment step reads)."""
        from ..common.net import net_desc_seq
        nd = net_desc_seq(list(self.members), 1.0)
        out = []
        for e in range(nd.E):
            n = L.GemvNetT()
            n.n_layers, n.out_scale = nd.nl, 1.0
            for i, v in enumerate(nd.dims):
                n.dims[i] = v
            for l in range(nd.nl):
                n.acts[l] = nd.acts[l]
                n.Wf[l] = nd.nets[e][l].wf_ptr
                n.b[l] = nd.nets[e][l].b.data_ptr()
            out.append(n)
        return out


class DynamicsTrainer:
    """``train_one_step`` on the caller's batch (``StepEngine.BATCH`` order; ``done`` is ignored), or ``model.engine(B)`` +
    ``attach_replay(store)`` + ``step_replay()`` with the minibatch drawn inside the step.  One statistic:
    ``loss/dynamics_loss``, the sum over the members of the batch-mean squared error in normalised units; for a
    ``probabilistic`` model the sum over the members of ``sum_rows [sum_{c <= od} ((mu_c - t_c)^2 exp(-lv_c) + lv_c) +
    (cost - t_cost)^2] / (B (od + 2))``, the Gaussian negative log-likelihood up to a constant (it may be negative)."""

    def __init__(self, model: Dynamics, logger=None, lr: float = 1e-3, seed: int = 0, stats_mode: str = "lazy",
                 use_graph: bool = True) -> None:
        self.model = model
        if logger is None:
            from ..common.logger import DummyLogger
            logger = DummyLogger()
        self.logger = logger
        self.stats_mode, self.use_graph = stats_mode, use_graph
        model.seed = int(seed)
        model.setup_optimizers(lr)

    def train_one_step(self, observations, next_observations, actions, rewards, costs, done=None):
        eng = self.model.engine(observations.shape[0])
        eng.step(observations, next_observations, actions, rewards, costs, eng.done if done is None else done,
                 use_graph=self.use_graph)
        from ..common.logger import store_stats
        store_stats(self.logger, eng.st, self.stats_mode)
