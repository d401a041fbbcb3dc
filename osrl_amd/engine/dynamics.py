"""The train step of the ensemble dynamics model (algorithms/dynamics.py) as a static launch plan on MI355X.

There is no reference file to follow.  Every member regresses the same normalised target -- state delta, reward, raw cost
-- by mean squared error:

    loss = sum_m mean_{rows, columns} (net_m([s~, a]) - target)^2

One chain on one stream, one one-step hipGraph:  prologue -> ``osrl_dyn_prepare`` (s~ and the target from the batch and the
model's normaliser tables) -> the members' forward on a shared input tile -> the backward launch that computes its own dY
(``OSRL_SEED_MSE``: every net of the launch against the one target table) -> dW + Adam.  The tables are read from the
model's buffers in place: ``fit_normalizer`` between two replays is followed.

A ``probabilistic`` model (members ``[.., 2 od + 3]``: means, cost, raw log-variances) is fitted by the Gaussian negative
log-likelihood instead: the same chain and the same target table, the backward launch seeded with ``OSRL_SEED_GAUSS_NLL``.
With ``s = 1 / (B (od + 2))`` and ``lv`` the bounded log-variance (algorithms/dynamics.py),

    loss = sum_m s sum_rows [ sum_{c <= od} ((mu_c - t_c)^2 exp(-lv_c) + lv_c) + (y_cost - t_cost)^2 ]

logged under the same key, ``loss/dynamics_loss``.
"""
from __future__ import annotations

import torch

from .. import _lib as L
from ..common.net import net_desc_seq
from . import glue as G
from ._step import StepEngine
from .core import DwPlan, MlpRun, StepState, cur_stream

STAT_KEYS = ["loss/dynamics_loss"]


class DynamicsEngine(StepEngine):
    SIDE_STREAMS = 0

    def __init__(self, model, batch_size: int, seed: int = 0, dist=None):
        if dist is not None:
            raise ValueError("the dynamics model has no data-parallel step (dist must be None)")
        m = self.model = model
        B = self.B = int(batch_size)
        self.dist, self.seed, self.rows_global = None, int(seed), 0
        dev = torch.device(m.device)
        od, ad, E = m.state_dim, m.action_dim, m.num_models
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)  # noqa: E731
        self.st = StepState(dev, STAT_KEYS)
        self.obs, self.nobs, self.act = z(B, od), z(B, od), z(B, ad)
        self.rew, self.cost, self.done = z(B), z(B), z(B)
        self.xs, self.target = z(B, od), z(B, od + 2)
        m.repack()
        self.r_f = MlpRun(net_desc_seq(list(m.members), 1.0), B, True, dev)
        self.dy = z(E, B, m.out_width)
        self.r_f.setup_backward(self.dy)
        self.plan = DwPlan(m.groups["dynamics"], self.r_f.dw_entries(), B, dev)
        self.seed_mse = self._seed_nll(dev) if m.probabilistic else self._seed_mse(dev)
        self._plans_built()

    def _seed_mse(self, dev) -> "L.SeedT":
        """dY_m = 2 (y_m - target) / (B (od + 2)) for every net m of the launch; the statistic is the sum over the nets of
        the mean squared error."""
        import numpy as np
        ws = G.SeedStat(dev, self.model.num_models, self.B)
        s = G._seed(L.SEED_MSE, self.B, 0, ws, self.st.stat_ptr(STAT_KEYS[0]))
        s.x0 = self.target.data_ptr()
        s.scale = s.stat_scale = float(np.float32(1.0) / np.float32(self.B * (self.model.state_dim + 2)))
        s._keep += [self.target]
        return s

    def _seed_nll(self, dev) -> "L.SeedT":
        """``OSRL_SEED_GAUSS_NLL`` (include/osrl_amd.h): the members' Gaussian negative log-likelihood against the same
        target table, the cost column by MSE; the statistic is the loss of the module docstring.  The log-variance
        bounds are by-value arguments of the launch, read from the model's buffers when the engine is built."""
        s = self._seed_mse(dev)
        s.kind = L.SEED_GAUSS_NLL
        s.gamma, s.thres = float(self.model.logvar_min.item()), float(self.model.logvar_max.item())
        return s

    def attach_replay(self, store) -> None:
        if store is not None:
            self.model.check_store(store)
        super().attach_replay(store)

    def body(self, device_noise: bool) -> None:
        m, st = self.model, self.st
        batch = (self.obs, self.nobs, self.act, self.rew, self.cost, self.done)
        # (a store built with state_init carries a 7th table, is_init, that the step does not read)
        fields = range(len(batch)) if self.replay is not None and self.replay.n_fields != len(batch) else None
        st.prologue(self.replay, batch, None, self.seed, device_noise, fields)
        L.check(L.load().osrl_dyn_prepare(self.obs.data_ptr(), self.nobs.data_ptr(), self.rew.data_ptr(),
                                          self.cost.data_ptr(), m.mu_s.data_ptr(), m.sd_s.data_ptr(), m.mu_d.data_ptr(),
                                          m.sd_d.data_ptr(), m.mu_r.data_ptr(), m.sd_r.data_ptr(), self.B, m.state_dim,
                                          self.xs.data_ptr(), self.target.data_ptr(), cur_stream()), "osrl_dyn_prepare")
        self.r_f.forward(self.xs, self.act)
        self.r_f.backward_dz(seed=self.seed_mse)
        self._optim("dynamics", self.plan)
