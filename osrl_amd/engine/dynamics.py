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

A ``bootstrap`` model takes ``BootDynamicsEngine``: the loss is a launch of its own (csrc/dyn_loss.hip
``osrl_dyn_member_loss``) between the forward and an unseeded backward launch, so that every member's output gradient can
be scaled row by row with that member's Poisson(1) bootstrap weight.  The weight is a function of (``model.boot_seed``,
the row's index in the store, the member): the gather writes the drawn row indices beside the batch, the loss launch
turns them into weights.  The minibatch rows are those a default engine draws at the same seed and step; the statistic is
the weighted loss, still divided by the batch size.  ``validate`` (algorithms/dynamics.py) uses the same launch for the
unweighted per-row losses of a holdout set.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
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


def member_loss_desc(model, y: torch.Tensor, target: torch.Tensor, rows: int, idx=None, dy=None, row_loss=None,
                     weights_out=None, stat: int = 0, ws=None, scale: float = 0.0, stat_scale: float = 0.0) -> "L.DynLossT":
    """The ``osrl_dyn_loss_t`` of ``model``'s members on ``rows`` rows: ``y`` the forward launch's output, ``target``
    ``osrl_dyn_prepare``'s table; ``idx`` (int32 ``[rows]``, the rows' indices in the store) turns the bootstrap weights
    on; ``stat`` the address of the statistic with ``ws`` its ``DynLossStat`` scratch.  The log-variance bounds are
    by-value arguments, read from the model's buffers here."""
    d = L.DynLossT()
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    d.y, d.target, d.idx, d.dy, d.row_loss, d.weights_out = p(y), p(target), p(idx), p(dy), p(row_loss), p(weights_out)
    if idx is not None:
        assert idx.dtype == torch.int32 and idx.numel() >= rows
        d.boot_seed = model.boot_seed.data_ptr()
    if stat:
        d.stat, d.partials, d.counter = stat, ws.partials.data_ptr(), ws.counter.data_ptr()
    d.n_nets, d.rows, d.state_dim = model.num_models, int(rows), model.state_dim
    d.kind = L.DYN_LOSS_GAUSS_NLL if model.probabilistic else L.DYN_LOSS_MSE
    if model.probabilistic:
        d.lo, d.hi = float(model.logvar_min.item()), float(model.logvar_max.item())
    d.scale, d.stat_scale = float(scale), float(stat_scale)
    d._keep = [y, target, idx, dy, row_loss, weights_out, ws]
    return d


def member_loss(d: "L.DynLossT") -> None:
    L.check(L.load().osrl_dyn_member_loss(C.byref(d), cur_stream()), "osrl_dyn_member_loss")


class DynLossStat:
    """Scratch of one ``osrl_dyn_member_loss`` call site that logs a statistic: one partial per ``OSRL_DYN_LOSS_TILE``
    rows + the arrival counter."""

    def __init__(self, device, rows: int):
        self.partials = torch.zeros((rows + L.DYN_LOSS_TILE - 1) // L.DYN_LOSS_TILE, dtype=torch.float32, device=device)
        self.counter = torch.zeros(1, dtype=torch.int32, device=device)


class BootDynamicsEngine(DynamicsEngine):
    """The train step of a ``bootstrap`` model (the module docstring): tick -> gather (+ the drawn row indices) ->
    ``osrl_dyn_prepare`` -> forward -> ``osrl_dyn_member_loss`` -> backward -> dW + Adam, one chain, one one-step graph."""

    def __init__(self, model, batch_size: int, seed: int = 0, dist=None):
        super().__init__(model, batch_size, seed=seed, dist=dist)
        dev = torch.device(model.device)
        self.row_idx = torch.zeros(self.B, dtype=torch.int32, device=dev)
        s = float(np.float32(1.0) / np.float32(self.B * (model.state_dim + 2)))
        self.loss_d = member_loss_desc(model, self.r_f.y, self.target, self.B, idx=self.row_idx, dy=self.dy,
                                       stat=self.st.stat_ptr(STAT_KEYS[0]), ws=DynLossStat(dev, self.B), scale=s,
                                       stat_scale=s)

    def load_row_ids(self, row_ids) -> None:
        """The caller batch's dataset indices (int32 ``[B]``): what the bootstrap weights are keyed by."""
        t = torch.as_tensor(row_ids)
        if t.numel() != self.B or t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"row_ids: {self.B} integer dataset indices, got {tuple(t.shape)} {t.dtype}")
        self.row_idx.copy_(t.reshape(-1).to(torch.int32), non_blocking=True)

    def body(self, device_noise: bool) -> None:
        m, st = self.model, self.st
        batch = (self.obs, self.nobs, self.act, self.rew, self.cost, self.done)
        st.tick()
        if self.replay is not None:  # the rows the fused prologue would draw: a function of (seed, step, row) alone
            if self.replay.n_fields != len(batch):
                self.replay.gather_fields(range(len(batch)), batch, st.ptr, idx_out=self.row_idx)
            else:
                self.replay.gather(batch, st.ptr, idx_out=self.row_idx)
        L.check(L.load().osrl_dyn_prepare(self.obs.data_ptr(), self.nobs.data_ptr(), self.rew.data_ptr(),
                                          self.cost.data_ptr(), m.mu_s.data_ptr(), m.sd_s.data_ptr(), m.mu_d.data_ptr(),
                                          m.sd_d.data_ptr(), m.mu_r.data_ptr(), m.sd_r.data_ptr(), self.B, m.state_dim,
                                          self.xs.data_ptr(), self.target.data_ptr(), cur_stream()), "osrl_dyn_prepare")
        self.r_f.forward(self.xs, self.act)
        member_loss(self.loss_d)
        self.r_f.backward_dz()
        self._optim("dynamics", self.plan)
