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

All members see the same minibatch rows.  By default their diversity comes from initialisation alone; ``bootstrap=True``
gives member m a Poisson(1) weight ``w_m(i)`` on every dataset row i -- a function of (``boot_seed``, the row's index in the
store, m) only, so each member is fitted on one fixed resample of the dataset (PETS / MBPO), with the loss still divided
by the batch size (csrc/dyn_loss.hip ``osrl_dyn_member_loss``).  In a ring store the weight belongs to the physical slot.
``boot_seed`` is a device word the kernel reads: it may be changed between steps without a recapture.

``num_elites=k`` keeps an ascending int64 buffer ``elites`` of k member indices (initially 0 .. k-1): ``set_elites`` /
``DynamicsTrainer.select_elites`` choose them (the k members of lowest holdout loss, ``DynamicsTrainer.validate``), and a
``ModelVecEnv`` steps the elites only -- mean, spread, max-std, the random member draw and halting all range over them.
Every member keeps training; elites affect rollouts only.  A model built with the defaults has the ``state_dict`` keys
and the launches it always had.

The six normaliser tables and the state bounds ``s_lo`` / ``s_hi`` are registered buffers, as are ``boot_seed`` and
``elites`` where the model has them: ``state_dict`` and the checkpoints carry them.  The arithmetic of the train step is
the HIP plan in ``osrl_amd/engine/dynamics.py``.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
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
                 device: str = "cuda", probabilistic: bool = False, logvar_min: float = -10.0, logvar_max: float = 0.5,
                 bootstrap: bool = False, boot_seed: int = 0, num_elites: Optional[int] = None):
        super().__init__()
        self.state_dim, self.action_dim = int(state_dim), int(action_dim)
        self.hidden_sizes, self.num_models = list(hidden_sizes), int(num_models)
        self.probabilistic, self.bootstrap = bool(probabilistic), bool(bootstrap)
        self.num_elites = None if num_elites is None else int(num_elites)
        self.elite_epoch = 0  # advanced by set_elites: a rollout rebuilds its descriptor (ModelVecEnv.launch_epoch)
        if not 1 <= self.num_models <= L.MAX_NETS:
            raise ValueError(f"num_models = {num_models}: the ensemble runs as one launch, 1 <= num_models <= {L.MAX_NETS}")
        if self.num_elites is not None and not 1 <= self.num_elites <= self.num_models:
            raise ValueError(f"num_elites = {num_elites}: 1 <= num_elites <= num_models = {self.num_models}")
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
        if self.bootstrap:  # a device word: the loss launch reads it, so a captured step follows a new value
            self.register_buffer("boot_seed", torch.full((1,), int(boot_seed) & 0x7FFFFFFFFFFFFFFF, dtype=torch.int64,
                                                         device=dev))
        if self.num_elites is not None:
            self.register_buffer("elites", torch.arange(self.num_elites, dtype=torch.int64, device=dev))
            self._elites_host = list(range(self.num_elites))  # host mirror of the buffer: no sync where a rollout asks
        self.seed = 0
        self._engine = None
        self._lrs: Optional[dict] = None

    def setup_optimizers(self, lr):
        self._lrs = dict(dynamics=lr)

    def _engine_class(self):
        cls = super()._engine_class()
        if self.bootstrap:  # the loss as a launch of its own, weighted per member and row (engine/dynamics.py)
            from ..engine.dynamics import BootDynamicsEngine as cls
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

    def set_elites(self, indices) -> None:
        """The members a ``ModelVecEnv`` steps from now on: exactly ``num_elites`` distinct indices below ``num_models``
        (ValueError otherwise), kept in ascending order.  Rollouts rebuild their descriptor and drop their captured
        graph at their next run."""
        if self.num_elites is None:
            raise ValueError("set_elites: build the Dynamics with num_elites=")
        idx = sorted(int(i) for i in np.asarray(indices).reshape(-1))
        if len(idx) != self.num_elites or len(set(idx)) != len(idx) or idx[0] < 0 or idx[-1] >= self.num_models:
            raise ValueError(f"set_elites: {self.num_elites} distinct member indices below {self.num_models}, got "
                             f"{list(np.asarray(indices).reshape(-1))}")
        self.elites.copy_(torch.as_tensor(idx, dtype=torch.int64))
        self._elites_host = idx
        self.elite_epoch += 1

    def elite_members(self) -> List[int]:
        """The elite member indices, ascending; every member when the model has no ``num_elites``."""
        return list(range(self.num_models)) if self.num_elites is None else list(self._elites_host)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        res = super().load_state_dict(state_dict, strict=strict, assign=assign)
        if self.num_elites is not None:  # (the elites may have changed)
            idx = sorted(int(i) for i in self.elites.cpu().tolist())
            if len(set(idx)) != len(idx) or idx[0] < 0 or idx[-1] >= self.num_models:
                raise ValueError(f"load_state_dict: elites {idx} are not distinct member indices below {self.num_models}")
            self.elites.copy_(torch.as_tensor(idx, dtype=torch.int64))
            self._elites_host = idx
            self.elite_epoch += 1
        return res

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
    (cost - t_cost)^2] / (B (od + 2))``, the Gaussian negative log-likelihood up to a constant (it may be negative).  On a
    ``bootstrap`` model every row's term is weighted by that member's bootstrap weight (still divided by B).
    ``validate`` is the holdout loss per member, ``select_elites`` ranks the members by it."""

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

    def train_one_step(self, observations, next_observations, actions, rewards, costs, done=None, row_ids=None):
        """``row_ids`` (int32 ``[B]``): the batch rows' indices in the dataset -- what a ``bootstrap`` model's weights are
        keyed by, so such a model needs them (ValueError without); any other model ignores them."""
        eng = self.model.engine(observations.shape[0])
        if self.model.bootstrap:
            if row_ids is None:
                raise ValueError("a bootstrap model weighs every batch row by its dataset index: pass row_ids= (int32 [B])")
            eng.load_row_ids(row_ids)
        eng.step(observations, next_observations, actions, rewards, costs, eng.done if done is None else done,
                 use_graph=self.use_graph)
        from ..common.logger import store_stats
        store_stats(self.logger, eng.st, self.stats_mode)

    # ---- holdout loss and elite selection ---------------------------------------------------------------------------------
    def _holdout_tables(self, data):
        """(observations, next_observations, actions, rewards, costs) of ``data`` as contiguous fp32 device tensors: a
        ``ReplayStore``'s live rows, rewards as the store scales them, or a DSRL-layout mapping."""
        m = self.model
        dev = m.mu_s.device
        if hasattr(data, "tables"):
            m.check_store(data)
            t = [data.live(i) for i in range(5)]
            t[3] = t[3] * float(data.scales[3])
        else:
            t = [torch.as_tensor(data[k]) for k in ("observations", "next_observations", "actions", "rewards", "costs")]
        n = int(t[0].shape[0])
        t = [x.to(dev, torch.float32).reshape(n, -1).contiguous() for x in t]
        if n < 1 or [x.shape[1] for x in t] != [m.state_dim, m.state_dim, m.action_dim, 1, 1]:
            raise ValueError(f"validate: >= 1 rows of ({m.state_dim}, {m.state_dim}, {m.action_dim}, 1, 1)-wide observations, "
                             f"next_observations, actions, rewards, costs; got {[tuple(x.shape) for x in t]}")
        return t

    @torch.no_grad()
    def validate(self, data, chunk_rows: int = 1024) -> np.ndarray:
        """The holdout loss: per member the UNWEIGHTED mean loss ``sum_r l_m(r) / (rows (od + 2))`` over ``data`` (a
        ``ReplayStore``, its live rows, or a DSRL-layout mapping) in the model's normalised units, float64
        ``[num_models]`` -- the mean squared error, or for a ``probabilistic`` model the Gaussian negative log-likelihood
        of the train step's statistic.  Chunk by chunk: ``osrl_dyn_prepare`` -> the members' forward on 16-row tiles ->
        ``osrl_dyn_member_loss`` (row losses only) -> ``osrl_fqe_value_sums`` into ``num_models`` device doubles.
        ``chunk_rows`` is rounded up to whole periods of the forward's k-walk (``validate_unit``), so that a row's loss
        has the same bits at every chunk size and the result depends on it through the order of the fp64 sums alone.
        Reads the parameters; touches neither them, the optimizer state, the step counter nor the train graph.
        Synchronises."""
        from ..engine.core import MlpRun, cur_stream
        from ..engine.dynamics import member_loss, member_loss_desc
        m, lib = self.model, L.load()
        if int(chunk_rows) < 1:
            raise ValueError(f"validate: chunk_rows = {chunk_rows} must be >= 1")
        unit = validate_unit([m.state_dim + m.action_dim] + m.hidden_sizes)
        chunk = (int(chunk_rows) + unit - 1) // unit * unit
        obs, nobs, act, rew, cost = self._holdout_tables(data)
        n, od, E, dev = obs.shape[0], m.state_dim, m.num_models, obs.device
        m.repack()
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)  # noqa: E731
        acc = torch.zeros(E, dtype=torch.float64, device=dev)
        from ..common.net import net_desc_seq
        nd, runs = net_desc_seq(list(m.members), 1.0), {}
        for r0 in range(0, n, chunk):
            k = min(chunk, n - r0)
            if k not in runs:  # (at most two sizes: the chunk and a partial last one)
                run, xs, target, row_loss = MlpRun(nd, k, False, dev, tile_rows=16), z(k, od), z(k, od + 2), z(E, k)
                runs[k] = (run, xs, target, row_loss, member_loss_desc(m, run.y, target, k, row_loss=row_loss))
            run, xs, target, row_loss, d = runs[k]
            o = obs[r0:r0 + k]
            L.check(lib.osrl_dyn_prepare(o.data_ptr(), nobs[r0:r0 + k].data_ptr(), rew[r0:r0 + k].data_ptr(),
                                         cost[r0:r0 + k].data_ptr(), m.mu_s.data_ptr(), m.sd_s.data_ptr(),
                                         m.mu_d.data_ptr(), m.sd_d.data_ptr(), m.mu_r.data_ptr(), m.sd_r.data_ptr(), k, od,
                                         xs.data_ptr(), target.data_ptr(), cur_stream()), "osrl_dyn_prepare")
            run.forward(xs, act[r0:r0 + k])
            member_loss(d)
            L.check(lib.osrl_fqe_value_sums(row_loss.data_ptr(), E, k, acc.data_ptr(), cur_stream()),
                    "osrl_fqe_value_sums")
        return acc.cpu().numpy() / float(n * (od + 2))

    def select_elites(self, data, k: Optional[int] = None) -> np.ndarray:
        """``validate(data)``, then ``model.set_elites`` with the ``k`` members of lowest loss (None: the model's
        ``num_elites``, which ``k`` must equal: the buffer has that many entries); a stable sort, so ties go to the lower
        index.  Returns the losses."""
        m = self.model
        if m.num_elites is None or (k is not None and int(k) != m.num_elites):
            raise ValueError(f"select_elites(k={k}): the model was built with num_elites={m.num_elites}")
        losses = self.validate(data)
        m.set_elites(elite_indices(losses, m.num_elites))
        return losses


def validate_unit(layer_inputs, limit: int = 1 << 16) -> int:
    """The row count ``validate``'s chunks are multiples of.  The tile kernels' forward starts a workgroup's walk over a
    layer's 16-wide k-steps at step ``(5 tile + ..) mod n`` (csrc/mlp_common.h ``k_rot``; n = the layer's k-steps, or a
    wave's quarter of them where the four waves split K), so the fp32 sum order of a row depends on its tile's index in
    the launch modulo those n.  A chunk of ``16 lcm(n)`` rows keeps every row's index the same modulo each n at every
    chunk size.  ``layer_inputs``: the input width of every layer.  Where the period exceeds ``limit`` rows (unusual
    width mixes) the unit is one 16-row tile and two chunk sizes agree to fp32 rounding only."""
    p = 1
    for width in layer_inputs:
        nk = (int(width) + 15) // 16
        for n in (nk, nk // 4, (nk + 3) // 4):
            if n > 1:
                p = int(np.lcm(p, n))
    return 16 * p if 16 * p <= limit else 16


def elite_indices(losses, k: int) -> List[int]:
    """The ``k`` members of lowest loss, ties to the lower index (a stable sort), ascending."""
    order = np.argsort(np.asarray(losses, np.float64), kind="stable")[:int(k)]
    return sorted(int(i) for i in order)
