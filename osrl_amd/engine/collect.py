"""Datasets made on device: the batched rollout of ``engine/rollout.py`` with per-episode exploration noise, every
transition recorded in HBM under the seven DSRL keys ("Collecting datasets on device").

``Collector`` is a ``BatchedRollout`` whose step ends in ``osrl_env_collect`` (csrc/collect.hip) instead of
``osrl_env_step``: same policy launches, same environment arithmetic, plus the noise on the action, one table row per
episode and step, and the discounted sums.  What comes out goes into ``ReplayStore`` / ``SequenceStore.from_dataset`` /
``process_bc_dataset`` as it is -- collect -> store -> train -> evaluate -> FQE without leaving the device.

Noise: ``a = clip(pi(s) + sigma_e * eps)``.  ``eps`` is Philox4x32-10 keyed by (seed, episode id = base_seed + e, the
episode's own step, action column) on stream ``_EPS_STREAM``: it does not depend on E, on the graph chunking or on which
replay a step falls in.  Seed, gamma and sigma live in device memory, so a captured graph follows them.

``CDTCollector`` is the same for CDT (``CDTTrainer.collect_targets``): a ``CDTBatchedRollout`` whose step after the
transformer forward is the one launch ``osrl_cdt_collect`` (csrc/cdt_collect.hip) instead of pick, environment, push and
cursor, with per-episode targets and, with ``sample=True``, the Gaussian head's own standard deviation as the noise scale.

``ModelCollector`` is ``Collector`` on a learned model (``Trainer.collect_model``): the step ends in
``osrl_model_env_collect`` (csrc/model_env.hip), episodes start at the environment's initial states or at rows drawn on
device from a store (``osrl_model_env_branch``, Philox stream 15), and run ``horizon`` steps -- MOPO's / MBPO's branched
rollouts (DESIGN.md "Training on a learned model").  On an environment with a ``halt_threshold`` an episode may end early:
the run then compacts the tables on device (csrc/compact.hip ``osrl_collect_compact``) and hands out the live rows only.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from .. import _lib as L
from .core import cur_stream
from .rollout import _CHUNK, BatchedRollout, CDTBatchedRollout, cached

_EPS_STREAM = 13   # Philox stream id of the exploration noise (11 / 12: the BCQL decode noise of rollout.py / fqe.py)
_GUARD_ROWS = 4    # sentinel rows before and after every table (``Collector.guards_intact``)
_SENTINEL = 0x5EA7BEEF
KEYS = ("observations", "actions", "next_observations", "rewards", "costs", "terminals", "timeouts")


class Collected(NamedTuple):
    """``dataset``: fresh device tensors under the seven DSRL keys, ``E * L`` rows, episode-major (row ``e * L + t``);
    costs raw 0 / 1, ``terminals`` all 0, ``timeouts`` 1 on each episode's last row (``collect_model`` on an environment that
    can halt: ``sum(lengths)`` rows, dense and episode-major, ``terminals`` 1 and ``timeouts`` 0 on a halting row).  The per-episode sums are numpy
    fp64 ``[E]``; the two cost sums carry the collector's ``cost_scale`` (as ``BatchedRollout.run``'s do), the discounted
    ones weigh step t by ``gamma ** t``.  ``dataset`` is None when the run appended its rows to a store (``into=``).
    From ``collect_jobs`` (host environments, engine/act.py): one entry per JOB, the rows job-major with each job's true
    length, ``terminals`` 1 where the environment terminated and ``timeouts`` 1 where it truncated or reached
    ``episode_len``, and the sums accumulated on the host in fp64."""
    dataset: Optional[Dict[str, torch.Tensor]]
    returns: np.ndarray
    cost_returns: np.ndarray
    lengths: np.ndarray
    disc_returns: np.ndarray
    disc_cost_returns: np.ndarray


def merge_datasets(datasets: List[Dict[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
    """Several collections as one dataset: a ``torch.cat`` per key, in the order given."""
    if not datasets:
        raise ValueError("merge_datasets needs at least one dataset")
    return {k: torch.cat([d[k] for d in datasets], 0) for k in datasets[0]}


def _check_replay_store(into, state_dim: int, action_dim: int, who: str = "collect", weighted_ok: bool = False) -> None:
    """``into=`` a ``ReplayStore``: ValueError unless it grows, draws uniformly (``weighted_ok``: the caller has its own
    rule for weights) and has the environment's widths."""
    if into is None:
        return
    if getattr(into, "capacity", None) is None:
        raise ValueError(f"{who}(into=): the store is fixed, build it with capacity=")
    if into.weighted and not weighted_ok:
        raise ValueError("collect(into=): the store draws by weight; collect a dataset and append it with sample_prob=")
    into.check_append_widths(observations=state_dim, next_observations=state_dim, actions=action_dim)


class _Tables:
    """What the collectors share: the guarded tables, the ``osrl_collect_t`` descriptor, the noise parameters that live in
    device memory, and the start (``_begin``) and the recorded loop (``_drive_recorded``) of a run.  The host class is a
    rollout of engine/rollout.py with a ``seed``."""

    def _init_tables(self) -> None:
        dev, E = self.obs.device, self.venv.E
        self.disc = torch.zeros(E, 4, dtype=torch.float32, device=dev)
        self.sigma = torch.zeros(E, dtype=torch.float32, device=dev)
        self.gamma = torch.ones(1, dtype=torch.float32, device=dev)
        self.seed_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self.bufs: Dict[str, torch.Tensor] = {}
        self.tables: Dict[str, torch.Tensor] = {}
        self.rec: Optional[L.CollectT] = None
        self._eps: Optional[torch.Tensor] = None  # the injected noise of the run in progress
        self._steps = 0                           # rows per episode of the tables

    def _alloc(self, steps: int) -> None:
        E, od, ad, dev = self.venv.E, self.venv.state_dim, self.model.action_dim, self.obs.device
        n, g = E * steps, _GUARD_ROWS
        self.bufs, self.tables, self._steps = {}, {}, steps
        for k in KEYS:
            w = {"observations": od, "next_observations": od, "actions": ad}.get(k, 0)  # 0: a 1-D table, as DSRL's are
            buf = torch.full(((n + 2 * g) * max(w, 1),), _SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
            body = buf[g * max(w, 1):(g + n) * max(w, 1)]
            self.bufs[k], self.tables[k] = buf, body.view(n, w) if w else body
        r = self.rec = L.CollectT()
        for k in KEYS:
            setattr(r, k, self.tables[k].data_ptr())
        r.disc, r.sigma, r.gamma = self.disc.data_ptr(), self.sigma.data_ptr(), self.gamma.data_ptr()
        r.seed, r.eps_in = self.seed_dev.data_ptr(), None
        r.episode_base, r.stream_id = self.venv.base_seed & 0xFFFFFFFF, _EPS_STREAM

    def guards_intact(self) -> bool:
        """True while the sentinel rows around every table hold their pattern (one host sync: a diagnostic)."""
        ok = torch.ones((), dtype=torch.bool, device=self.obs.device)
        for k, buf in self.bufs.items():
            w = buf.numel() // (self.tables[k].shape[0] + 2 * _GUARD_ROWS)
            i = buf.view(torch.int32)
            ok = ok & (i[:_GUARD_ROWS * w] == _SENTINEL).all() & (i[-_GUARD_ROWS * w:] == _SENTINEL).all()
        return bool(ok.item())

    def _rec_now(self) -> L.CollectT:
        """The descriptor of the step being issued: in an eager run with injected noise, a copy with the tensor's address."""
        if self._eps is None:
            return self.rec
        rec = L.CollectT.from_buffer_copy(self.rec)
        rec.eps_in = self._eps.data_ptr()
        return rec

    def _load_noise(self, noise_std, gamma: Optional[float], noise, steps: int) -> Optional[torch.Tensor]:
        """``noise_std`` and the injected ``noise`` checked (the one place: ValueError before anything is launched), then
        sigma, gamma and ``self.seed`` into their device words and the noise onto the device."""
        E, ad, dev = self.venv.E, self.model.action_dim, self.obs.device
        if (noise_std.dim() if torch.is_tensor(noise_std) else np.ndim(noise_std)) != 0:
            noise_std = torch.as_tensor(noise_std, dtype=torch.float32).reshape(-1)
            if noise_std.numel() != E:
                raise ValueError(f"noise_std holds {noise_std.numel()} values, the environment {E} episodes")
        if noise is not None:
            noise = torch.as_tensor(noise, dtype=torch.float32)
            if tuple(noise.shape) != (steps, E, ad):
                raise ValueError(f"noise must be [{steps}, {E}, {ad}] (steps, episodes, action_dim), "
                                 f"got {tuple(noise.shape)}")
            noise = noise.to(dev).contiguous()
        if torch.is_tensor(noise_std) and noise_std.dim():
            self.sigma.copy_(noise_std, non_blocking=True)
        else:
            self.sigma.fill_(float(noise_std))
        self.gamma.fill_(1.0 if gamma is None else float(gamma))
        s64 = self.seed & 0xFFFFFFFFFFFFFFFF
        self.seed_dev.fill_(s64 - (1 << 64) if s64 >= (1 << 63) else s64)
        return noise

    def _begin(self, steps: int, seed: Optional[int], noise_std, gamma, noise) -> Optional[torch.Tensor]:
        """The start of every recorded run, after the caller's own argument checks: the seed taken (BCQ-L's decode noise
        has it as a by-value argument of its launch: a new one drops the graph), the noise checked and loaded, the
        environment descriptor and the tables brought to ``steps`` (by-value arguments too).  Returns the injected noise
        on the device, or None."""
        if seed is not None and int(seed) != self.seed:
            self.seed = int(seed)
            if getattr(self, "kind", None) == "bcql" and not self.z_fixed:
                self.graph = None
        noise = self._load_noise(noise_std, gamma, noise, steps)
        self._sync_desc(steps)
        if self.rec is None or self._steps != steps:
            self._alloc(steps)
            self.graph = None
        return noise

    def _reset_disc(self) -> None:
        self.disc.zero_()
        self.disc[:, 2] = 1.0

    def _drive_recorded(self, steps: int, chunk: int, noise: Optional[torch.Tensor]) -> None:
        """``_drive`` with the injected noise, if any, visible to ``body`` while it runs (the run is then eager)."""
        self._eps = noise
        try:
            self._drive(steps, chunk, self.use_graph and noise is None)
        finally:
            self._eps = None

    def _finish(self, into, sample_prob=None) -> Collected:
        """The tables into the store or out as copies, and the per-episode sums (the one host sync of the run)."""
        if into is not None:  # (every episode starts at an initial state: the chunk's is_init is right by construction)
            if sample_prob is None:
                into.append(self.tables)
            else:
                into.append(self.tables, sample_prob=sample_prob)
            data = None
        else:
            data = {k: t.clone() for k, t in self.tables.items()}
        tot = torch.cat([self.venv.acc, self.disc], 1).cpu().numpy().astype(np.float64)
        return Collected(data, tot[:, 0], tot[:, 1], tot[:, 2], tot[:, 4], tot[:, 5])


class _DenseTables(_Tables):
    """A second set of guarded tables as large as ``owner``'s, ``row_unc`` included: where ``osrl_collect_compact``
    writes.  The descriptor's other words are the owner's; the compaction reads the seven tables only."""

    def __init__(self, owner):
        self.obs, self.venv, self.model = owner.obs, owner.venv, owner.model
        self.disc, self.sigma, self.gamma, self.seed_dev = owner.disc, owner.sigma, owner.gamma, owner.seed_dev
        self._alloc(owner._steps)
        self._unc_buf, self._row_unc = owner._alloc_unc(owner._steps)


class Collector(_Tables, BatchedRollout):
    """``run`` = all ``venv.E`` episodes to completion, recorded.  The tables are this object's (sized at the first run,
    again when the episode length changes); ``run`` hands out copies, or appends the tables to a store (``into=``)."""

    def __init__(self, model, venv, kind: str, cost_scale: float = 1.0, extra_obs: Optional[float] = None,
                 seed: int = 0, z: Optional[torch.Tensor] = None, use_graph: bool = True):
        super().__init__(model, venv, kind, cost_scale, extra_obs, seed, z, use_graph)
        self._init_tables()

    def body(self) -> None:
        act = self.policy()
        v = self.venv
        L.check(L.load().osrl_env_collect(self.env_c, self._rec_now(), act.data_ptr(), v.state.data_ptr(),
                                          self.obs.data_ptr(), self.obs.stride(0), v.acc.data_ptr(), v.E, cur_stream()),
                "osrl_env_collect")

    def _snapshot(self):
        return super()._snapshot() + [(self.disc, self.disc.clone())]

    @torch.no_grad()
    def run(self, noise_std=0.0, gamma: Optional[float] = None, seed: Optional[int] = None,
            noise: Optional[torch.Tensor] = None, into=None) -> Collected:
        """``noise_std``: one sigma for all episodes or ``[E]`` of them.  ``gamma`` (None: 1.0) weighs the discounted
        sums.  ``seed`` (None: keep the current one) keys the noise drawn on device.  ``noise``: ``[L, E, action_dim]``
        injected instead (the run is then eager); rows of episodes whose sigma is 0 are not read.  ``into``: a
        ``ReplayStore`` built with ``capacity`` -- the tables go straight into ``into.append`` (one device copy per
        table, no clone) and the result's ``dataset`` is None; a store whose widths differ from the environment's
        (BC multi-task appends the cost return to the observations) is a ValueError before the run."""
        _check_replay_store(into, self.venv.state_dim, self.model.action_dim)
        steps = self._episode_steps()
        noise = self._begin(steps, seed, noise_std, gamma, noise)
        self.venv.reset(self.obs)
        self._reset_disc()
        self._drive_recorded(steps, _CHUNK, noise)
        return self._finish(into)


def check_model_target(into, start, state_dim: int, action_dim: int, rows: int, sample_prob, halting: bool = False):
    """``collect_model``'s ``into=`` / ``sample_prob=`` / ``start=``, judged on the host before anything runs: the new
    rows' weights as a flat fp64 tensor (None on a uniform target).  ``_check_replay_store``'s width rules, except that a
    weighted store is taken WITH ``sample_prob`` (a scalar or ``[rows]``); ValueError for a weighted store without it, a
    uniform one (or no store) with it, a ``state_init`` target of branched rollouts (a branch start is not an initial
    state: ``is_init`` and every FQE read-out would be wrong), and a ``start`` store of another observation width.
    ``halting``: the environment can end an episode early -- ``rows`` is then the worst case ``E * horizon``, and a per-row
    ``sample_prob`` is refused: the number of rows is known only after the run."""
    from ..common.replay import _checked_weights
    if halting and sample_prob is not None and \
            (sample_prob.dim() if torch.is_tensor(sample_prob) else np.ndim(sample_prob)) != 0:
        raise ValueError("collect_model(sample_prob=) on an environment that can halt: the number of rows is known only "
                         "after the run, pass one value for all of them")
    if start is not None:
        if not hasattr(start, "tables") or not hasattr(start, "widths"):
            raise ValueError(f"start= takes a ReplayStore (or None: the environment's own initial states), not "
                             f"{type(start).__name__}")
        if start.widths[0] != state_dim:
            raise ValueError(f"start=: the store's observations have {start.widths[0]} columns, the model's states "
                             f"{state_dim}")
        if start.n_rows < 1:
            raise ValueError("start=: the store is empty")
    if into is None:
        if sample_prob is not None:
            raise ValueError("sample_prob= are the weights of rows appended to a store: pass into=")
        return None
    _check_replay_store(into, state_dim, action_dim, "collect_model", weighted_ok=True)
    if into.weighted and sample_prob is None:
        raise ValueError("collect_model(into=): the store draws by weight, pass the new rows' sample_prob=")
    if not into.weighted and sample_prob is not None:
        raise ValueError("collect_model(into=): the store draws uniformly, sample_prob= has no table to go to")
    if start is not None and getattr(into, "state_init", False):
        raise ValueError("collect_model(start=store, into=): a branch start is not an initial state, a state_init store "
                         "would mark it as one")
    if sample_prob is None:
        return None
    if (sample_prob.dim() if torch.is_tensor(sample_prob) else np.ndim(sample_prob)) == 0:
        sample_prob = np.full(rows, float(sample_prob), np.float64)
    return _checked_weights(sample_prob, rows, "transition", positive_sum=False)


class ModelCollector(_Tables, BatchedRollout):
    """``Collector`` on a ``ModelVecEnv``: the evaluating rollout's policy launches, then ``osrl_model_env_collect``
    (csrc/model_env.hip) where the evaluating rollout issues ``osrl_model_env_step`` -- the same step behind a compile-time
    flag, so without noise a run is ``BatchedRollout.run``'s bit for bit.  ``run`` rolls every episode ``horizon`` steps
    from the environment's initial states or from rows of a store (``osrl_model_env_branch``: one launch, drawn on
    device from the store's live count) and records them with the penalised reward.  What comes out is a model's
    opinion.  ``start_rows`` (int64 ``[E]``, None without a start store) and ``row_disagreement`` (``[E * horizon]``, the
    members' disagreement at each recorded row) are device tensors of the last run.

    On an environment that can halt (``venv.can_halt``) an episode may end before ``horizon``: the run then ends with
    ``osrl_collect_compact`` (csrc/compact.hip) into a second set of guarded tables and reads the row count -- the one
    extra host sync.  ``dataset`` / ``into=`` / ``row_disagreement`` hold the ``sum(len_e)`` live rows, episode-major and
    dense; ``row_offsets`` (int64 ``[E + 1]`` on the device, None otherwise) says where each episode's rows start."""

    def __init__(self, model, venv, kind: str, cost_scale: float = 1.0, extra_obs: Optional[float] = None,
                 seed: int = 0, z: Optional[torch.Tensor] = None, use_graph: bool = True):
        from ..common.model_env import ModelVecEnv
        if not isinstance(venv, ModelVecEnv):
            raise TypeError(f"collect_model() records rollouts on a learned model: a ModelVecEnv, not "
                            f"{type(venv).__name__}")
        super().__init__(model, venv, kind, cost_scale, extra_obs, seed, z, use_graph)
        self._init_tables()
        self._starts = torch.zeros(venv.E, dtype=torch.int64, device=self.obs.device)
        self.start_rows: Optional[torch.Tensor] = None
        self.row_disagreement: Optional[torch.Tensor] = None
        self.row_offsets: Optional[torch.Tensor] = None
        self._offsets = torch.zeros(venv.E + 1, dtype=torch.int64, device=self.obs.device)
        self._dense: Optional[_Tables] = None  # the compaction's destination: tables of the same size, guarded alike

    def _alloc(self, steps: int) -> None:
        super()._alloc(steps)
        self._unc_buf, self._row_unc = self._alloc_unc(steps)
        self.row_disagreement, self._dense = self._row_unc, None

    def _alloc_unc(self, steps: int):
        n, g = self.venv.E * steps, _GUARD_ROWS
        buf = torch.full((n + 2 * g,), _SENTINEL, dtype=torch.int32, device=self.obs.device).view(torch.float32)
        return buf, buf[g:g + n]

    @staticmethod
    def _unc_guards(buf) -> torch.Tensor:
        i = buf.view(torch.int32)
        return (i[:_GUARD_ROWS] == _SENTINEL).all() & (i[-_GUARD_ROWS:] == _SENTINEL).all()

    def guards_intact(self) -> bool:
        ok = super().guards_intact() and bool(self._unc_guards(self._unc_buf).item())
        if ok and self._dense is not None:
            ok = self._dense.guards_intact() and bool(self._unc_guards(self._dense._unc_buf).item())
        return ok

    def _compact(self) -> int:
        """The padded tables' live rows into the dense ones (allocated at the first halting run of this horizon):
        ``osrl_collect_compact``, then the row count -- a host sync."""
        v = self.venv
        if self._dense is None:
            self._dense = _DenseTables(self)
        d = self._dense
        L.check(L.load().osrl_collect_compact(self.rec, self._row_unc.data_ptr(), d.rec, d._row_unc.data_ptr(),
                                              v.acc.data_ptr(), self._offsets.data_ptr(), v.E, self._steps, v.state_dim,
                                              self.model.action_dim, cur_stream()), "osrl_collect_compact")
        return int(self._offsets[v.E].item())

    def _finish(self, into, sample_prob=None) -> Collected:
        if not self.venv.can_halt:
            self.row_disagreement, self.row_offsets = self._row_unc, None
            return super()._finish(into, sample_prob)
        n = self._compact()
        tables = {k: t[:n] for k, t in self._dense.tables.items()}
        self.row_disagreement, self.row_offsets = self._dense._row_unc[:n], self._offsets
        if into is not None:
            if n:
                if sample_prob is None:
                    into.append(tables)
                else:  # (a scalar, spread over the worst case before the run: the live rows' share of it)
                    into.append(tables, sample_prob=sample_prob[:n])
            data = None
        else:
            data = {k: t.clone() for k, t in tables.items()}
        tot = torch.cat([self.venv.acc, self.disc], 1).cpu().numpy().astype(np.float64)
        return Collected(data, tot[:, 0], tot[:, 1], tot[:, 2], tot[:, 4], tot[:, 5])

    def body(self) -> None:
        import ctypes as C
        act = self.policy()
        v = self.venv
        # (a probabilistic model's descriptor: the sampled next state and the penalised reward are what is recorded)
        c = self.env_c
        if isinstance(c, L._HaltDesc):  # halting / the pessimistic cost: the same descriptor beside osrl_model_env_pess_t
            name, head = c.collect_fn, (C.byref(c.env), C.byref(c.pess))
        else:
            name = "osrl_model_env_collect_gauss" if isinstance(c, L.ModelEnvGaussT) else "osrl_model_env_collect"
            head = (C.byref(c),)
        L.check(getattr(L.load(), name)(*head, self._rec_now(), act.data_ptr(), v.state.data_ptr(),
                                        self.obs.data_ptr(), self.obs.stride(0), v.acc.data_ptr(), v.unc.data_ptr(),
                                        self._row_unc.data_ptr(), v.E, cur_stream()), name)

    def _snapshot(self):  # (venv.unc is the environment's extra_state: the base class has it)
        return super()._snapshot() + [(self.disc, self.disc.clone())]

    def _branch(self, store) -> None:
        """One launch: a start row per episode, uniform over the store's pinned prefix when it has one, else over its
        live rows (read from the live-count word: the draw follows ``append`` without a host sync), whatever sampling
        weights the store carries -- weighted starts are out of scope."""
        v = self.venv
        fixed = store.capacity is None
        L.check(L.load().osrl_model_env_branch(
            store.tables[0].data_ptr(), store.n_rows if fixed else store.capacity, store._live_ptr(),
            int(getattr(store, "pinned_rows", 0)), v.state_dim, self.seed_dev.data_ptr(), v.base_seed & 0xFFFFFFFF,
            v.state.data_ptr(), self.obs.data_ptr(), self.obs.stride(0), v.acc.data_ptr(), v.unc.data_ptr(),
            self.disc.data_ptr(), self._starts.data_ptr(), v.E, cur_stream()), "osrl_model_env_branch")
        if v.can_halt:  # (otherwise it holds -1 already: ModelVecEnv.reset's rule)
            v.halt_step.fill_(-1)
        self.start_rows = self._starts

    @torch.no_grad()
    def run(self, horizon: Optional[int] = None, start=None, noise_std=0.0, gamma: Optional[float] = None,
            seed: Optional[int] = None, noise: Optional[torch.Tensor] = None, into=None, sample_prob=None) -> Collected:
        """``horizon`` (None: the environment's ``episode_len``) steps of every episode, from the environment's initial
        states (``start=None``) or from rows of the ``ReplayStore`` ``start``.  ``noise_std``, ``gamma``, ``seed`` and
        ``noise`` (``[horizon, E, action_dim]``) as ``Collector.run`` takes them; ``seed`` keys the branch starts too
        (Philox stream 15; the noise is stream 13).  ``into`` / ``sample_prob``: ``check_model_target``.  Every refusal
        comes before the first launch.  ``min(horizon, _CHUNK)`` steps per captured graph; the graph is dropped when the
        horizon or a by-value argument of the environment (mode, member, penalty: ``launch_epoch``) changes.  On an
        environment that can halt the result holds the live rows only (the class docstring), ``into`` / ``sample_prob``
        are still judged for the worst case ``E * horizon``, and ``sample_prob`` is a scalar: a per-row vector has no
        rows to belong to before the lengths exist."""
        v = self.venv
        steps = int(v.episode_len if horizon is None else horizon)
        if steps < 1:
            raise ValueError(f"horizon {steps}: at least one step")
        w_new = check_model_target(into, start, v.state_dim, self.model.action_dim, v.E * steps, sample_prob, v.can_halt)
        if start is not None and torch.device(start.device) != self.obs.device:
            raise ValueError(f"start=: the store is on {start.device}, the environment on {self.obs.device}")
        noise = self._begin(steps, seed, noise_std, gamma, noise)
        if start is None:
            v.reset(self.obs)
            self._reset_disc()
            self.start_rows = None
        else:
            self._branch(start)
        self._drive_recorded(steps, min(steps, _CHUNK), noise)
        return self._finish(into, w_new)


class CDTCollector(_Tables, CDTBatchedRollout):
    """``CDTBatchedRollout`` recorded: the same transformer forward on the same window buffers, then ONE launch
    (csrc/cdt_collect.hip ``osrl_cdt_collect``) where the evaluating rollout issues pick, environment, push and cursor.
    Every episode advances by its own step count ``acc[e][2]``; without noise the run is ``CDTBatchedRollout.run``'s bit
    for bit.  ``acc[:, 1]`` and the discounted cost sum carry ``cost_scale`` here (``Collected``'s contract); the window's
    costs-to-go carry it as the evaluating rollout's do, with ``cost_reverse``."""

    def __init__(self, model, venv, cost_scale: float = 1.0, cost_reverse: bool = False, seed: int = 0,
                 use_graph: bool = True):
        super().__init__(model, venv, cost_scale, cost_reverse, use_graph)
        self.seed, self.sample = int(seed), False
        self.env_c = self._desc(model.episode_len)
        self._init_tables()
        e, w = self.eng, L.CdtWindowT()
        w.states, w.actions, w.returns, w.costs_to_go = (e.states.data_ptr(), e.actions.data_ptr(), e.returns.data_ptr(),
                                                         e.ctg.data_ptr())
        w.time_steps, w.mask, w.head = e.time_steps.data_ptr(), e.mask.data_ptr(), e.head.data_ptr()
        w.seq_len, w.head_width, w.sample = model.seq_len, e.head.shape[1], 0
        w.cost_reverse, w.cost_scale = int(self.cost_reverse), self.cost_scale
        self.win = w

    def _desc(self, steps: int):
        return self.venv.desc(steps, self.cost_scale)

    def body(self) -> None:
        v = self.venv
        self.eng.forward(train=False)
        L.check(L.load().osrl_cdt_collect(self.env_c, self._rec_now(), self.win, v.state.data_ptr(), v.acc.data_ptr(), v.E,
                                          cur_stream()), "osrl_cdt_collect")

    @torch.no_grad()
    def run(self, target_return, target_cost, noise_std=0.0, sample: bool = False, gamma: Optional[float] = None,
            seed: Optional[int] = None, noise: Optional[torch.Tensor] = None, into=None) -> Collected:
        """The targets as ``CDTBatchedRollout.run`` takes them; ``noise_std``, ``gamma``, ``seed``, ``noise`` as
        ``Collector.run`` does.  ``sample``: the noise scale is the Gaussian head's own ``exp(log_std)`` at the position
        acted from (a by-value flag of the launch: switching it recaptures, nothing else does).  ``into``: a
        ``SequenceStore`` built with capacities (``check_append`` refuses, before the run, a store that cannot take ``E``
        trajectories of ``episode_len`` rows) or a ``ReplayStore`` under ``Collector.run``'s rules."""
        from ..common.replay import SequenceStore
        v, m = self.venv, self.model
        check_sampling(m, sample, noise_std)
        target_return, target_cost = self._targets(target_return, target_cost)
        steps = self._episode_steps()
        if isinstance(into, SequenceStore):
            into.check_append(v.E, v.E * steps, observations=v.state_dim, actions=m.action_dim)
        else:
            _check_replay_store(into, v.state_dim, m.action_dim)
        if bool(sample) != self.sample:
            self.sample, self.graph = bool(sample), None
            self.win.sample = int(self.sample)
        noise = self._begin(steps, seed, noise_std, gamma, noise)
        m.repack()
        if self.use_graph and noise is None and self.graph is None:
            self._capture()  # runs the body on scratch state; the reset below starts the real run
        self._reset(target_return, target_cost)
        self._reset_disc()
        self._drive_recorded(steps, _CHUNK, noise)
        return self._finish(into)


def check_sampling(model, sample: bool, noise_std) -> None:
    """``sample=True`` needs a Gaussian head and excludes ``noise_std``: ValueError otherwise (host work only)."""
    if not sample:
        return
    if not model.stochastic:
        raise ValueError("sample=True draws from the Gaussian head's own standard deviation: the model was built with "
                         "stochastic=False")
    nz = bool((noise_std != 0).any()) if torch.is_tensor(noise_std) else bool(np.any(np.asarray(noise_std) != 0))
    if nz:
        raise ValueError("sample=True and a non-zero noise_std are two noise scales for one action: pass one of them")


def collect_cdt_batched(trainer, **run_kw) -> Collected:
    """``CDTTrainer.collect_targets`` on a ``VecSyntheticSafeEnv``; the collector is cached on the trainer like
    ``collect_batched``'s."""
    venv = trainer.env
    co = cached(trainer, "_collector", (id(venv), float(trainer.cost_scale), bool(trainer.cost_reverse)),
                lambda: CDTCollector(trainer.model, venv, trainer.cost_scale, trainer.cost_reverse,
                                     use_graph=getattr(trainer, "use_graph", True)))
    return co.run(**run_kw)


def collect_batched(trainer, kind: str, cost_scale: float = 1.0, extra_obs: Optional[float] = None, **run_kw) -> Collected:
    """``Trainer.collect`` on a ``VecSyntheticSafeEnv``; the collector (buffers, tables, captured graph) is cached on the
    trainer like ``evaluate``'s rollout, and reads the model's packed weights in place."""
    venv = trainer.env
    co = cached(trainer, "_collector", (id(venv), kind, float(cost_scale), extra_obs),
                lambda: Collector(trainer.model, venv, kind, cost_scale, extra_obs,
                                  use_graph=getattr(trainer, "use_graph", True)))
    return co.run(**run_kw)
