"""Device-resident transition store + on-device sampler (uniform, or in proportion to per-transition weights).

Replaces the reference's minibatch source -- ``TransitionDataset`` (osrl/common/dataset.py:790-847:
``done = terminals | timeouts`` as fp32 :815-816, ``rewards*reward_scale``, ``costs*cost_scale``,
one uniform-with-replacement index per sample :846) + torch ``DataLoader`` + six ``.to(device)``
copies per step (examples/train/train_cpq.py:122-142) -- with tables that stay in HBM and a gather
kernel (csrc/rng.hip ``osrl_replay_gather``) that draws the indices on device inside the captured
train step.  In the data-parallel setting every rank holds its own shard of the transitions
(``shard(rank, world)``) and samples locally: with random partitions this is distributionally the
same as global uniform sampling.

``sample_prob`` / ``set_sample_prob``: rows are drawn with probability weight / sum instead (with replacement, the same
Philox words as the uniform draw) through a fixed-point cdf table in HBM that the gather kernels search
(include/osrl_amd.h ``osrl_replay_gather_w``, DESIGN.md "Weighted transition sampling").
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .. import _lib as L
from ..engine.core import cur_stream

FIELDS = ("observations", "next_observations", "actions", "rewards", "costs", "done")


class ReplayStore:
    def __init__(self, data: Dict[str, "np.ndarray | torch.Tensor"], device, reward_scale: float = 1.0,
                 cost_scale: float = 1.0, seed: int = 0, rank: int = 0, world: int = 1, state_init: bool = False,
                 sample_prob=None):
        """``data`` uses the DSRL dataset keys (observations, next_observations, actions, rewards, costs,
        and either ``done`` or ``terminals``+``timeouts``).  ``state_init`` (TransitionDataset(state_init=True),
        dataset.py:817-820, used by COptiDICE): a 7th table ``is_init`` = ``done`` shifted by one transition with
        ``is_init[0] = 1``, computed on the FULL dataset before any sharding.  ``sample_prob``: per-transition sampling
        weights of the FULL dataset (``set_sample_prob``); None = uniform."""
        d = dict(data)
        self.state_init = bool(state_init)
        if "done" not in d:
            if torch.is_tensor(d["terminals"]):  # device tables of common.ingest.process_bc_dataset
                d["done"] = torch.logical_or(d["terminals"] == 1, d["timeouts"] == 1)
            else:
                d["done"] = np.logical_or(np.asarray(d["terminals"]) == 1, np.asarray(d["timeouts"]) == 1)
        n = len(d["observations"])
        fields = FIELDS
        if self.state_init:
            dn = d["done"]
            dn = dn.detach().cpu().numpy() if torch.is_tensor(dn) else np.asarray(dn)
            init = np.asarray(dn, np.float32).reshape(-1).copy()
            init[1:] = init[:-1]
            init[0] = 1.0
            d["is_init"] = init
            fields = FIELDS + ("is_init",)
            # TransitionDataset.get_dataset_states (dataset.py:822-830): what COptiDICE's constructor is fed
            as_np = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)  # noqa: E731
            self.init_state_propotion = float(init.mean())
            self.observations_std = as_np(d["observations"]).std(0, keepdims=True)
            self.actions_std = as_np(d["actions"]).std(0, keepdims=True)
        sl = self._shard = slice(rank, n, world) if world > 1 else slice(None)
        self.n_total = n
        self.tables = []
        for k in fields:
            t = torch.as_tensor(np.asarray(d[k])[sl] if not torch.is_tensor(d[k]) else d[k][sl])
            t = t.to(device=device, dtype=torch.float32).reshape(t.shape[0], -1).contiguous()
            self.tables.append(t)
        self.n_rows = self.tables[0].shape[0]
        self.widths = [t.shape[1] for t in self.tables]
        self.scales = [1.0, 1.0, 1.0, float(reward_scale), float(cost_scale), 1.0] + ([1.0] if self.state_init else [])
        self.seed = int(seed) * 1000003 + rank
        self.device = torch.device(device)
        nf = self.n_fields = len(self.tables)
        self._src = (C.c_void_p * nf)(*[t.data_ptr() for t in self.tables])
        self._w = (C.c_int32 * nf)(*self.widths)
        self._s = (C.c_float * nf)(*self.scales)
        self.bytes_per_row = 4 * sum(self.widths)
        # weighted sampling: the table and its scratch are allocated at the first set_sample_prob and then only ever
        # rewritten (captured graphs hold the address); sample_epoch counts the uniform <-> weighted switches, which
        # change the launches' arguments -- the engines compare it before every replay (StepEngine._sync_replay)
        self._cum_buf: Optional[torch.Tensor] = None
        self._cum_ws: Optional[torch.Tensor] = None
        self._w64: Optional[torch.Tensor] = None
        self.weighted = False
        self.sample_epoch = 0
        if sample_prob is not None:
            self.set_sample_prob(sample_prob)

    @property
    def cum(self) -> Optional[torch.Tensor]:
        """The sampler's table -- int64 storage of the uint64 fixed-point cdf, [n_rows] -- or None while uniform."""
        return self._cum_buf if self.weighted else None

    def _cum_ptr(self) -> Optional[int]:
        return self._cum_buf.data_ptr() if self.weighted else None

    def set_sample_prob(self, weights) -> None:
        """Draw row i with probability ``weights[i] / sum`` from now on (with replacement); None: back to uniform.
        ``weights``: one non-negative finite value per transition of the FULL dataset (numpy or tensor, host or device),
        with a positive sum; ValueError otherwise -- for host inputs before any device work.  Data parallel: the weights
        are sliced like the rows (``[rank::world]``) and every rank normalises its own shard, which is global weighted
        sampling only as far as the shards' weight masses are equal (the caveat of uniform sampling from random
        partitions, for masses instead of row counts).
        The table is rewritten in place on the current stream: a captured step draws from the new weights at its next
        replay, nothing is recaptured.  Switching between uniform and weighted changes the launches' arguments instead;
        the engines notice (``sample_epoch``) and rebuild their graphs / descriptors before the next step."""
        if weights is None:
            if self.weighted:
                self.weighted = False
                self.sample_epoch += 1
            return
        if torch.is_tensor(weights) and weights.is_cuda:
            w = weights.reshape(-1)
            if int(w.shape[0]) != self.n_total:
                raise ValueError(f"{self.n_total} transition weights expected, got {int(w.shape[0])}")
            w = w[self._shard].to(device=self.device, dtype=torch.float64).contiguous()
            lo, total = float(w.min()), float(w.sum())  # host reads, once per distribution (NaN fails both tests)
            ok = lo >= 0.0 and 0.0 < total < float("inf")
        else:
            w = weights.detach().cpu().numpy() if torch.is_tensor(weights) else np.asarray(weights)
            w = np.asarray(w, np.float64).reshape(-1)
            if w.shape[0] != self.n_total:
                raise ValueError(f"{self.n_total} transition weights expected, got {w.shape[0]}")
            w = np.ascontiguousarray(w[self._shard])
            total = float(w.sum()) if np.isfinite(w).all() else float("nan")
            ok = bool((w >= 0.0).all()) and 0.0 < total < float("inf")
        if not ok:
            raise ValueError("the weights must be non-negative and finite, with a positive sum"
                             + (" on this rank's shard" if self._shard != slice(None) else ""))
        lib = L.load()
        if self._cum_buf is None:
            self._cum_buf = torch.zeros(self.n_rows, dtype=torch.int64, device=self.device)
            self._cum_ws = torch.zeros(int(lib.osrl_weights_cum_u64_ws_elems(self.n_rows)), dtype=torch.float64,
                                       device=self.device)
            self._w64 = torch.zeros(self.n_rows, dtype=torch.float64, device=self.device)
        self._w64.copy_(w if torch.is_tensor(w) else torch.from_numpy(w))
        L.check(lib.osrl_weights_cum_u64(self._w64.data_ptr(), self.n_rows, self._cum_buf.data_ptr(),
                                         self._cum_ws.data_ptr(), cur_stream()), "osrl_weights_cum_u64")
        if not self.weighted:
            self.weighted = True
            self.sample_epoch += 1

    def get_dataset_states(self):
        """(init_state_propotion, observations_std, actions_std) -- dataset.py:822-830; needs ``state_init``."""
        if not self.state_init:
            raise RuntimeError("build the store with state_init=True")
        return self.init_state_propotion, self.observations_std, self.actions_std

    def gather(self, dst: Sequence[torch.Tensor], st_ptr: Optional[int], idx_out: Optional[torch.Tensor] = None,
               stream_id: int = 1) -> None:
        """dst = (obs, next_obs, act, rew, cost, done[, is_init]) batch buffers; asynchronous on the current stream."""
        B = dst[0].shape[0]
        if len(dst) != self.n_fields:
            raise ValueError(f"the store holds {self.n_fields} tables, {len(dst)} destination buffers were given")
        d = (C.c_void_p * self.n_fields)(*[t.data_ptr() for t in dst])
        L.check(L.load().osrl_replay_gather_w(self.n_fields, self._src, d, self._w, self._s, self.n_rows, B,
                                              None if idx_out is None else idx_out.data_ptr(), self.seed, stream_id,
                                              st_ptr, self._cum_ptr(), cur_stream()), "osrl_replay_gather")

    def gather_args(self, dst: Sequence[torch.Tensor], fields: Optional[Sequence[int]] = None, stream_id: int = 1):
        """The arguments of ``gather`` / ``gather_fields`` as the tuple ``StepState.begin(gather=...)`` takes (the
        fused step prologue draws the same rows: the indices are a function of (seed, step, row) and the weight table
        only); the last element is the table's address, None while uniform."""
        if fields is None:
            fields = range(self.n_fields)
        fields = list(fields)
        if len(dst) != len(fields):
            raise ValueError(f"{len(fields)} tables selected, {len(dst)} destination buffers were given")
        n = len(fields)
        src = (C.c_void_p * n)(*[self.tables[i].data_ptr() for i in fields])
        d = (C.c_void_p * n)(*[t.data_ptr() for t in dst])
        w = (C.c_int32 * n)(*[self.widths[i] for i in fields])
        sc = (C.c_float * n)(*[self.scales[i] for i in fields])
        return (n, src, d, w, sc, self.n_rows, dst[0].shape[0], self.seed, stream_id, list(dst), self._cum_ptr())

    def gather_fields(self, fields: Sequence[int], dst: Sequence[torch.Tensor], st_ptr: Optional[int],
                      stream_id: int = 1) -> None:
        """The same draw as ``gather`` (the row indices are a function of (seed, step, row) only) restricted to some
        of the tables -- (0, 2) = observations, actions is all BC reads (train_bc.py:121)."""
        n, B = len(fields), dst[0].shape[0]
        src = (C.c_void_p * n)(*[self.tables[i].data_ptr() for i in fields])
        d = (C.c_void_p * n)(*[t.data_ptr() for t in dst])
        w = (C.c_int32 * n)(*[self.widths[i] for i in fields])
        sc = (C.c_float * n)(*[self.scales[i] for i in fields])
        L.check(L.load().osrl_replay_gather_w(n, src, d, w, sc, self.n_rows, B, None, self.seed, stream_id, st_ptr,
                                              self._cum_ptr(), cur_stream()), "osrl_replay_gather")

def synthetic_transitions(n: int, od: int, ad: int, seed: int = 1, max_action: float = 1.0) -> Dict[str, np.ndarray]:
    """Synthetic DSRL-shaped data: obs~N(0,1), act~U(-1,1), rew~N(0,1), cost~Bern(.1),
    terminals~Bern(.01)."""
    rs = np.random.RandomState(seed)
    f = np.float32
    return dict(observations=rs.randn(n, od).astype(f), next_observations=rs.randn(n, od).astype(f),
                actions=(rs.uniform(-1, 1, (n, ad)) * max_action).astype(f), rewards=rs.randn(n).astype(f),
                costs=(rs.uniform(size=n) < 0.1).astype(f), terminals=(rs.uniform(size=n) < 0.01).astype(f),
                timeouts=np.zeros(n, f))


class SequenceStore:
    """Device-resident trajectory store + on-device window sampler for CDT: replaces ``SequenceDataset``
    (osrl/common/dataset.py:633-787; ``from_dataset`` covers its augmentation paths) + DataLoader.
    ``trajectories``: list of dicts with observations [L,od], actions [L,ad], returns [L] (return-to-go),
    cost_returns [L] (cost-to-go), costs [L].  ``sample_prob``: optional per-trajectory probabilities
    (dataset.py:439-459 ``compute_cost_sample_prob`` output); None = uniform."""

    def __init__(self, trajectories, seq_len: int, device, reward_scale: float = 1.0, cost_scale: float = 1.0,
                 sample_prob=None, seed: int = 0, rank: int = 0, start_sampling: bool = False, prob: float = 0.4):
        self.T, self.device = int(seq_len), torch.device(device)
        cat = lambda k: torch.as_tensor(np.concatenate([np.asarray(t[k], np.float32).reshape(len(t["costs"]), -1)  # noqa: E731
                                                        for t in trajectories]), device=self.device).contiguous()
        self.obs, self.act = cat("observations"), cat("actions")
        self.ret, self.cret, self.cost = cat("returns").view(-1), cat("cost_returns").view(-1), cat("costs").view(-1)
        lens = np.array([len(t["costs"]) for t in trajectories], np.int64)
        self.traj_len = torch.as_tensor(lens.astype(np.int32), device=self.device)
        self.traj_start = torch.as_tensor(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), device=self.device)
        self.n_traj = len(trajectories)
        self.cdf = None
        if sample_prob is not None:
            c = np.cumsum(np.asarray(sample_prob, np.float64))
            c /= c[-1]
            self.cdf = torch.as_tensor(c.astype(np.float32), device=self.device)
        self.reward_scale, self.cost_scale = float(reward_scale), float(cost_scale)
        self.base_seed = int(seed)
        self.set_rank(rank)
        self.od, self.ad = self.obs.shape[1], self.act.shape[1]
        self.start_cdf = None
        if start_sampling:
            self.enable_start_sampling(prob)

    def enable_start_sampling(self, prob: float = 0.4) -> None:
        """``SequenceDataset(start_sampling=True, prob=...)`` (dataset.py:742-744,781-783): window starts are drawn
        from ``compute_start_index_sample_prob`` instead of uniformly (computed on device, csrc/ingest.hip)."""
        from .ingest import compute_start_index_sample_prob
        tables = dict(costs=self.cost, traj_start=self.traj_start, traj_len=self.traj_len)
        self.start_cdf = compute_start_index_sample_prob(tables, prob, with_cdf=True)[1]

    def set_sample_prob(self, weights) -> None:
        """Sample trajectories in proportion to ``weights``: any non-negative per-trajectory values (numpy or
        tensor, host or device), normalised and turned into the cdf the sampler reads on device.  Replaces any
        earlier trajectory distribution (``sample_prob``, ``cost_sample``, ``enable_pf_sampling``)."""
        from .ingest import sample_prob_from_weights
        w = weights if torch.is_tensor(weights) else torch.as_tensor(np.asarray(weights, np.float64))
        w = w.reshape(-1)
        if int(w.shape[0]) != self.n_traj:
            raise ValueError(f"{self.n_traj} trajectory weights expected, got {int(w.shape[0])}")
        w = w.to(device=self.device, dtype=torch.float64)
        lo, total = float(w.min()), float(w.sum())  # host reads, once per distribution
        if not (lo >= 0.0 and 0.0 < total < float("inf")):
            raise ValueError("the weights must be non-negative and finite, with a positive sum")
        self.cdf = sample_prob_from_weights(w, with_cdf=True)[1]

    def enable_pf_sampling(self, beta: float = 1.0, frontier=None) -> None:
        """``SequenceDataset(pf_sample=True)`` (dataset.py:736-737): trajectories are drawn with probability
        ~ ``1 / (distance to the Pareto frontier + beta)`` (``common.ingest.compute_sample_prob``, csrc/pf_dist.h),
        over the original and the augmented trajectories.  ``frontier``: an ``ingest.Frontier`` (e.g. from
        ``ingest.pareto_frontier``) for a store built without augmentation; by default the one the augmentation
        fitted (``aug_info["frontier"]``), else AttributeError as ``compute_pareto_return``.  Replaces any other
        trajectory distribution.  Two things the reference's constructor does differently: there ``cost_sample``
        wins when both flags are set (pf_sample is then ignored), and beta is hard-wired to 1 (:737) whatever
        the ``beta`` argument -- which only feeds the augmentation's partner draws -- says."""
        from .ingest import compute_sample_prob
        if frontier is None:
            info = getattr(self, "aug_info", None)
            frontier = None if info is None else info["frontier"]
        if frontier is None:
            raise AttributeError("no Pareto frontier: the store was built without augment_percent (pass frontier=)")
        tables = dict(returns=self.ret, cost_returns=self.cret, traj_start=self.traj_start)
        self.cdf = compute_sample_prob(tables, frontier, beta, with_cdf=True)[1]

    def set_rank(self, rank: int) -> None:
        """Data parallel: every rank draws its own windows (same mixing as ReplayStore); the CDT engine calls this
        from ``attach_store`` when it runs under a DataParallel hook."""
        self.rank = int(rank)
        self.seed = self.base_seed * 1000003 + self.rank if self.rank else self.base_seed

    @classmethod
    def from_tables(cls, tables: Dict[str, torch.Tensor], seq_len: int, reward_scale: float = 1.0,
                    cost_scale: float = 1.0, cdf: Optional[torch.Tensor] = None, seed: int = 0,
                    rank: int = 0, start_sampling: bool = False, prob: float = 0.4) -> "SequenceStore":
        """Wrap the flat device tables of ``common.ingest.process_sequence_dataset`` (nothing is copied)."""
        self = cls.__new__(cls)
        self.T, self.device = int(seq_len), tables["observations"].device
        self.obs, self.act = tables["observations"].contiguous(), tables["actions"].contiguous()
        self.ret, self.cret, self.cost = tables["returns"], tables["cost_returns"], tables["costs"]
        self.traj_start, self.traj_len = tables["traj_start"], tables["traj_len"]
        self.n_traj = int(self.traj_start.shape[0])
        self.cdf = cdf
        self.reward_scale, self.cost_scale = float(reward_scale), float(cost_scale)
        self.base_seed = int(seed)
        self.set_rank(rank)
        self.od, self.ad = self.obs.shape[1], self.act.shape[1]
        self.start_cdf = None
        if start_sampling:
            self.enable_start_sampling(prob)
        return self

    @classmethod
    def from_dataset(cls, dataset, seq_len: int, device, reward_scale: float = 1.0, cost_scale: float = 1.0,
                     cost_reverse: bool = False, cost_sample: bool = False,
                     cost_transform=("affine", -1.0, 50.0), seed: int = 0, rank: int = 0,
                     start_sampling: bool = False, prob: float = 0.4, deg: int = 3, pf_sample: bool = False,
                     max_rew_decrease: float = 1.0, beta: float = 1.0, augment_percent: float = 0,
                     max_reward: float = 1000.0, min_reward: float = 5, pf_only: bool = False, rmin: float = 0,
                     cost_bins: int = 60, npb: int = 5, random_aug: float = 0, aug_rmin: float = 0,
                     aug_rmax: float = 600, aug_cmin: float = 5, aug_cmax: float = 50, cgap: float = 5,
                     rstd: float = 1, cstd: float = 0.2, draws: Optional[dict] = None) -> "SequenceStore":
        """``SequenceDataset(dataset, seq_len, reward_scale, cost_scale, ...)`` (dataset.py:633-747) with the whole
        preprocessing on device.  The constructor's branches run in the reference's order: ``pf_only`` (which only
        suppresses the augmentations: the reference discards select_optimal_trajectory's result), else
        ``random_aug > 0`` (``common.ingest.random_augmentation``), else ``augment_percent > 0``
        (``common.ingest.augmentation``); cost / start sampling then act on the original + augmented trajectories.
        The random draws are keyed by ``seed`` (never the rank), so every data-parallel rank builds the same tables;
        ``draws`` injects them instead (tests).  ``rmin``, ``cost_bins``, ``npb`` only feed the reference's discarded
        ``pf_only`` selection and are accepted for signature parity.  ``cost_transform`` is one of the two tuple forms
        of ``common.ingest.compute_cost_sample_prob`` (all on device) or a python callable as in the reference
        (applied on the host to the per-trajectory cost returns).  ``pf_sample=True`` raises: the frontier-distance
        distribution is installed afterwards with ``enable_pf_sampling()`` (in the reference ``cost_sample`` wins
        over ``pf_sample``, and its beta is hard-wired to 1, dataset.py:734-737)."""
        from .ingest import augmentation, compute_cost_sample_prob, process_sequence_dataset, random_augmentation
        if pf_sample:
            raise NotImplementedError("pf_sample=True is not built by from_dataset: build the store without it and "
                                      "call enable_pf_sampling() (compute_sample_prob, dataset.py:399-436, on device)")
        tables = process_sequence_dataset(dataset, cost_reverse, device)
        n_orig = int(tables["traj_start"].shape[0])
        info = None
        if pf_only:
            pass
        elif random_aug > 0:
            tables, info = random_augmentation(tables, random_aug, aug_rmin, aug_rmax, aug_cmin, aug_cmax, cgap, rstd,
                                               cstd, seed=seed, draws=draws)
        elif augment_percent > 0:
            tables, info = augmentation(tables, deg, max_rew_decrease, beta, augment_percent, max_reward, min_reward,
                                        seed=seed, draws=draws)
        cdf = compute_cost_sample_prob(tables, cost_transform, with_cdf=True)[1] if cost_sample else None
        self = cls.from_tables(tables, seq_len, reward_scale, cost_scale, cdf, seed, rank, start_sampling, prob)
        self.n_original = n_orig
        self.n_augmented = 0 if info is None else int(info["n_augmented"])
        self.aug_info = info
        return self

    # what SequenceDataset keeps after augmentation (dataset.py:718-738); read back from the device on access
    @property
    def idx(self):
        info = getattr(self, "aug_info", None)
        return None if info is None else info["idx"].cpu().numpy().astype(np.int64)

    @property
    def indices(self):
        info = getattr(self, "aug_info", None)
        return None if info is None or info["indices"] is None else info["indices"].cpu().numpy().astype(np.int64)

    @property
    def pareto_frontier(self):
        info = getattr(self, "aug_info", None)
        return None if info is None or info["frontier"] is None else info["frontier"].poly

    def compute_pareto_return(self, cost):
        """SequenceDataset.compute_pareto_return (dataset.py:746-747)."""
        pf = self.pareto_frontier
        if pf is None:
            raise AttributeError("no Pareto frontier: the store was built without augment_percent")
        return pf(cost)

    def gather(self, states, actions, returns, cost_returns, time_steps, mask, episode_cost, costs, st_ptr,
               idx_out=None, stream_id: int = 2, idx_in=None) -> None:
        """``idx_in``: optional int32 [B,2] device tensor of (trajectory, start) pairs to use instead of drawing."""
        B = states.shape[0]
        L.check(L.load().osrl_seq_window_gather(
            self.obs.data_ptr(), self.act.data_ptr(), self.ret.data_ptr(), self.cret.data_ptr(), self.cost.data_ptr(),
            self.traj_start.data_ptr(), self.traj_len.data_ptr(), None if self.cdf is None else self.cdf.data_ptr(),
            None if self.start_cdf is None else self.start_cdf.data_ptr(),
            None if idx_in is None else idx_in.data_ptr(), self.n_traj, B, self.T, self.od, self.ad, self.reward_scale, self.cost_scale, states.data_ptr(),
            actions.data_ptr(), returns.data_ptr(), cost_returns.data_ptr(), time_steps.data_ptr(), mask.data_ptr(),
            episode_cost.data_ptr(), costs.data_ptr(), None if idx_out is None else idx_out.data_ptr(), self.seed,
            stream_id, st_ptr, cur_stream()), "osrl_seq_window_gather")
