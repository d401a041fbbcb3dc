"""Device-resident transition store + on-device sampler (uniform, or in proportion to per-transition weights).

Replaces the reference's minibatch source -- ``TransitionDataset`` (osrl/common/dataset.py:790-847:
``done = terminals | timeouts`` as fp32 :815-816, ``rewards*reward_scale``, ``costs*cost_scale``,
one uniform-with-replacement index per sample :846) + torch ``DataLoader`` + six ``.to(device)``
copies per step (examples/train/train_cpq.py:122-142) -- with tables that stay in HBM and a gather
kernel (csrc/rng.hip ``osrl_replay_gather``) that draws the indices on device inside the captured
train step.  In the data-parallel setting every rank holds its own shard of the transitions
(``shard(rank, world)``) and samples locally: with random partitions this is distributionally the
same as global uniform sampling.

``capacity`` / ``append``: a store that grows in place.  The tables are allocated once for ``capacity`` rows and the live
row count sits in one device word that the sampling kernels read (include/osrl_amd.h ``osrl_replay_gather_n``), so a
captured train step follows ``append`` at its next replay -- nothing is re-uploaded, nothing is recaptured
(DESIGN.md "Stores that grow").

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


def ring_spans(cursor: int, m: int, capacity: int):
    """Where ``m`` new rows land in a ring of ``capacity`` rows whose next free slot is ``cursor``: row ``i`` of the chunk
    goes to ``(cursor + i) % capacity``, later rows winning where a chunk longer than the ring laps itself.  Returns at
    most two ``(dst, src, length)`` triples of contiguous copies ``ring[dst:dst + length] = chunk[src:src + length]``."""
    cursor, m, capacity = int(cursor), int(m), int(capacity)
    if capacity < 1 or not 0 <= cursor < capacity or m < 0:
        raise ValueError(f"ring_spans({cursor}, {m}, {capacity})")
    src = max(m - capacity, 0)  # (rows before this are overwritten by the chunk's own later rows)
    n = m - src
    if n == 0:
        return []
    dst = (cursor + src) % capacity
    first = min(n, capacity - dst)
    return [(dst, src, first)] + ([(0, src + first, n - first)] if n > first else [])


def ring_spans_pinned(cursor: int, m: int, capacity: int, pinned: int):
    """``ring_spans`` for a store whose first ``pinned`` rows are never overwritten: the ring runs over
    ``[pinned, capacity)``, so row ``i`` of the chunk goes to ``pinned + (cursor - pinned + i) % (capacity - pinned)``.
    ``pinned <= cursor < capacity``; the same ``(dst, src, length)`` triples, and ``pinned = 0`` is ``ring_spans``."""
    cursor, m, capacity, pinned = int(cursor), int(m), int(capacity), int(pinned)
    if not 0 <= pinned < capacity or not pinned <= cursor < capacity:
        raise ValueError(f"ring_spans_pinned({cursor}, {m}, {capacity}, {pinned})")
    return [(dst + pinned, src, n) for dst, src, n in ring_spans(cursor - pinned, m, capacity - pinned)]


def seq_ring_plan(starts, lens, tail: int, mr: int, mt: int, capacity_rows: int, capacity_traj: int):
    """Where a chunk of ``mt`` whole trajectories in ``mr`` rows lands in a ``SequenceStore(evict="oldest")`` whose live
    trajectories, oldest first, occupy rows ``[starts[i], starts[i] + lens[i])`` and whose newest one ends at ``tail``:
    ``(p, n_evict, new_tail)``.  ValueError when the chunk can never fit (``mr > capacity_rows`` or
    ``mt > capacity_traj``).  The chunk stays contiguous: ``p = tail`` while it fits behind the newest trajectory, else
    ``p = 0`` (the rows from ``tail`` to the end stay unused for this lap); then the oldest trajectories go, one at a
    time, while there are too many slots in use or any live trajectory still touches ``[p, p + mr)``."""
    tail, mr, mt, cr, ct = int(tail), int(mr), int(mt), int(capacity_rows), int(capacity_traj)
    if mr > cr or mt > ct:
        raise ValueError(f"the chunk ({mr} rows, {mt} trajectories) is larger than the store ({cr} rows, {ct} "
                         "trajectories)")
    s, n = np.asarray(starts, np.int64).reshape(-1), np.asarray(lens, np.int64).reshape(-1)
    p = tail if tail + mr <= cr else 0
    hit = np.nonzero((s < p + mr) & (s + n > p))[0]  # evicting oldest first: everything up to the last one that touches
    k = max(0, s.shape[0] + mt - ct, int(hit[-1]) + 1 if hit.shape[0] else 0)
    return p, k, p + mr


def _done_of(d):
    if "done" in d:
        return d["done"]
    if torch.is_tensor(d["terminals"]):  # device tables of common.ingest.process_bc_dataset
        return torch.logical_or(d["terminals"] == 1, d["timeouts"] == 1)
    return np.logical_or(np.asarray(d["terminals"]) == 1, np.asarray(d["timeouts"]) == 1)


def _shift_done(dn) -> np.ndarray:
    """``is_init`` of a run of transitions that starts at an episode start: ``done`` shifted by one, 1 on the first row."""
    dn = dn.detach().cpu().numpy() if torch.is_tensor(dn) else np.asarray(dn)
    init = np.asarray(dn, np.float32).reshape(-1).copy()
    init[1:] = init[:-1]
    if init.shape[0]:
        init[0] = 1.0
    return init


def _checked_weights(weights, n: int, what: str, shard: slice = slice(None), positive_sum: bool = True) -> torch.Tensor:
    """``weights`` (numpy or tensor, host or device) as a flat fp64 tensor ON THE DEVICE IT CAME FROM -- a host input is
    judged on the host, before any device work -- cut to ``shard``.  ValueError unless there are ``n`` of them, one per
    ``what``, non-negative and finite, and (``positive_sum``) with a positive finite sum over the shard."""
    w = weights.detach() if torch.is_tensor(weights) else torch.from_numpy(
        np.ascontiguousarray(np.asarray(weights, np.float64)))
    w = w.reshape(-1)
    if int(w.shape[0]) != n:
        raise ValueError(f"{n} {what} weights expected, got {int(w.shape[0])}")
    w = w[shard].to(torch.float64).contiguous()
    ok = True
    if w.shape[0] > 0:  # host reads, once per distribution (a NaN fails the first test, an infinity the second)
        ok = float(w.min()) >= 0.0 and float(w.max()) < float("inf")
    if not positive_sum:
        if not ok:
            raise ValueError("the weights must be non-negative and finite")
        return w
    if not (ok and w.shape[0] > 0 and 0.0 < float(w.sum()) < float("inf")):
        raise ValueError("the weights must be non-negative and finite, with a positive sum"
                         + (" on this rank's shard" if shard != slice(None) else ""))
    return w


class ReplayStore:
    def __init__(self, data: Dict[str, "np.ndarray | torch.Tensor"], device, reward_scale: float = 1.0,
                 cost_scale: float = 1.0, seed: int = 0, rank: int = 0, world: int = 1, state_init: bool = False,
                 capacity: Optional[int] = None, pinned_rows: int = 0, sample_prob=None):
        """``data`` uses the DSRL dataset keys (observations, next_observations, actions, rewards, costs,
        and either ``done`` or ``terminals``+``timeouts``).  ``state_init`` (TransitionDataset(state_init=True),
        dataset.py:817-820, used by COptiDICE): a 7th table ``is_init`` = ``done`` shifted by one transition with
        ``is_init[0] = 1``, computed on the FULL dataset before any sharding.  ``sample_prob``: per-transition sampling
        weights of the FULL dataset (``set_sample_prob``); None = uniform.
        ``capacity`` (None: a fixed store, exactly as before): allocate the tables for that many rows (>= ``len(data)``,
        zero past the data) so that ``append`` can add transitions in place; single rank only (ValueError with
        ``world > 1``).  ``n_rows`` is then the LIVE row count, ``capacity`` the allocation; the launches carry the
        capacity and the address of the device word that holds the live count.  With ``state_init``,
        ``init_state_propotion`` and the two ``*_std`` are those of the construction-time data and are not updated by
        ``append``.
        ``pinned_rows`` p (only with ``capacity``; ``p <= len(data)``, ``p < capacity``, ValueError otherwise): the first
        p rows are never overwritten -- ``append``'s ring runs over ``[p, capacity)`` (``ring_spans_pinned``), so logged
        data stays while generated rows behind it turn over.  0, the default: the store as it always was."""
        d = dict(data)
        self.state_init = bool(state_init)
        d["done"] = _done_of(d)
        n = len(d["observations"])
        pinned_rows = int(pinned_rows)
        if pinned_rows:
            if capacity is None:
                raise ValueError("pinned_rows= needs a store built with capacity=")
            if not 0 < pinned_rows <= n or pinned_rows >= int(capacity):
                raise ValueError(f"pinned_rows {pinned_rows} must lie in [0, {n}] (the rows of the data) and below the "
                                 f"capacity {int(capacity)}")
        self.pinned_rows = pinned_rows
        if capacity is not None:
            capacity = int(capacity)
            if world > 1:
                raise ValueError("capacity= with world > 1: a sharded store does not grow (build one store per rank)")
            if capacity < max(n, 1):
                raise ValueError(f"capacity {capacity} is below the {n} rows of the data")
        fields = FIELDS
        if self.state_init:
            init = _shift_done(d["done"])
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
            if capacity is not None:  # one allocation for the store's life: captured graphs hold these addresses
                full = torch.zeros(capacity, t.shape[1], dtype=torch.float32, device=device)
                full[:n].copy_(t)
                t = full
            self.tables.append(t)
        self.n_rows = n if capacity is not None else self.tables[0].shape[0]
        self.capacity = capacity
        self.version = 0  # incremented by every append (caches keyed on the store's contents compare it)
        self._cursor = 0 if capacity is None else n % capacity  # the ring's next slot
        if pinned_rows and self._cursor < pinned_rows:  # (a full store: the ring wraps to its own first row)
            self._cursor = pinned_rows
        self._live = None if capacity is None else torch.full((1,), n, dtype=torch.int64, device=device)
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
        """The sampler's table -- int64 storage of the uint64 fixed-point cdf, [n_rows] ([capacity] on a store that
        grows, valid over the live rows) -- or None while uniform."""
        return self._cum_buf if self.weighted else None

    @property
    def _alloc_rows(self) -> int:
        """The row count the launches carry: the allocation (the draw itself runs over the live word, if there is one)."""
        return self.n_rows if self.capacity is None else self.capacity

    def _live_ptr(self) -> Optional[int]:
        return None if self._live is None else self._live.data_ptr()

    def live(self, i: int) -> torch.Tensor:
        """Table ``i`` sliced to the live rows (the whole table on a fixed store)."""
        return self.tables[i][:self.n_rows]

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
        the engines notice (``sample_epoch``) and rebuild their graphs / descriptors before the next step.
        A store built with ``capacity``: one weight per LIVE row, in physical (table) order."""
        if weights is None:
            if self.weighted:
                self.weighted = False
                self.sample_epoch += 1
            return
        w = _checked_weights(weights, self.n_total, "transition", self._shard)
        self._alloc_weights()
        self._w64[:self.n_rows].copy_(w)
        self._build_cum()
        if not self.weighted:
            self.weighted = True
            self.sample_epoch += 1

    def _alloc_weights(self) -> None:
        if self._cum_buf is None:
            cap = self._alloc_rows
            self._cum_buf = torch.zeros(cap, dtype=torch.int64, device=self.device)
            self._cum_ws = torch.zeros(int(L.load().osrl_weights_cum_u64_ws_elems(cap)), dtype=torch.float64,
                                       device=self.device)
            self._w64 = torch.zeros(cap, dtype=torch.float64, device=self.device)

    def _build_cum(self) -> None:
        """The table over the live rows, in place (one osrl_weights_cum_u64 call on the current stream)."""
        L.check(L.load().osrl_weights_cum_u64(self._w64.data_ptr(), self.n_rows, self._cum_buf.data_ptr(),
                                              self._cum_ws.data_ptr(), cur_stream()), "osrl_weights_cum_u64")

    # ---- growth -------------------------------------------------------------------------------------------------------
    def check_append_widths(self, **widths: int) -> None:
        """ValueError unless a chunk with these column counts (``observations=17, actions=6, ...``) fits the tables."""
        names = FIELDS + ("is_init",)
        for k, w in widths.items():
            i = names.index(k)
            if i < self.n_fields and int(w) != self.widths[i]:
                raise ValueError(f"the store's {k} have {self.widths[i]} columns, the new rows {int(w)}")

    def append(self, data: Dict[str, "np.ndarray | torch.Tensor"], sample_prob=None) -> None:
        """Add the transitions of ``data`` (the DSRL keys, as the constructor takes them: numpy or tensors, host or
        device) to a store built with ``capacity``.  Values are stored raw (the scales stay in the gather).  Row ``i`` of
        the chunk lands at ``(cursor + i) % capacity``: a full store overwrites its oldest rows, the live count
        saturates at the capacity (with ``pinned_rows`` the ring is ``[pinned_rows, capacity)``: the rows before it stay).
        At most two contiguous copies per table (``ring_spans``) and one write of the live
        word, all on the current stream: a captured step that draws from this store sees the new rows at its next
        replay, and nothing is recaptured.  ``version`` is incremented.
        ``state_init`` stores: the chunk's ``is_init`` is its ``done`` shifted by one row with 1 on its first row, so a
        chunk must START at an episode start (a chunk that continues the previous one's last episode would mark a
        spurious initial state); ``init_state_propotion`` / ``observations_std`` / ``actions_std`` stay as constructed.
        Weighted stores need ``sample_prob``: the new rows' weights (they join the others in physical row order and the
        table is rebuilt over the live rows); ValueError without it, and on a uniform store with it.  Widths and keys
        are checked before any device work (ValueError)."""
        if self.capacity is None:
            raise ValueError("this store is fixed: build it with capacity= to append")
        d = dict(data)
        missing = [k for k in FIELDS[:5] if k not in d] + \
            ([] if "done" in d or ("terminals" in d and "timeouts" in d) else ["done (or terminals + timeouts)"])
        if missing:
            raise ValueError(f"append: missing {', '.join(missing)}")
        shape = lambda x: tuple(x.shape) if torch.is_tensor(x) else np.shape(x)  # noqa: E731
        m = int(shape(d["observations"])[0])
        lead = ("done",) if "done" in d else ("terminals", "timeouts")
        for k in FIELDS[:5] + lead:
            sh = shape(d[k])
            if len(sh) < 1 or int(sh[0]) != m:
                raise ValueError(f"append: {k} holds {sh[0] if sh else 0} rows, observations {m}")
            w = int(np.prod(sh[1:], dtype=np.int64))
            want = self.widths[FIELDS.index(k)] if k in FIELDS else 1
            if w != want:
                raise ValueError(f"the store's {k} have {want} columns, the new rows {w}")
        if self.weighted and sample_prob is None:
            raise ValueError("the store draws by weight: append(data, sample_prob=) needs the new rows' weights")
        if not self.weighted and sample_prob is not None:
            raise ValueError("the store draws uniformly: call set_sample_prob() over the live rows instead")
        w_new = None if sample_prob is None else _checked_weights(sample_prob, m, "transition", positive_sum=False)
        if m == 0:
            return
        d["done"] = _done_of(d)
        if self.state_init:
            d["is_init"] = _shift_done(d["done"])
        p = self.pinned_rows
        spans = ring_spans_pinned(self._cursor, m, self.capacity, p) if p else ring_spans(self._cursor, m, self.capacity)
        names = FIELDS + (("is_init",) if self.state_init else ())
        for k, table in zip(names, self.tables):
            x = d[k] if torch.is_tensor(d[k]) else torch.from_numpy(np.ascontiguousarray(np.asarray(d[k])))
            x = x.reshape(m, -1)
            for dst, src, n in spans:
                table[dst:dst + n].copy_(x[src:src + n], non_blocking=True)  # (casts to fp32, host or device source)
        if w_new is not None:
            for dst, src, n in spans:
                self._w64[dst:dst + n].copy_(w_new[src:src + n], non_blocking=True)
        self._cursor = p + (self._cursor - p + m) % (self.capacity - p)
        self.n_rows = self.n_total = min(self.n_rows + m, self.capacity)
        self._live.fill_(self.n_rows)
        self.version += 1
        if w_new is not None:
            self._build_cum()

    # ---- checkpointing (common.checkpoint.save_store / load_store) ------------------------------------------------------
    def state_dict(self) -> dict:
        """The contents of a store built with ``capacity``, as host tensors, numbers and strings: the tables over the
        live rows IN PHYSICAL ORDER (the ring as it lies, not unrolled), the ring's cursor, the raw sampling weights
        and, with ``state_init``, the construction-time statistics.  Seeds and ranks belong to the constructor.
        ValueError on a fixed store: that one is rebuilt from its dataset."""
        if self.capacity is None:
            raise ValueError("this store is fixed: it is rebuilt from its dataset, only a store built with capacity= "
                             "is saved")
        n = self.n_rows
        sd = dict(kind="ReplayStore", format=1, capacity=self.capacity, widths=list(self.widths),
                  scales=[float(x) for x in self.scales], state_init=self.state_init, n_rows=n, cursor=self._cursor,
                  weighted=bool(self.weighted), tables=[t[:n].detach().cpu().clone() for t in self.tables],
                  w64=self._w64[:n].detach().cpu().clone() if self.weighted else None)
        if self.pinned_rows:  # (only when set: the dictionary of a store without pinned rows is what it always was)
            sd["pinned_rows"] = self.pinned_rows
        if self.state_init:
            sd["init_state_propotion"] = float(self.init_state_propotion)
            sd["observations_std"] = torch.from_numpy(np.array(self.observations_std))
            sd["actions_std"] = torch.from_numpy(np.array(self.actions_std))
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Make this store the saved one, in the allocations it has: same tables, cursor, live count and weights, so it
        draws the same minibatches and every later ``append`` lands the same.  The store must have been built with the
        saved capacity, widths, ``state_init`` and scales (ValueError naming the difference, before any device work).
        Everything is written in place on the current stream -- an attached engine follows at its next replay;
        ``version`` is incremented, and ``sample_epoch`` when the load switches between uniform and weighted."""
        if self.capacity is None:
            raise ValueError("this store is fixed: build it with capacity= to load a saved store into it")
        if sd.get("kind") != "ReplayStore" or sd.get("format") != 1:
            raise ValueError(f"not a saved ReplayStore (kind {sd.get('kind')!r}, format {sd.get('format')!r})")
        for what, mine, theirs in (("capacity", self.capacity, sd["capacity"]),
                                   ("state_init", self.state_init, sd["state_init"]),
                                   ("pinned_rows", self.pinned_rows, int(sd.get("pinned_rows", 0))),
                                   ("widths", list(self.widths), list(sd["widths"])),
                                   ("scales", [float(x) for x in self.scales], [float(x) for x in sd["scales"]])):
            if mine != theirs:
                raise ValueError(f"the saved store's {what} is {theirs}, this store's {mine}")
        n = int(sd["n_rows"])
        for t, src in zip(self.tables, sd["tables"]):
            t[:n].copy_(src, non_blocking=True)
            t[n:].zero_()
        if sd["weighted"]:
            self._alloc_weights()
            self._w64[:n].copy_(sd["w64"], non_blocking=True)
            self._w64[n:].zero_()
        self.n_rows = self.n_total = n
        self._cursor = int(sd["cursor"])
        self._live.fill_(n)
        if self.state_init:
            self.init_state_propotion = float(sd["init_state_propotion"])
            self.observations_std = sd["observations_std"].numpy().copy()
            self.actions_std = sd["actions_std"].numpy().copy()
        self.version += 1
        if sd["weighted"]:
            self._build_cum()
        if self.weighted != bool(sd["weighted"]):
            self.weighted = bool(sd["weighted"])
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
        self._gather(self.n_fields, self._src, d, self._w, self._s, B, None if idx_out is None else idx_out.data_ptr(),
                     stream_id, st_ptr)

    def _gather(self, n, src, d, w, sc, B, idx_ptr, stream_id, st_ptr) -> None:
        lib = L.load()
        if self._live is None:  # a fixed store: the entry point and the arguments it always had
            rc = lib.osrl_replay_gather_w(n, src, d, w, sc, self.n_rows, B, idx_ptr, self.seed, stream_id, st_ptr,
                                          self._cum_ptr(), cur_stream())
        else:
            rc = lib.osrl_replay_gather_n(n, src, d, w, sc, self.capacity, B, idx_ptr, self.seed, stream_id, st_ptr,
                                          self._cum_ptr(), self._live.data_ptr(), cur_stream())
        L.check(rc, "osrl_replay_gather")

    def gather_args(self, dst: Sequence[torch.Tensor], fields: Optional[Sequence[int]] = None, stream_id: int = 1):
        """The arguments of ``gather`` / ``gather_fields`` as the tuple ``StepState.begin(gather=...)`` takes (the
        fused step prologue draws the same rows: the indices are a function of (seed, step, row) and the weight table
        only); the last two elements are the weight table's address, None while uniform, and the live-count word's, None
        on a fixed store (the row count is then the store's capacity)."""
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
        return (n, src, d, w, sc, self._alloc_rows, dst[0].shape[0], self.seed, stream_id, list(dst), self._cum_ptr(),
                self._live_ptr())

    def gather_fields(self, fields: Sequence[int], dst: Sequence[torch.Tensor], st_ptr: Optional[int],
                      stream_id: int = 1, idx_out: Optional[torch.Tensor] = None) -> None:
        """The same draw as ``gather`` (the row indices are a function of (seed, step, row) only) restricted to some
        of the tables -- (0, 2) = observations, actions is all BC reads (train_bc.py:121).  ``idx_out`` (int32 ``[B]``
        on the device, optional) receives the drawn row indices, as ``gather``'s does."""
        n, B = len(fields), dst[0].shape[0]
        src = (C.c_void_p * n)(*[self.tables[i].data_ptr() for i in fields])
        d = (C.c_void_p * n)(*[t.data_ptr() for t in dst])
        w = (C.c_int32 * n)(*[self.widths[i] for i in fields])
        sc = (C.c_float * n)(*[self.scales[i] for i in fields])
        self._gather(n, src, d, w, sc, B, None if idx_out is None else idx_out.data_ptr(), stream_id, st_ptr)

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
    (dataset.py:439-459 ``compute_cost_sample_prob`` output); None = uniform.

    A store that grows (``from_dataset`` / ``from_tables`` with ``capacity_rows`` / ``capacity_traj``): the row tables,
    ``traj_start`` / ``traj_len``, ``cdf`` and ``start_cdf`` are allocated once at their capacities and rewritten in
    place, the live trajectory count sits in one device word the window sampler reads (include/osrl_amd.h
    ``osrl_seq_gather_t.n_traj_dev``), and ``append`` adds whole trajectories after the live ones -- a captured CDT step
    follows at its next replay.  With ``evict="oldest"`` a full store drops its oldest trajectories to make room
    (``append``, ``evict_oldest``): the live trajectories stay dense and in age order in slots ``[0, n_traj)``, each one
    contiguous in the row tables, ``tail`` is the row behind the newest one, and ``n_rows`` is the sum of the live
    lengths -- the live rows are no longer a prefix of the row tables.  ``state_dict`` / ``load_state_dict`` save and
    restore a store built with capacities.
    (Switching an attached store between a uniform and a non-uniform distribution, or start sampling on and off, changes
    the launch's arguments as it always did: re-attach the store.)"""

    # a fixed store (the constructor, from_tables without capacities): no live word, nothing remembered
    _live: Optional[torch.Tensor] = None
    capacity_rows: Optional[int] = None
    capacity_traj: Optional[int] = None
    _dist: Optional[tuple] = None        # how the trajectory distribution was made: ("cost", transform) | ("pf", beta,
    _start_prob: Optional[float] = None  # frontier) | ("weights",) | ("cdf",); the ``prob`` of start sampling
    _traj_w: Optional[torch.Tensor] = None
    cost_reverse = False
    n_appended = 0
    version = 0
    evict: Optional[str] = None          # "oldest": append makes room by dropping whole trajectories, oldest first
    n_evicted = 0
    tail: Optional[int] = None           # (evicting stores) the row after the newest trajectory's last row
    _mirror: Optional[tuple] = None      # (evicting stores) host copy of the live (traj_start, traj_len), int64 arrays

    def __init__(self, trajectories, seq_len: int, device, reward_scale: float = 1.0, cost_scale: float = 1.0,
                 sample_prob=None, seed: int = 0, rank: int = 0, start_sampling: bool = False, prob: float = 0.4):
        dev = torch.device(device)
        cat = lambda k: torch.as_tensor(np.concatenate([np.asarray(t[k], np.float32).reshape(len(t["costs"]), -1)  # noqa: E731
                                                        for t in trajectories]), device=dev).contiguous()
        lens = np.array([len(t["costs"]) for t in trajectories], np.int64)
        tables = dict(observations=cat("observations"), actions=cat("actions"), returns=cat("returns").view(-1),
                      cost_returns=cat("cost_returns").view(-1), costs=cat("costs").view(-1),
                      traj_len=torch.as_tensor(lens.astype(np.int32), device=dev),
                      traj_start=torch.as_tensor(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), device=dev))
        cdf = None
        if sample_prob is not None:
            c = np.cumsum(np.asarray(sample_prob, np.float64))
            c /= c[-1]
            cdf = torch.as_tensor(c.astype(np.float32), device=dev)
        self._wrap(tables, seq_len, reward_scale, cost_scale, cdf, seed, rank, start_sampling, prob)

    def enable_start_sampling(self, prob: float = 0.4) -> None:
        """``SequenceDataset(start_sampling=True, prob=...)`` (dataset.py:742-744,781-783): window starts are drawn
        from ``compute_start_index_sample_prob`` instead of uniformly (computed on device, csrc/ingest.hip)."""
        from .ingest import compute_start_index_sample_prob
        t = self._live_tables()
        tables = dict(costs=t["costs"], traj_start=t["traj_start"], traj_len=t["traj_len"])
        self._start_prob = float(prob)
        self._set_table("start_cdf", compute_start_index_sample_prob(tables, prob, with_cdf=True)[1], self.capacity_rows)

    def _live_tables(self) -> Dict[str, torch.Tensor]:
        """The tables sliced to the live rows / trajectories (the tables themselves on a fixed store; the whole row tables
        and the live trajectories on a store that evicts)."""
        r, n = self.n_rows, self.n_traj
        if self.evict is not None:  # the live rows are wherever traj_start points: the whole row tables
            r = self.capacity_rows
        return dict(observations=self.obs[:r], actions=self.act[:r], returns=self.ret[:r], cost_returns=self.cret[:r],
                    costs=self.cost[:r], traj_start=self.traj_start[:n], traj_len=self.traj_len[:n])

    def _set_table(self, name: str, new: torch.Tensor, cap: Optional[int]) -> None:
        """``cdf`` / ``start_cdf``: a fresh tensor on a fixed store; on a store that grows one buffer at capacity,
        allocated at the first use and then rewritten in place (captured graphs hold its address).  Either way the
        gather's descriptor is rebuilt when the table's address changes."""
        if self._live is None:
            setattr(self, name, new)
            self._describe()
            return
        buf = getattr(self, name)
        if buf is None:
            buf = torch.zeros(cap, dtype=torch.float32, device=self.device)
            setattr(self, name, buf)
            self._describe()
        buf[:new.shape[0]].copy_(new)

    def set_sample_prob(self, weights) -> None:
        """Sample trajectories in proportion to ``weights``: any non-negative per-trajectory values (numpy or
        tensor, host or device), normalised and turned into the cdf the sampler reads on device.  Replaces any
        earlier trajectory distribution (``sample_prob``, ``cost_sample``, ``enable_pf_sampling``)."""
        from .ingest import sample_prob_from_weights
        w = _checked_weights(weights, self.n_traj, "trajectory").to(self.device)
        self._dist = ("weights",)
        if self._live is not None:  # kept, so that append(weights=) can extend them
            if self._traj_w is None:
                self._traj_w = torch.zeros(self.capacity_traj, dtype=torch.float64, device=self.device)
            self._traj_w[:self.n_traj].copy_(w)
        self._set_table("cdf", sample_prob_from_weights(w, with_cdf=True)[1], self.capacity_traj)

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
        t = self._live_tables()
        tables = dict(returns=t["returns"], cost_returns=t["cost_returns"], traj_start=t["traj_start"])
        self._dist = ("pf", float(beta), frontier)
        self._set_table("cdf", compute_sample_prob(tables, frontier, beta, with_cdf=True)[1], self.capacity_traj)

    def set_rank(self, rank: int) -> None:
        """Data parallel: every rank draws its own windows (same mixing as ReplayStore); the CDT engine calls this
        from ``attach_store`` when it runs under a DataParallel hook."""
        self.rank = int(rank)
        self.seed = self.base_seed * 1000003 + self.rank if self.rank else self.base_seed

    @classmethod
    def from_tables(cls, tables: Dict[str, torch.Tensor], seq_len: int, reward_scale: float = 1.0,
                    cost_scale: float = 1.0, cdf: Optional[torch.Tensor] = None, seed: int = 0,
                    rank: int = 0, start_sampling: bool = False, prob: float = 0.4,
                    capacity_rows: Optional[int] = None, capacity_traj: Optional[int] = None,
                    evict: Optional[str] = None) -> "SequenceStore":
        """Wrap the flat device tables of ``common.ingest.process_sequence_dataset`` (nothing is copied).
        ``capacity_rows`` / ``capacity_traj`` (either one; the other defaults to the tables' size): a store that grows --
        the tables are COPIED into allocations of those sizes, zero past the data, and ``append`` adds trajectories.
        ``evict="oldest"`` (only with capacities, ValueError otherwise): a full store drops its oldest trajectories."""
        self = cls.__new__(cls)
        self._wrap(tables, seq_len, reward_scale, cost_scale, cdf, seed, rank, start_sampling, prob, capacity_rows,
                   capacity_traj, evict)
        return self

    def _wrap(self, tables, seq_len, reward_scale, cost_scale, cdf, seed, rank, start_sampling, prob,
              capacity_rows=None, capacity_traj=None, evict=None) -> None:
        if evict not in (None, "oldest"):
            raise ValueError(f'evict must be None or "oldest", got {evict!r}')
        if evict is not None and capacity_rows is None and capacity_traj is None:
            raise ValueError('evict="oldest" needs a store built with capacity_rows= / capacity_traj=')
        self.T, self.device = int(seq_len), tables["observations"].device
        self.obs, self.act = tables["observations"].contiguous(), tables["actions"].contiguous()
        self.ret, self.cret, self.cost = tables["returns"], tables["cost_returns"], tables["costs"]
        self.traj_start, self.traj_len = tables["traj_start"], tables["traj_len"]
        self.n_traj = int(self.traj_start.shape[0])
        self.n_rows = int(self.obs.shape[0])
        if capacity_rows is not None or capacity_traj is not None:
            cr = self.n_rows if capacity_rows is None else int(capacity_rows)
            ct = self.n_traj if capacity_traj is None else int(capacity_traj)
            if cr < max(self.n_rows, 1) or ct < max(self.n_traj, 1):
                raise ValueError(f"capacities ({cr} rows, {ct} trajectories) below the data ({self.n_rows}, {self.n_traj})")
            self.capacity_rows, self.capacity_traj = cr, ct

            def grown(t, cap):
                full = torch.zeros((cap,) + tuple(t.shape[1:]), dtype=t.dtype, device=self.device)
                full[:t.shape[0]].copy_(t)
                return full
            self.obs, self.act = grown(self.obs, cr), grown(self.act, cr)
            self.ret, self.cret, self.cost = grown(self.ret, cr), grown(self.cret, cr), grown(self.cost, cr)
            self.traj_start, self.traj_len = grown(self.traj_start, ct), grown(self.traj_len, ct)
            self._live = torch.full((1,), self.n_traj, dtype=torch.int32, device=self.device)
            if cdf is not None:
                cdf = grown(cdf.to(torch.float32), ct)
            if evict is not None:
                self.evict, self.tail = evict, self.n_rows
                self._mirror = (tables["traj_start"].cpu().numpy().astype(np.int64).reshape(-1),
                                tables["traj_len"].cpu().numpy().astype(np.int64).reshape(-1))
        self.cdf = cdf
        if cdf is not None:
            self._dist = ("cdf",)
        self.reward_scale, self.cost_scale = float(reward_scale), float(cost_scale)
        self.base_seed = int(seed)
        self.set_rank(rank)
        self.od, self.ad = self.obs.shape[1], self.act.shape[1]
        self.start_cdf = None
        self._describe()
        if start_sampling:
            self.enable_start_sampling(prob)

    def _describe(self) -> None:
        """The table half of the window gather's descriptor (include/osrl_amd.h ``osrl_seq_gather_t``): rebuilt wherever
        a table's address can change (construction, a new ``cdf`` / ``start_cdf``); ``gather`` fills in the rest.  A store
        that grows carries its trajectory capacity and the address of the live-count word.
        RULE: whoever gives the store another tensor for a table, ``cdf`` or ``start_cdf`` calls this afterwards
        (``_set_table`` does); writing INTO the existing tensors, as ``append`` does, needs nothing."""
        g = self._g = L.SeqGatherT()
        g.obs, g.act, g.returns, g.cost_returns = self.obs.data_ptr(), self.act.data_ptr(), self.ret.data_ptr(), self.cret.data_ptr()
        g.costs, g.traj_start, g.traj_len = self.cost.data_ptr(), self.traj_start.data_ptr(), self.traj_len.data_ptr()
        g.cdf = None if self.cdf is None else self.cdf.data_ptr()
        g.start_cdf = None if self.start_cdf is None else self.start_cdf.data_ptr()
        g.n_traj = self.n_traj if self._live is None else self.capacity_traj
        g.n_traj_dev = None if self._live is None else self._live.data_ptr()
        g.T, g.od, g.ad, g.reward_scale, g.cost_scale = self.T, self.od, self.ad, self.reward_scale, self.cost_scale

    @classmethod
    def from_dataset(cls, dataset, seq_len: int, device, reward_scale: float = 1.0, cost_scale: float = 1.0,
                     cost_reverse: bool = False, cost_sample: bool = False,
                     cost_transform=("affine", -1.0, 50.0), seed: int = 0, rank: int = 0,
                     start_sampling: bool = False, prob: float = 0.4, deg: int = 3, pf_sample: bool = False,
                     max_rew_decrease: float = 1.0, beta: float = 1.0, augment_percent: float = 0,
                     max_reward: float = 1000.0, min_reward: float = 5, pf_only: bool = False, rmin: float = 0,
                     cost_bins: int = 60, npb: int = 5, random_aug: float = 0, aug_rmin: float = 0,
                     aug_rmax: float = 600, aug_cmin: float = 5, aug_cmax: float = 50, cgap: float = 5,
                     rstd: float = 1, cstd: float = 0.2, draws: Optional[dict] = None,
                     capacity_rows: Optional[int] = None, capacity_traj: Optional[int] = None,
                     evict: Optional[str] = None) -> "SequenceStore":
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
        over ``pf_sample``, and its beta is hard-wired to 1, dataset.py:734-737).
        ``capacity_rows`` / ``capacity_traj``: a store that grows (``append``); the capacities count the augmented
        trajectories too.  ``evict="oldest"`` (only with capacities): see ``append``."""
        from .ingest import augmentation, compute_cost_sample_prob, process_sequence_dataset, random_augmentation
        if evict not in (None, "oldest"):
            raise ValueError(f'evict must be None or "oldest", got {evict!r}')
        if evict is not None and capacity_rows is None and capacity_traj is None:
            raise ValueError('evict="oldest" needs a store built with capacity_rows= / capacity_traj=')
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
        self = cls.from_tables(tables, seq_len, reward_scale, cost_scale, cdf, seed, rank, start_sampling, prob,
                               capacity_rows, capacity_traj, evict)
        self.cost_reverse = bool(cost_reverse)
        self._dist = ("cost", cost_transform) if cost_sample else None
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
        g = self._g
        g.B, g.seed, g.stream_id = states.shape[0], self.seed, stream_id
        g.idx_in = None if idx_in is None else idx_in.data_ptr()
        g.idx_out = None if idx_out is None else idx_out.data_ptr()
        g.o_states, g.o_actions, g.o_returns, g.o_cost_returns = (states.data_ptr(), actions.data_ptr(), returns.data_ptr(),
                                                                  cost_returns.data_ptr())
        g.o_time_steps, g.o_mask, g.o_episode_cost, g.o_costs = (time_steps.data_ptr(), mask.data_ptr(),
                                                                 episode_cost.data_ptr(), costs.data_ptr())
        L.check(L.load().osrl_seq_window_gather(g, st_ptr, cur_stream()), "osrl_seq_window_gather")

    def check_append(self, n_traj: int, n_rows: int, **widths: int) -> None:
        """ValueError unless ``append`` (without ``weights=``) would take a chunk of ``n_traj`` trajectories in ``n_rows``
        rows with these column counts (``observations=17, actions=6``): the store grows, the chunk fits, the widths are
        the tables', and the trajectory distribution can follow (not ``set_sample_prob`` weights, not a ready-made cdf).
        A store that evicts makes room: only a chunk larger than the store itself does not fit.
        Nothing is changed: for callers that produce the chunk on device and want the refusal first."""
        if self._live is None:
            raise ValueError("this store is fixed: build it with capacity_rows= / capacity_traj= to append")
        for k, w in widths.items():
            want = {"observations": self.od, "actions": self.ad}[k]
            if int(w) != want:
                raise ValueError(f"the store's {k} have {want} columns, the new rows {int(w)}")
        kind = None if self._dist is None else self._dist[0]
        if kind == "cdf":
            raise ValueError("the trajectory distribution was given as a cdf: call set_sample_prob(weights) before append")
        if kind == "weights":
            raise ValueError("the store draws by set_sample_prob's weights: append(dataset, weights=) needs the new "
                             "trajectories' weights")
        if self.evict is not None:
            if int(n_rows) > self.capacity_rows or int(n_traj) > self.capacity_traj:
                raise ValueError(f"the chunk ({int(n_rows)} rows, {int(n_traj)} trajectories) is larger than the store "
                                 f"({self.capacity_rows} rows, {self.capacity_traj} trajectories)")
            return
        if self.n_traj + int(n_traj) > self.capacity_traj or self.n_rows + int(n_rows) > self.capacity_rows:
            raise ValueError(f"the chunk ({int(n_rows)} rows, {int(n_traj)} trajectories) does not fit: {self.n_rows} of "
                             f"{self.capacity_rows} rows and {self.n_traj} of {self.capacity_traj} trajectories are live")

    def append(self, dataset, weights=None) -> None:
        """Add the complete episodes of ``dataset`` (DSRL keys, host or device) to a store built with capacities: the
        chunk goes through ``process_sequence_dataset`` as a dataset of its own (with the store's ``cost_reverse``) and
        its trajectories are appended after the live ones, in place, on the current stream.  Without ``evict`` there is no
        ring: a chunk that does not fit raises ValueError and changes nothing.  New chunks are not augmented (``n_original`` /
        ``n_augmented`` describe the construction-time data, ``n_appended`` counts the rest).
        The trajectory distribution follows the data: ``cost_sample`` (its transform), ``enable_pf_sampling`` (its beta
        and frontier) and start sampling (its ``prob``) are recomputed over the live trajectories into the same buffers.
        After ``set_sample_prob`` the new trajectories need ``weights=`` (ValueError without); a store whose distribution
        was given as a ready-made cdf cannot extend it (ValueError: call ``set_sample_prob`` first).
        ``evict="oldest"``: a chunk that does not fit makes room instead (``seq_ring_plan``, DESIGN.md "Stores that
        grow"): it lands behind the newest trajectory, or at row 0 when it does not fit there, and the oldest
        trajectories are dropped, whole, until none touches its rows and there are slots for its trajectories; only a
        chunk larger than the store raises.  ``n_evicted`` counts the dropped trajectories."""
        from .ingest import process_sequence_dataset
        if self._live is None:
            raise ValueError("this store is fixed: build it with capacity_rows= / capacity_traj= to append")
        shape = lambda x: tuple(x.shape) if torch.is_tensor(x) else np.shape(x)  # noqa: E731
        for k, want in (("observations", self.od), ("actions", self.ad)):
            sh = shape(dataset[k])
            if int(np.prod(sh[1:], dtype=np.int64)) != want:
                raise ValueError(f"the store's {k} have {want} columns, the new rows {int(np.prod(sh[1:]))}")
        kind = None if self._dist is None else self._dist[0]
        if kind == "cdf":
            raise ValueError("the trajectory distribution was given as a cdf: call set_sample_prob(weights) before append")
        if kind == "weights" and weights is None:
            raise ValueError("the store draws by set_sample_prob's weights: append(dataset, weights=) needs the new "
                             "trajectories' weights")
        if kind != "weights" and weights is not None:
            raise ValueError("weights= extends the weights of set_sample_prob, which this store does not draw by")
        t = process_sequence_dataset(dataset, self.cost_reverse, self.device)
        mt, mr = int(t["traj_start"].shape[0]), int(t["observations"].shape[0])
        if self.evict is not None:
            if mr > self.capacity_rows or mt > self.capacity_traj:
                raise ValueError(f"the chunk ({mr} rows, {mt} trajectories) is larger than the store "
                                 f"({self.capacity_rows} rows, {self.capacity_traj} trajectories)")
        elif self.n_traj + mt > self.capacity_traj or self.n_rows + mr > self.capacity_rows:
            raise ValueError(f"the chunk ({mr} rows, {mt} trajectories) does not fit: {self.n_rows} of "
                             f"{self.capacity_rows} rows and {self.n_traj} of {self.capacity_traj} trajectories are live")
        w_new = None if weights is None else _checked_weights(weights, mt, "trajectory", positive_sum=False).to(self.device)
        if mt == 0:
            return
        r0, n0 = self.n_rows, self.n_traj
        if self.evict is not None:
            # the plan on the host mirror (one small copy of the chunk's lengths), then in stream order: drop the oldest
            # entries and lower the live word (one launch), write the rows, add the entries -- a sampler replayed on this
            # stream never sees an entry that points at overwritten rows
            lens = t["traj_len"].cpu().numpy().astype(np.int64)
            r0, k, tail = seq_ring_plan(*self._mirror, self.tail, mr, mt, self.capacity_rows, self.capacity_traj)
            self._drop_front(k)
            n0 = self.n_traj
            self._mirror = (np.concatenate([self._mirror[0], r0 + np.cumsum(lens) - lens]),
                            np.concatenate([self._mirror[1], lens]))
            self.tail = tail
        self.obs[r0:r0 + mr].copy_(t["observations"].reshape(mr, -1))
        self.act[r0:r0 + mr].copy_(t["actions"].reshape(mr, -1))
        self.ret[r0:r0 + mr].copy_(t["returns"])
        self.cret[r0:r0 + mr].copy_(t["cost_returns"])
        self.cost[r0:r0 + mr].copy_(t["costs"])
        self.traj_start[n0:n0 + mt].copy_(t["traj_start"] + r0)
        self.traj_len[n0:n0 + mt].copy_(t["traj_len"])
        self.n_rows, self.n_traj = (r0 + mr, n0 + mt) if self.evict is None else (int(self._mirror[1].sum()), n0 + mt)
        self.n_appended += mt
        self.version += 1
        if kind == "weights":
            self._traj_w[n0:n0 + mt].copy_(w_new)
        self._redistribute()
        self._live.fill_(self.n_traj)  # last: the tables and the distributions are in place when the count moves

    def _redistribute(self) -> None:
        """The trajectory distribution and the start distribution over the live trajectories, from the recipe the store
        remembers (``_dist``, ``_start_prob``), into the buffers the sampler already reads."""
        from .ingest import (compute_cost_sample_prob, compute_sample_prob, compute_start_index_sample_prob,
                             sample_prob_from_weights)
        kind = None if self._dist is None else self._dist[0]
        lt = self._live_tables()
        if kind == "cost":
            self._set_table("cdf", compute_cost_sample_prob(lt, self._dist[1], with_cdf=True)[1], self.capacity_traj)
        elif kind == "pf":
            self._set_table("cdf", compute_sample_prob(lt, self._dist[2], self._dist[1], with_cdf=True)[1],
                            self.capacity_traj)
        elif kind == "weights":
            self._set_table("cdf", sample_prob_from_weights(self._traj_w[:self.n_traj], with_cdf=True)[1],
                            self.capacity_traj)
        if self._start_prob is not None:
            self._set_table("start_cdf", compute_start_index_sample_prob(lt, self._start_prob, with_cdf=True)[1],
                            self.capacity_rows)

    # ---- eviction -----------------------------------------------------------------------------------------------------
    def _drop_front(self, k: int) -> None:
        """The ``k`` oldest trajectories leave the tables, the host mirror and the counts: one ``osrl_seq_evict_front``
        launch on the current stream shifts ``traj_start`` / ``traj_len`` (and the ``set_sample_prob`` weights) to slot
        0 in place, zeroes the vacated slots and lowers the live word.  The rows stay where they are."""
        if k == 0:
            return
        e = L.SeqEvictT()
        e.traj_start, e.traj_len, e.n_traj_dev = self.traj_start.data_ptr(), self.traj_len.data_ptr(), self._live.data_ptr()
        e.traj_w = None if self._traj_w is None else self._traj_w.data_ptr()
        e.n_live, e.n_drop = self.n_traj, k
        L.check(L.load().osrl_seq_evict_front(e, cur_stream()), "osrl_seq_evict_front")
        self._mirror = (self._mirror[0][k:], self._mirror[1][k:])
        self.n_traj -= k
        self.n_rows = int(self._mirror[1].sum())
        self.n_evicted += k

    def evict_oldest(self, k: int) -> None:
        """Drop the ``k`` oldest trajectories of a store built with ``evict="oldest"``, in place on the current stream
        (their rows are simply no longer referenced), and recompute the distributions over the rest.
        ``0 <= k < n_traj`` -- the store never becomes empty this way -- ValueError otherwise, nothing changed.
        ``n_evicted`` and, unless ``k`` is 0, ``version`` move."""
        if self.evict is None:
            raise ValueError('this store does not evict: build it with evict="oldest"')
        k = int(k)
        if not 0 <= k < self.n_traj:
            raise ValueError(f"evict_oldest({k}): 0 .. {self.n_traj - 1} of the {self.n_traj} live trajectories can go")
        if k == 0:
            return
        kind = None if self._dist is None else self._dist[0]
        if kind == "cdf":
            raise ValueError("the trajectory distribution was given as a cdf: call set_sample_prob(weights) before "
                             "evict_oldest")
        self._drop_front(k)
        self.version += 1
        self._redistribute()

    # ---- checkpointing (common.checkpoint.save_store / load_store) ------------------------------------------------------
    def _recipe(self):
        """``_dist`` as plain data: the tuple forms as they are, a frontier as its tensors."""
        d = self._dist
        if d is None or d[0] in ("weights", "cdf"):
            return None if d is None else (d[0],)
        if d[0] == "cost":
            if callable(d[1]):
                raise ValueError('a python callable cost_transform cannot be saved: use ("affine", a, b) or '
                                 '("reciprocal", b)')
            return ("cost", tuple(d[1]))
        f = d[2]
        cpu = lambda x: x.detach().cpu().clone()  # noqa: E731
        return ("pf", float(d[1]), dict(coef=cpu(f.coef_dev), deg=cpu(f.deg_dev), pareto_idx=cpu(f._pidx),
                                        pcount=cpu(f._pcount), stats=cpu(f.stats)))

    def _config(self) -> dict:
        return dict(capacity_rows=self.capacity_rows, capacity_traj=self.capacity_traj, seq_len=self.T,
                    observations=self.od, actions=self.ad, reward_scale=self.reward_scale, cost_scale=self.cost_scale,
                    evict=self.evict)

    def state_dict(self) -> dict:
        """The contents of a store built with capacities, as host tensors, numbers, strings and tuples: the row tables as
        they lie up to the last used row (the physical layout: where the next chunk lands and what it evicts depends on
        it), the live trajectory tables, ``tail`` and the counters, the ``set_sample_prob`` weights, the cdf tables, and
        the recipe of the trajectory distribution (a frontier as its tensors).  Seeds and ranks belong to the constructor.
        ValueError on a fixed store (it is rebuilt from its dataset) and with a python callable ``cost_transform``."""
        if self._live is None:
            raise ValueError("this store is fixed: it is rebuilt from its dataset, only a store built with capacity_rows= "
                             "/ capacity_traj= is saved")
        recipe = self._recipe()
        n = self.n_traj
        used = self.n_rows if self.evict is None else int((self._mirror[0] + self._mirror[1]).max())
        cpu = lambda x, m: None if x is None else x[:m].detach().cpu().clone()  # noqa: E731
        return dict(kind="SequenceStore", format=1, config=self._config(), n_traj=n, n_rows=self.n_rows, used_rows=used,
                    tail=self.tail, n_evicted=self.n_evicted, n_appended=self.n_appended,
                    n_original=getattr(self, "n_original", None), n_augmented=getattr(self, "n_augmented", None),
                    cost_reverse=bool(self.cost_reverse), start_prob=self._start_prob, dist=recipe,
                    tables=dict(observations=cpu(self.obs, used), actions=cpu(self.act, used), returns=cpu(self.ret, used),
                                cost_returns=cpu(self.cret, used), costs=cpu(self.cost, used),
                                traj_start=cpu(self.traj_start, n), traj_len=cpu(self.traj_len, n)),
                    traj_w=cpu(self._traj_w, n), cdf=cpu(self.cdf, n), start_cdf=cpu(self.start_cdf, used))

    def load_state_dict(self, sd: dict) -> None:
        """Make this store the saved one, in the allocations it has: it then draws the same windows, and every later
        ``append`` lands, evicts and reweights the same.  The store must have been built with the saved capacities,
        widths, ``seq_len``, scales and ``evict`` (ValueError naming the difference, before any device work).  The
        tables are written in place on the current stream, live word last, so an attached engine follows at its next
        replay; ``version`` is incremented.  (A store that had no ``cdf`` / ``start_cdf`` table and gets one, or the
        reverse, changes the gather's arguments as ``set_sample_prob`` does: re-attach it.)  What the augmentation of
        this store's own construction left behind (``aug_info``) does not describe the loaded data and is dropped."""
        from .ingest import Frontier
        if self._live is None:
            raise ValueError("this store is fixed: build it with capacity_rows= / capacity_traj= to load a saved store "
                             "into it")
        if sd.get("kind") != "SequenceStore" or sd.get("format") != 1:
            raise ValueError(f"not a saved SequenceStore (kind {sd.get('kind')!r}, format {sd.get('format')!r})")
        mine = self._config()
        for what, theirs in sd["config"].items():
            if mine[what] != theirs:
                raise ValueError(f"the saved store's {what} is {theirs}, this store's {mine[what]}")
        n, used, dev = int(sd["n_traj"]), int(sd["used_rows"]), self.device
        tb = sd["tables"]
        for dst, key in ((self.obs, "observations"), (self.act, "actions"), (self.ret, "returns"),
                         (self.cret, "cost_returns"), (self.cost, "costs")):
            dst[:used].copy_(tb[key])
            dst[used:].zero_()
        for dst, key in ((self.traj_start, "traj_start"), (self.traj_len, "traj_len")):
            dst[:n].copy_(tb[key])
            dst[n:].zero_()
        if sd["traj_w"] is not None:
            if self._traj_w is None:
                self._traj_w = torch.zeros(self.capacity_traj, dtype=torch.float64, device=dev)
            self._traj_w[:n].copy_(sd["traj_w"])
            self._traj_w[n:].zero_()
        else:
            self._traj_w = None
        for name, cap in (("cdf", self.capacity_traj), ("start_cdf", self.capacity_rows)):
            if sd[name] is None:
                if getattr(self, name) is not None:
                    setattr(self, name, None)
                    self._describe()
            else:
                if getattr(self, name) is not None:
                    getattr(self, name).zero_()
                self._set_table(name, sd[name].to(dev), cap)
        d = sd["dist"]
        if d is not None and d[0] == "pf":
            f = {k: v.to(dev) for k, v in d[2].items()}
            d = ("pf", float(d[1]), Frontier(f["coef"], f["deg"], f["pareto_idx"], f["pcount"], f["stats"]))
        elif d is not None and d[0] == "cost":
            d = ("cost", tuple(d[1]))
        self._dist = None if d is None else tuple(d)
        self._start_prob = sd["start_prob"]
        self.cost_reverse = bool(sd["cost_reverse"])
        self.n_traj, self.n_rows, self.tail = n, int(sd["n_rows"]), sd["tail"]
        self.n_evicted, self.n_appended = int(sd["n_evicted"]), int(sd["n_appended"])
        for k in ("n_original", "n_augmented"):
            if sd[k] is not None:
                setattr(self, k, int(sd[k]))
        self.aug_info = None
        if self.evict is not None:
            self._mirror = (tb["traj_start"].numpy().astype(np.int64).reshape(-1),
                            tb["traj_len"].numpy().astype(np.int64).reshape(-1))
        self.version += 1
        self._live.fill_(n)
