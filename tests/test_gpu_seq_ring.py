"""SequenceStore(evict="oldest") and checkpointing of stores on the GPU (csrc/seq_ring.hip ``osrl_seq_evict_front``,
common/replay.py, common/checkpoint.py ``save_store`` / ``load_store``).  Every comparison is exact: a window is a pure
function of (seed, step, sample, live trajectory tables), the live trajectories of an evicting store are dense and in age
order, and the cdf kernels walk them through ``traj_start`` -- so an evicting store draws what a fixed store built from
the concatenation of its survivors draws, bit for bit, wherever the survivors' rows lie.  The survivors come from this
file's own model of the rule (tests/test_seq_ring_cpu.py ``Model``: an occupancy array and an age list), not from
``seq_ring_plan``.

Shapes: those of tests/test_gpu_store_append.py (12 trajectories of 3..9 steps in 67 rows per chunk, od 5, ad 2, T 4)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from test_gpu_store_append import (AD, CS, DEV, LENS, OD, RS, T, _cat, _data, _draws, _episodes, _same_draws,  # noqa: E402
                                   _same_windows, _store, _windows)
from test_seq_ring_cpu import Model  # noqa: E402

pytestmark = pytest.mark.gpu
OFFS = np.concatenate([[0], np.cumsum(LENS)])
KW = dict(reward_scale=RS, cost_scale=CS, seed=3)


# ---- 1. the kernel alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_w", [False, True])
@pytest.mark.parametrize("n_live,n_drop", [(1, 0), (1, 1), (5, 1), (5, 5), (70, 1), (70, 63), (70, 64), (3000, 1),
                                           (3000, 1023), (3000, 1025), (3000, 2999)])
def test_the_kernel_shifts_in_place(n_live, n_drop, with_w):
    """A shift below one wave, below one 1024-entry pass and across passes: the sizes at which an in-place pass could
    read what it has already overwritten.  37 entries past ``n_live`` must stay as they are."""
    from osrl_amd import _lib as L
    from osrl_amd.engine.core import cur_stream
    n = n_live + 37
    rs = np.random.RandomState(n_live * 7 + n_drop)
    start = rs.randint(1, 2 ** 40, size=n).astype(np.int64)
    length = rs.randint(1, 2 ** 20, size=n).astype(np.int32)
    w = rs.uniform(1.0, 2.0, size=n)
    d_start, d_len, d_w = (torch.as_tensor(x, device=DEV) for x in (start, length, w))
    word = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    e = L.SeqEvictT()
    e.traj_start, e.traj_len, e.n_traj_dev = d_start.data_ptr(), d_len.data_ptr(), word.data_ptr()
    e.traj_w = d_w.data_ptr() if with_w else None
    e.n_live, e.n_drop = n_live, n_drop
    L.check(L.load().osrl_seq_evict_front(e, cur_stream()), "osrl_seq_evict_front")
    torch.cuda.synchronize()

    def want(a):
        return np.concatenate([a[n_drop:n_live], np.zeros(n_drop, a.dtype), a[n_live:]])
    np.testing.assert_array_equal(d_start.cpu().numpy(), want(start))
    np.testing.assert_array_equal(d_len.cpu().numpy(), want(length))
    np.testing.assert_array_equal(d_w.cpu().numpy(), want(w) if with_w else w)
    assert int(word.item()) == n_live - n_drop


def test_the_kernel_refuses_a_bad_descriptor():
    from osrl_amd import _lib as L
    a = torch.ones(8, dtype=torch.int64, device=DEV)
    b = torch.ones(8, dtype=torch.int32, device=DEV)
    word = torch.full((1,), 8, dtype=torch.int32, device=DEV)

    def rc(n_live=8, n_drop=1, start=a, length=b, live=word):
        e = L.SeqEvictT()
        e.traj_start = None if start is None else start.data_ptr()
        e.traj_len = None if length is None else length.data_ptr()
        e.n_traj_dev = None if live is None else live.data_ptr()
        e.n_live, e.n_drop = n_live, n_drop
        return L.load().osrl_seq_evict_front(e, None)
    assert rc(n_drop=9) == -1 and rc(n_drop=-1) == -1 and rc(n_live=(1 << 20) + 1) == -1
    assert rc(start=None) == -1 and rc(length=None) == -1 and rc(live=None) == -1
    torch.cuda.synchronize()
    assert int(word.item()) == 8 and bool((a == 1).all()) and bool((b == 1).all())


# ---- 2. an evicting store draws what the store of its survivors draws ---------------------------------------------------
def _traj(d, j):
    return {k: v[OFFS[j]:OFFS[j + 1]] for k, v in d.items()}


def _first(d, n):
    return {k: v[:OFFS[n]] for k, v in d.items()}


class Tracker:
    """The brute-force model plus, per trajectory id, where its rows came from and its explicit weight."""

    def __init__(self, d, n, cr, ct):
        self.m = Model(list(LENS[:n]), cr, ct)
        self.origin = [_traj(d, j) for j in range(n)]
        self.evicted = 0

    def append(self, d):
        _, k, _ = self.m.append(list(LENS))
        self.origin += [_traj(d, j) for j in range(len(LENS))]
        self.evicted += k

    def drop(self, k):
        for _ in range(k):
            start, n = self.m.where.pop(self.m.age.pop(0))
            self.m.cell[start:start + n] = -1
        self.evicted += k

    def survivors(self):
        out = self.origin[self.m.age[0]]
        for i in self.m.age[1:]:
            out = _cat(out, self.origin[i])
        return out

    def weights(self, ids=None):
        return np.array([1.0 + (i * 7) % 5 for i in (self.m.age if ids is None else ids)])


def _frontier():
    from osrl_amd.common import ingest
    d = _episodes(1)
    c = np.array([_traj(d, j)["costs"].sum() for j in range(len(LENS))], np.float64)
    r = np.array([_traj(d, j)["rewards"].sum() for j in range(len(LENS))], np.float64)
    return ingest.pareto_frontier(c, r, deg=2, device=DEV)


MODES = {"uniform": {}, "cost_sample": dict(cost_sample=True), "start_sampling": dict(start_sampling=True),
         "weights": {}, "pf": {}}


def _install(store, mode, weights, frontier):
    if mode == "weights":
        store.set_sample_prob(weights)
    if mode == "pf":
        store.enable_pf_sampling(beta=0.7, frontier=frontier)


def _tables(s):
    return [t for t in (s.obs, s.act, s.ret, s.cret, s.cost, s.traj_start, s.traj_len, s.cdf, s.start_cdf, s._live,
                        s._traj_w) if t is not None]


def _check(store, tr, mode, frontier, what, steps=4):
    """``store`` against the fixed store of the model's survivors: counts, the host mirror, the windows."""
    from osrl_amd.common.replay import SequenceStore
    live = tr.m.live()
    assert (store.n_traj, store.n_evicted, store.tail) == (len(live), tr.evicted, tr.m.tail), what
    assert store.n_rows == sum(n for _, n in live) and int(store._live.item()) == len(live)
    assert list(zip(store._mirror[0].tolist(), store._mirror[1].tolist())) == live
    np.testing.assert_array_equal(store.traj_start[:len(live)].cpu().numpy(), [s for s, _ in live])
    np.testing.assert_array_equal(store.traj_len[:len(live)].cpu().numpy(), [n for _, n in live])
    fresh = SequenceStore.from_dataset(tr.survivors(), T, DEV, **KW, **MODES[mode])
    _install(fresh, mode, tr.weights(), frontier)
    a, b = _windows((store, fresh), steps)
    _same_windows(a, b, f"{mode}: {what}")
    return a


@pytest.mark.parametrize("mode", sorted(MODES))
def test_an_evicting_store_draws_what_the_store_of_its_survivors_draws(mode):
    """100 rows, 20 slots, the first 4 trajectories (18 rows) of ``_episodes(1)``; then three chunks of 12 trajectories in
    67 rows.  The first lands at row 18 and evicts nothing (16 live, tail 85).  The second does not fit behind row 85: it
    lands at row 0, leaves the gap [85, 100) and evicts the 4 + 9 trajectories that touch [0, 67) -- the 3 at rows
    [67, 85) survive, OLDER than the new ones and at HIGHER rows.  The third lands at row 0 again (tail 67) and, oldest
    first, evicts everything."""
    from osrl_amd.common.replay import SequenceStore
    d0 = _episodes(1)
    fr = _frontier() if mode == "pf" else None
    tr = Tracker(d0, 4, 100, 20)
    store = SequenceStore.from_dataset(_first(d0, 4), T, DEV, capacity_rows=100, capacity_traj=20, evict="oldest", **KW,
                                       **MODES[mode])
    _install(store, mode, tr.weights(), fr)
    ptrs = [t.data_ptr() for t in _tables(store)]
    _check(store, tr, mode, fr, "as built", steps=2)
    evicted = []
    for v, seed in enumerate((2, 3, 4), 1):
        d = _episodes(seed)
        first_new = tr.m.next_id
        tr.append(d)
        store.append(d, **(dict(weights=tr.weights(range(first_new, first_new + 12))) if mode == "weights" else {}))
        assert store.version == v and store.n_appended == 12 * v
        drawn = _check(store, tr, mode, fr, f"append {v}")
        assert [t.data_ptr() for t in _tables(store)] == ptrs, "a table moved"
        evicted.append(tr.evicted)
        assert max(int(x[-1][:, 0].max()) for x in drawn) >= store.n_traj - 12  # (the new trajectories are reached)
    assert evicted == [0, 13, 28] and store.tail == 67 and store.n_traj == 12


@pytest.mark.parametrize("mode", ["cost_start", "weights"])
@pytest.mark.parametrize("k", [0, 1, 11])
def test_evict_oldest(k, mode):
    from osrl_amd.common.replay import SequenceStore
    d0 = _episodes(1)
    kw = dict(cost_sample=True, start_sampling=True) if mode == "cost_start" else {}
    tr = Tracker(d0, 12, 100, 20)
    store = SequenceStore.from_dataset(d0, T, DEV, capacity_rows=100, capacity_traj=20, evict="oldest", **KW, **kw)
    _install(store, mode, tr.weights(), None)
    ptrs = [t.data_ptr() for t in _tables(store)]
    for bad in (12, 13, -1):
        with pytest.raises(ValueError):
            store.evict_oldest(bad)
    assert (store.n_traj, store.n_evicted, store.version, int(store._live.item())) == (12, 0, 0, 12)
    store.evict_oldest(k)
    tr.drop(k)
    assert store.version == (1 if k else 0) and [t.data_ptr() for t in _tables(store)] == ptrs
    fresh = SequenceStore.from_dataset(tr.survivors(), T, DEV, **KW, **kw)
    _install(fresh, mode, tr.weights(), None)
    live = tr.m.live()
    assert (store.n_traj, store.n_evicted, store.tail, store.n_rows) == (12 - k, k, 67, sum(n for _, n in live))
    assert list(zip(store._mirror[0].tolist(), store._mirror[1].tolist())) == live
    _same_windows(*_windows((store, fresh), 4), f"evict_oldest({k})")
    with pytest.raises(ValueError):
        SequenceStore.from_dataset(d0, T, DEV, capacity_rows=100, capacity_traj=20, **KW).evict_oldest(1)


def test_the_default_is_unchanged():
    from osrl_amd.common.replay import SequenceStore
    n = sum(LENS)
    d0, d1 = _episodes(1), _episodes(2)
    s = SequenceStore.from_dataset(d0, T, DEV, cost_sample=True, capacity_rows=100, capacity_traj=20, **KW)
    assert s.evict is None and s.tail is None and s.n_evicted == 0
    before = [t.clone() for t in _tables(s)]
    with pytest.raises(ValueError, match="does not fit"):
        s.append(d1)
    with pytest.raises(ValueError, match="does not fit"):
        s.check_append(12, n, observations=OD, actions=AD)
    assert (s.n_traj, s.n_rows, s.n_appended, s.version, int(s._live.item())) == (12, n, 0, 0, 12)
    assert all(torch.equal(x, y) for x, y in zip(before, _tables(s)))
    for build in (lambda **kw: SequenceStore.from_dataset(d0, T, DEV, **kw),
                  lambda **kw: SequenceStore.from_tables(dict(observations=s.obs[:n], actions=s.act[:n], returns=s.ret[:n],
                                                              cost_returns=s.cret[:n], costs=s.cost[:n],
                                                              traj_start=s.traj_start[:12], traj_len=s.traj_len[:12]),
                                                         T, **kw)):
        with pytest.raises(ValueError, match="capacity"):
            build(evict="oldest")
        with pytest.raises(ValueError, match="evict"):
            build(evict="newest", capacity_rows=100)
        assert build(evict="oldest", capacity_rows=100).evict == "oldest"
    # an evicting store refuses only what can never fit, and changes nothing when it does
    e = SequenceStore.from_dataset(d0, T, DEV, cost_sample=True, capacity_rows=66 + n, capacity_traj=11 + 12,
                                   evict="oldest", **KW)
    e.check_append(12, n, observations=OD, actions=AD)
    from osrl_amd.engine.act import check_jobs_store
    check_jobs_store(e, 12, 9, OD, AD)  # (collect_jobs(into=) asks the same question before its run)
    with pytest.raises(ValueError, match="does not fit"):
        check_jobs_store(s, 12, 9, OD, AD)
    with pytest.raises(ValueError, match="larger than the store"):
        check_jobs_store(e, 24, 9, OD, AD)
    small =SequenceStore.from_dataset(_first(d0, 4), T, DEV, cost_sample=True, capacity_rows=n - 1, capacity_traj=20,
                                       evict="oldest", **KW)
    few = SequenceStore.from_dataset(_first(d0, 4), T, DEV, cost_sample=True, capacity_rows=100, capacity_traj=11,
                                     evict="oldest", **KW)
    for st in (small, few):
        before = [t.clone() for t in _tables(st)]
        with pytest.raises(ValueError, match="larger than the store"):
            st.check_append(12, n, observations=OD, actions=AD)
        with pytest.raises(ValueError, match="larger than the store"):
            st.append(d1)
        with pytest.raises(ValueError, match="columns"):
            st.check_append(1, 1, observations=OD + 1)
        assert (st.n_traj, st.n_evicted, st.version, st.tail, int(st._live.item())) == (4, 0, 0, 18, 4)
        assert all(torch.equal(x, y) for x, y in zip(before, _tables(st)))


# ---- 3. the CDT step ------------------------------------------------------------------------------------------------------
def test_the_cdt_step_follows_an_eviction_with_the_graph_it_has():
    """2 + 2 ``step_store`` calls around two appends, the second of which lands at row 0 and evicts 13 trajectories (see
    above), on the graph captured before them, against a fresh engine stepped on fixed stores: the first 18 rows for two
    steps, then the store of the survivors.  ``time_emb=False``: see
    tests/test_gpu_store_append.py test_the_cdt_step_follows_an_append_with_the_graph_it_has."""
    from osrl_amd.algorithms import CDT, CDTTrainer
    from osrl_amd.common.logger import DummyLogger
    from osrl_amd.common.replay import SequenceStore
    d0, d1, d2 = _episodes(1), _episodes(2), _episodes(3)

    def engine():
        torch.manual_seed(0)
        m = CDT(OD, AD, 1.0, seq_len=T, episode_len=16, embedding_dim=32, num_layers=1, num_heads=2, time_emb=False,
                use_rew=True, use_cost=True, device=DEV)
        tr = CDTTrainer(m, None, DummyLogger(), learning_rate=1e-3, lr_warmup_steps=3, reward_scale=RS, cost_scale=CS,
                        device=DEV, stats_mode="none")
        return m, m.engine(8, tr.cfg)

    ma, ea = engine()
    store = SequenceStore.from_dataset(_first(d0, 4), T, DEV, capacity_rows=100, capacity_traj=20, evict="oldest", **KW)
    tr = Tracker(d0, 4, 100, 20)
    ea.attach_store(store)
    ea.step_store()
    ea.step_store()
    g = ea.graph
    assert g is not None
    for d in (d1, d2):
        store.append(d)
        tr.append(d)
    assert store.n_evicted == tr.evicted == 13 and store.n_traj == 15
    ea.step_store()
    ea.step_store()
    torch.cuda.synchronize()
    assert ea.graph is g
    mb, eb = engine()
    eb.attach_store(SequenceStore.from_dataset(_first(d0, 4), T, DEV, **KW))
    eb.step_store()
    eb.step_store()
    eb.attach_store(SequenceStore.from_dataset(tr.survivors(), T, DEV, **KW))
    eb.step_store()
    eb.step_store()
    torch.cuda.synchronize()
    assert ea.st.device_step() == eb.st.device_step() == 4
    for x, y in ((ea.states, eb.states), (ea.actions, eb.actions), (ea.time_steps, eb.time_steps)):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
    for name in ("p", "m", "v"):
        np.testing.assert_array_equal(getattr(ea.g, name).cpu().numpy(), getattr(eb.g, name).cpu().numpy(), err_msg=name)
    for s in range(1, 5):
        ra, rb = ea.st.read_stats(s), eb.st.read_stats(s)
        np.testing.assert_array_equal(np.array(list(ra.values())), np.array(list(rb.values())), err_msg=f"step {s}")


# ---- 4. collect_targets(into=) ----------------------------------------------------------------------------------------------
def test_collect_targets_into_a_full_evicting_store():
    """4 episodes x 8 steps per round into a store of 48 rows and 6 slots that starts with 2 episodes.  Round 1 ends at
    the last row exactly and fills the slots; round 2 lands at row 0 and evicts the two seed episodes and the first two
    of round 1: the store then holds round 1's episodes 2, 3 and round 2's four, in that order."""
    from osrl_amd.algorithms import CDT, CDTTrainer
    from osrl_amd.common.logger import DummyLogger
    from osrl_amd.common.replay import SequenceStore
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv, VecSyntheticSafeEnv
    from osrl_amd.engine.collect import merge_datasets
    E, EL = 4, 8
    torch.manual_seed(0)
    m = CDT(OD, AD, 1.0, seq_len=T, episode_len=EL, embedding_dim=32, num_layers=1, num_heads=2, time_emb=False,
            use_rew=True, use_cost=True, stochastic=True, target_entropy=-AD, device=DEV)
    tr = CDTTrainer(m, None, DummyLogger(), learning_rate=1e-3, lr_warmup_steps=3, reward_scale=RS, cost_scale=CS,
                    device=DEV, stats_mode="none")
    tr.env = VecSyntheticSafeEnv(SyntheticSafeEnv(OD, AD, EL, seed=3, init_noise=0.5), E, DEV, base_seed=7)
    gr, gc = np.array([30.0, 10.0, 20.0, 15.0]), np.array([5.0, 1.0, 3.0, 2.0])
    rows = lambda d, a, b: {k: v[a * EL:b * EL] for k, v in d.items()}  # noqa: E731
    d0, d1, d2 = (tr.collect_targets(gr, gc, sample=True, seed=s).dataset for s in (0, 1, 2))
    store = SequenceStore.from_dataset(rows(d0, 0, 2), T, DEV, capacity_rows=6 * EL, capacity_traj=6, evict="oldest", **KW)
    ptrs = [t.data_ptr() for t in _tables(store)]
    res = tr.collect_targets(gr, gc, sample=True, seed=1, into=store)
    assert res.dataset is None and (res.lengths == EL).all()
    assert (store.n_traj, store.n_rows, store.tail, store.n_evicted, store.version) == (6, 6 * EL, 6 * EL, 0, 1)
    tr.collect_targets(gr, gc, sample=True, seed=2, into=store)
    assert (store.n_traj, store.n_rows, store.tail, store.n_evicted, store.version) == (6, 6 * EL, 4 * EL, 4, 2)
    assert [t.data_ptr() for t in _tables(store)] == ptrs
    np.testing.assert_array_equal(store.traj_start[:6].cpu().numpy(), np.array([4, 5, 0, 1, 2, 3]) * EL)
    newest = merge_datasets([rows(d1, 2, 4), d2])
    at = (store.traj_start[:6, None] + torch.arange(EL, device=DEV)[None]).reshape(-1)
    assert torch.equal(store.obs[at], newest["observations"].reshape(6 * EL, -1).to(torch.float32))
    assert torch.equal(store.act[at], newest["actions"].reshape(6 * EL, -1).to(torch.float32))
    _same_windows(*_windows((store, SequenceStore.from_dataset(newest, T, DEV, **KW)), 3), "the newest episodes")
    # fewer slots than one round has episodes: refused before the run, the environment's totals and the store untouched
    tiny = SequenceStore.from_dataset(rows(d0, 0, 2), T, DEV, capacity_rows=6 * EL, capacity_traj=3, evict="oldest", **KW)
    acc = tr.env.acc.clone()
    with pytest.raises(ValueError, match="larger than the store"):
        tr.collect_targets(gr, gc, sample=True, seed=3, into=tiny)
    assert torch.equal(tr.env.acc, acc) and (tiny.version, tiny.n_traj, tiny.n_evicted) == (0, 2, 0)


# ---- 5. checkpoints -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["cost_sample", "weights", "start_sampling"])
def test_a_sequence_store_round_trip(mode, tmp_path):
    """150 rows, 20 slots.  A: 12 trajectories, then two appends -- the first evicts 4 for their slots, the second lands
    at row 0 and evicts 12 -- saved, then a third append (lands at row 67 behind the second chunk, evicts 12).  B: built
    from other data, loads the file, takes the same third append."""
    from osrl_amd.common.checkpoint import load_store, save_store
    from osrl_amd.common.replay import SequenceStore
    caps = dict(capacity_rows=150, capacity_traj=20, evict="oldest", **KW, **MODES[mode])
    tr = Tracker(_episodes(1), 12, 150, 20)
    w = lambda lo: dict(weights=tr.weights(range(lo, lo + 12))) if mode == "weights" else {}  # noqa: E731
    a = SequenceStore.from_dataset(_episodes(1), T, DEV, **caps)
    _install(a, mode, tr.weights(), None)
    for i, seed in enumerate((2, 3), 1):
        a.append(_episodes(seed), **w(12 * i))
        tr.append(_episodes(seed))
    assert (a.n_evicted, a.tail) == (tr.evicted, tr.m.tail) == (16, 67)
    path = str(tmp_path / "seq.pt")
    save_store(a, path)
    b = SequenceStore.from_dataset(_episodes(9), T, DEV, **caps)
    _install(b, mode, np.arange(1.0, 13.0), None)
    b.append(_episodes(8), **(dict(weights=np.ones(12)) if mode == "weights" else {}))
    ptrs, v = [t.data_ptr() for t in _tables(b)], b.version
    sd = load_store(b, path)
    assert all(t.device.type == "cpu" for t in sd["tables"].values())
    assert [t.data_ptr() for t in _tables(b)] == ptrs and b.version == v + 1
    _same_windows(*_windows((a, b), 2), f"{mode}: after the load")
    for s in (a, b):
        s.append(_episodes(4), **w(36))
    tr.append(_episodes(4))
    _same_windows(*_windows((a, b), 4), f"{mode}: after the third append")
    for s in (a, b):
        assert (s.n_traj, s.n_rows, s.tail, s.n_evicted, s.n_appended, s.n_original, s.n_augmented) == \
            (len(tr.m.age), sum(n for _, n in tr.m.live()), tr.m.tail, tr.evicted, 36, 12, 0)
        assert list(zip(s._mirror[0].tolist(), s._mirror[1].tolist())) == tr.m.live()
        assert int(s._live.item()) == s.n_traj
    assert tr.evicted == 28 and tr.m.tail == 134
    for x, y in zip(_tables(a), _tables(b)):
        assert torch.equal(x, y)
    _check(b, tr, mode, None, "the loaded store against its survivors", steps=2)


def test_sequence_store_refusals(tmp_path):
    from osrl_amd.common.replay import SequenceStore
    d0 = _episodes(1)
    caps = dict(capacity_rows=150, capacity_traj=20, evict="oldest", **KW)
    a = SequenceStore.from_dataset(d0, T, DEV, **caps)
    sd = a.state_dict()
    with pytest.raises(ValueError, match="affine"):
        SequenceStore.from_dataset(d0, T, DEV, cost_sample=True, cost_transform=lambda x: 70 - x, **caps).state_dict()
    fixed = SequenceStore.from_dataset(d0, T, DEV, **KW)
    with pytest.raises(ValueError, match="fixed"):
        fixed.state_dict()
    with pytest.raises(ValueError, match="fixed"):
        fixed.load_state_dict(sd)
    for kw, word in ((dict(capacity_rows=151), "capacity_rows"), (dict(capacity_traj=21), "capacity_traj"),
                     (dict(evict=None), "evict"), (dict(reward_scale=1.0), "reward_scale"),
                     (dict(cost_scale=1.0), "cost_scale")):
        other = SequenceStore.from_dataset(d0, T, DEV, **dict(caps, **kw))
        with pytest.raises(ValueError, match=word):
            other.load_state_dict(sd)
        assert other.version == 0
    with pytest.raises(ValueError, match="seq_len"):
        SequenceStore.from_dataset(d0, T + 1, DEV, **caps).load_state_dict(sd)
    wide = dict(d0, observations=np.concatenate([d0["observations"], d0["observations"][:, :1]], 1))
    with pytest.raises(ValueError, match="observations"):
        SequenceStore.from_dataset(wide, T, DEV, **caps).load_state_dict(sd)
    # a frontier travels as its tensors; a store that does not evict is saved too
    g = SequenceStore.from_dataset(d0, T, DEV, capacity_rows=150, capacity_traj=30, **KW)
    g.enable_pf_sampling(beta=0.7, frontier=_frontier())
    h = SequenceStore.from_dataset(_episodes(9), T, DEV, capacity_rows=150, capacity_traj=30, **KW)
    h.load_state_dict(g.state_dict())
    for s in (g, h):
        s.append(_episodes(2))
    assert h.tail is None and h.n_rows == 2 * sum(LENS) and torch.equal(g.cdf, h.cdf)
    _same_windows(*_windows((g, h), 3), "pf, growing store")


def test_a_replay_store_round_trip_across_a_wrapped_ring(tmp_path):
    from osrl_amd.common.checkpoint import load_store, save_store
    from replay_weighted_util import make_weights
    cap = 64
    a = _store(_data(50, 1), capacity=cap, state_init=True, sample_prob=make_weights(50, seed=1))
    a.append(_data(30, 2), sample_prob=make_weights(30, seed=2))  # wraps: cursor 16
    assert a._cursor == 16 and a.n_rows == cap
    path = str(tmp_path / "replay.pt")
    save_store(a, path)
    b = _store(_data(40, 9), capacity=cap, state_init=True)  # uniform: the load switches it to weighted
    ptrs, epoch = [t.data_ptr() for t in b.tables], b.sample_epoch
    load_store(b, path)
    assert b.weighted and b.sample_epoch == epoch + 1 and [t.data_ptr() for t in b.tables] == ptrs
    assert (b.n_rows, b._cursor, int(b._live.item())) == (cap, 16, cap)
    _same_draws(*_draws((a, b), 3, fields=7), "after the load")
    for s in (a, b):
        s.append(_data(10, 3), sample_prob=make_weights(10, seed=3))
    for x, y in zip(a.tables + [a._w64, a.cum], b.tables + [b._w64, b.cum]):
        assert torch.equal(x, y)
    _same_draws(*_draws((a, b), 4, fields=7), "after the append")
    assert b.get_dataset_states()[0] == a.get_dataset_states()[0]
    np.testing.assert_array_equal(b.observations_std, a.observations_std)
