"""Stores that grow (ReplayStore(capacity=) / append, SequenceStore capacities / append, collect(into=); include/osrl_amd.h
osrl_replay_gather_n / osrl_step_begin_peer_n / osrl_seq_gather_t.n_traj_dev): a captured step follows a store that was
appended to, with the graph it already has.  Every comparison is exact: a draw is a pure function of (seed, step, row,
live count, table), so a grown store draws what a fixed store with the same live rows draws, and an engine that kept its
graph over an append ends where an engine that re-attached a freshly built store ends, bit for bit.  The reference has
no counterpart (its datasets are fixed, osrl/common/dataset.py:790-847).

Shapes: od 5, ad 2, hidden [32, 32], B 32; the BC one-launch step is built for hidden layers of 129..448 columns, so that
case runs [256, 256], and the [32, 32] case runs BC's six-launch plan, whose fused prologue draws the minibatch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from replay_weighted_util import make_weights  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OD, AD, HID, B = 5, 2, [32, 32], 32
RS, CS = 0.5, 2.0
KEYS = ("observations", "next_observations", "actions", "rewards", "costs")


def _data(n, seed, od=OD, ad=AD):
    from osrl_amd.common.replay import synthetic_transitions
    d = synthetic_transitions(n, od, ad, seed=seed)
    d["timeouts"] = (np.arange(n) % 9 == 8).astype(np.float32)
    return d


def _cat(a, b):
    return {k: np.concatenate([a[k], b[k]]) for k in a}


def _done(d):
    return np.logical_or(d["terminals"] == 1, d["timeouts"] == 1).astype(np.float32)


def _store(d, **kw):
    from osrl_amd.common.replay import ReplayStore
    kw.setdefault("seed", 7)
    return ReplayStore(d, DEV, reward_scale=RS, cost_scale=CS, **kw)


def _bufs(store, rows=B, n=None):
    return [torch.full((rows, w), -7.0, device=DEV) for w in store.widths[:n]]


def _draws(stores, steps, rows=B, first_step=0, fields=6):
    """``gather(idx_out=)`` of every store at steps first_step + 1 ... : per store a list of (idx, [batch buffers])."""
    from osrl_amd.engine.core import StepState
    st = StepState(DEV, ["x"])
    st.set_step(first_step)
    out = [[] for _ in stores]
    for _ in range(steps):
        st.tick()
        for o, s in zip(out, stores):
            dst, idx = _bufs(s, rows), torch.full((rows,), -1, dtype=torch.int32, device=DEV)
            s.gather(dst, st.ptr, idx_out=idx)
            o.append((idx.cpu().numpy(), [t.cpu().numpy() for t in dst[:fields]]))
    torch.cuda.synchronize()
    return out


def _same_draws(a, b, what):
    assert len(a) == len(b)
    for s, ((ia, da), (ib, db)) in enumerate(zip(a, b), 1):
        np.testing.assert_array_equal(ia, ib, err_msg=f"{what}: indices of step {s}")
        for f, (x, y) in enumerate(zip(da, db)):
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: field {f} of step {s}")


def _cum(store, n):
    torch.cuda.synchronize()
    return store.cum.cpu().numpy().view(np.uint64)[:n]


# ---- 1. the same store ---------------------------------------------------------------------------------------------------
def test_a_capacity_store_draws_what_the_fixed_store_draws():
    from osrl_amd.engine.core import StepState
    d = _data(300, 3)
    grown, fixed = _store(d, capacity=512), _store(d)
    assert grown.capacity == 512 and grown.n_rows == fixed.n_rows == 300 and fixed.capacity is None
    assert grown.tables[0].shape == (512, OD) and not grown.tables[0][300:].any() and grown.live(0).shape == (300, OD)
    assert int(grown._live.item()) == 300
    a, b = _draws((grown, fixed), 4)
    _same_draws(a, b, "uniform")
    assert max(int(i.max()) for i, _ in a) < 300
    # the fused prologue and the two-table gather read the same word
    sa, sb = StepState(DEV, ["x"]), StepState(DEV, ["x"])
    for _ in range(2):
        da, db, fa, fb = _bufs(grown), _bufs(fixed), _bufs(grown, n=2), _bufs(fixed, n=2)
        sa.begin(None, 0, 0, grown.gather_args(da))
        sb.begin(None, 0, 0, fixed.gather_args(db))
        grown.gather_fields((0, 1), fa, sa.ptr)
        fixed.gather_fields((0, 1), fb, sb.ptr)
        torch.cuda.synchronize()
        for x, y in zip(da + fa, db + fb):
            np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
    w = make_weights(300, seed=2)
    grown.set_sample_prob(w)
    fixed.set_sample_prob(w)
    assert grown.cum.shape == (512,) and fixed.cum.shape == (300,)
    np.testing.assert_array_equal(_cum(grown, 300), _cum(fixed, 300))
    a, b = _draws((grown, fixed), 4)
    _same_draws(a, b, "weighted")
    assert all((w[i] > 0).all() for i, _ in a)


# ---- 2. growth without recapture -----------------------------------------------------------------------------------------
def _engine(kind):
    """(model, engine) of one of the paths that draw a minibatch, from fixed seeds: two calls give identical twins."""
    from osrl_amd.algorithms import BC, CPQ, FQE, BCTrainer, CPQTrainer, FQETrainer
    from osrl_amd.common.logger import DummyLogger
    torch.manual_seed(3)
    if kind in ("bc_one_launch", "bc_plan"):
        m = BC(OD, AD, 1.0, [256, 256] if kind == "bc_one_launch" else HID, 50, device=DEV)
        BCTrainer(m, None, DummyLogger(), actor_lr=1e-3, device=DEV, stats_mode="none")
        eng = m.engine(B)
        if kind == "bc_one_launch":
            assert eng.one_launch, "the shape should take the one-launch step"
        else:
            eng.one_launch = False  # (the six-launch plan: the fused prologue draws the minibatch)
    elif kind in ("cpq_step", "cpq_pipe"):
        m = CPQ(OD, AD, 1.0, HID, HID, 32, 2, device=DEV)
        CPQTrainer(m, None, DummyLogger(), 1e-3, 1e-3, 1e-3, 1e-3, device=DEV, stats_mode="none", use_graph=True)
        eng = m.engine(B)
    else:
        pol = BC(OD, AD, 1.0, [16, 12], 50, device=DEV)
        torch.manual_seed(11)
        m = FQE(pol, HID, gamma=0.9, tau=0.05, num_q=2, device=DEV)
        FQETrainer(m, critic_lr=1e-3, reward_scale=RS, cost_scale=CS, stats_mode="none")
        eng = m.engine(B)
        eng._policy = pol
    return m, eng


def _run(eng, kind, n):
    if kind == "cpq_pipe":
        eng.steps_replay(n, steps_per_graph=2)
    else:
        for _ in range(n):
            eng.step_replay()
    torch.cuda.synchronize()


def _graphs(eng, kind):
    """The captured objects a re-attachment would have dropped."""
    if kind == "bc_one_launch":  # (launched directly: its descriptor lives in the argument arena instead of a graph)
        return (eng._arena_direct,)
    if kind == "cpq_pipe":
        return (eng._pipe, eng._pipe.graph)
    return (eng.graph,)


@pytest.mark.parametrize("kind", ["bc_one_launch", "bc_plan", "cpq_step", "cpq_pipe", "fqe"])
def test_an_engine_follows_an_append_with_the_graph_it_has(kind):
    """A: a capacity store of 200 rows, n steps, append 150 rows, n more steps, nothing re-attached.  B: the same model
    and seed on fixed stores -- 200 rows for n steps, then ``attach_replay`` of the fixed 350-row store (which drops and
    recaptures everything) and n more.  Parameters, Adam moments, targets, packed copies and the statistics of every
    step are bit-equal; A holds the graph objects it had before the append; and the draws after the append reach the new
    rows (96 or more draws over 350 rows miss rows >= 200 with probability (200 / 350)^96 < 1e-23; they are
    deterministic given the seed)."""
    from test_gpu_pipeline import _state
    n = 4 if kind == "cpq_pipe" else 3
    d0, d1 = _data(200, 3), _data(150, 4)
    ma, ea = _engine(kind)
    grown = _store(d0, capacity=512, seed=11)
    ea.attach_replay(grown)
    _run(ea, kind, n)
    held = _graphs(ea, kind)
    assert all(g is not None for g in held)
    grown.append(d1)
    assert grown.n_rows == 350 and grown.version == 1
    _run(ea, kind, n)
    assert all(x is y for x, y in zip(_graphs(ea, kind), held)), "the append dropped what was captured"
    if kind == "bc_one_launch":
        assert ea.one_launch and ea._arena_direct.misses == 0

    mb, eb = _engine(kind)
    eb.attach_replay(_store(d0, seed=11))
    _run(eb, kind, n)
    fixed = _store(_cat(d0, d1), seed=11)
    eb.attach_replay(fixed)
    _run(eb, kind, n)
    assert ea.st.device_step() == eb.st.device_step() == 2 * n
    sa, sb = _state(ma, ea), _state(mb, eb)
    assert set(sa) == set(sb)
    for k in sa:
        np.testing.assert_array_equal(sa[k].cpu().numpy(), sb[k].cpu().numpy(), err_msg=f"{kind}: {k}")
    for s in range(1, 2 * n + 1):
        ra, rb = ea.st.read_stats(s), eb.st.read_stats(s)
        assert ra.keys() == rb.keys()
        np.testing.assert_array_equal(np.array(list(ra.values())), np.array(list(rb.values())),
                                      err_msg=f"{kind}: statistics of step {s}")
    # the rows those steps drew (steps n + 1 .. 2 n of a 350-row store): some lie past the original 200 ...
    drawn = _draws((fixed,), n, first_step=n)[0]
    assert max(int(i.max()) for i, _ in drawn) >= 200
    # ... and the last step's minibatch, still in A's buffers, is exactly those rows (the twin engine holds it when the
    # pipelined graph ran an even number of steps)
    last = ea._pipe.e[1] if kind == "cpq_pipe" else ea
    np.testing.assert_array_equal(last.obs.cpu().numpy(), drawn[-1][1][0])
    np.testing.assert_array_equal(last.act.cpu().numpy(), drawn[-1][1][2])


# ---- 3. the ring ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_a_full_store_overwrites_its_oldest_rows(weighted):
    cap, n0, m = 256, 200, 100
    d0, d1 = _data(n0, 3), _data(m, 4)
    w0, w1 = make_weights(n0, seed=1), make_weights(m, seed=2)
    s = _store(d0, capacity=cap, state_init=True, sample_prob=w0 if weighted else None)
    ptrs = [t.data_ptr() for t in s.tables]
    if weighted:
        with pytest.raises(ValueError):
            s.append(d1)
        s.append({k: torch.as_tensor(v, device=DEV) for k, v in d1.items()}, sample_prob=w1)  # (device tensors)
    else:
        s.append(d1)
    assert s.n_rows == cap and s.version == 1 and int(s._live.item()) == cap and [t.data_ptr() for t in s.tables] == ptrs
    cols = lambda d: [d[k].reshape(len(d["rewards"]), -1) for k in KEYS] + \
        [_done(d)[:, None], np.concatenate([[1.0], _done(d)[:-1]]).astype(np.float32)[:, None]]  # noqa: E731
    ring = [np.zeros((cap, w), np.float32) for w in s.widths]
    wring = np.zeros(cap)
    for r, c in zip(ring, cols(d0)):
        r[:n0] = c
    wring[:n0] = w0
    for i in range(m):
        for r, c in zip(ring, cols(d1)):
            r[(n0 + i) % cap] = c[i]
        wring[(n0 + i) % cap] = w1[i]
    for i, r in enumerate(ring):
        np.testing.assert_array_equal(s.tables[i].cpu().numpy(), r, err_msg=f"table {i}")
    phys = dict(zip(KEYS, ring[:5]), done=ring[5])
    plain = _store(phys, sample_prob=wring if weighted else None)
    if weighted:
        np.testing.assert_array_equal(_cum(s, cap), _cum(plain, cap))
    a, b = _draws((s, plain), 4, fields=7)
    for (ia, da), (ib, db) in zip(a, b):
        np.testing.assert_array_equal(ia, ib)
        for x, y in zip(da[:6], db):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(da[6], ring[6][ia])
        assert not weighted or (wring[ia] > 0).all()
    if not weighted:  # 128 uniform draws over 256 rows miss the 44 wrapped rows with probability (212 / 256)^128 < 1e-10
        assert min(int(i.min()) for i, _ in a) < (n0 + m) % cap


# ---- 4. the clamp --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("word", [0, -3, 64 + 5, 2 ** 40])
def test_whatever_the_live_word_holds_the_index_stays_inside_the_allocation(word, weighted):
    """The word is set behind the store's back; column 0 of the observations holds the row number, so the rows the fused
    prologue gathered (it has no index output) can be read off as well."""
    from osrl_amd.engine.core import StepState
    cap, rows = 64, 256
    d = _data(40, 3)
    d["observations"][:, 0] = np.arange(40)
    s = _store(d, capacity=cap, sample_prob=make_weights(40, seed=4) if weighted else None)
    s.tables[0][:, 0] = torch.arange(cap, device=DEV, dtype=torch.float32)
    s._live.fill_(word)
    idx = _draws((s,), 2, rows=rows)[0]
    st = StepState(DEV, ["x"])
    dst = _bufs(s, rows)
    st.begin(None, 0, 0, s.gather_args(dst))
    torch.cuda.synchronize()
    got = [i for i, _ in idx] + [dst[0][:, 0].cpu().numpy().astype(np.int64)]
    for i in got:
        assert i.min() >= 0 and i.max() < cap, (word, i.min(), i.max())
    if word < 1:  # one live row: row 0
        assert all((i == 0).all() for i in got)
    np.testing.assert_array_equal(got[0], got[2])  # (step 1 of both paths)


# ---- 5. sequences --------------------------------------------------------------------------------------------------------
LENS = (3, 4, 5, 6, 7, 8, 9, 3, 4, 5, 6, 7)
T = 4


def _episodes(seed):
    rs = np.random.RandomState(seed)
    n = sum(LENS)
    f = np.float32
    d = dict(observations=rs.randn(n, OD).astype(f), next_observations=rs.randn(n, OD).astype(f),
             actions=rs.uniform(-1, 1, (n, AD)).astype(f), rewards=rs.randn(n).astype(f),
             costs=(rs.uniform(size=n) < 0.3).astype(f), terminals=np.zeros(n, f), timeouts=np.zeros(n, f))
    d["timeouts"][np.cumsum(LENS) - 1] = 1
    return d


def _windows(stores, steps, rows=16):
    from osrl_amd.engine.core import StepState
    st = StepState(DEV, ["x"])
    out = [[] for _ in stores]
    for _ in range(steps):
        st.tick()
        for o, s in zip(out, stores):
            z = lambda *sh, dt=torch.float32: torch.full(sh, -7, dtype=dt, device=DEV)  # noqa: E731
            bufs = [z(rows, T, OD), z(rows, T, AD), z(rows, T), z(rows, T), z(rows, T, dt=torch.int64), z(rows, T),
                    z(rows), z(rows, T)]
            idx = z(rows, 2, dt=torch.int32)
            s.gather(*bufs, st.ptr, idx_out=idx)
            o.append([t.cpu().numpy() for t in bufs + [idx]])
    torch.cuda.synchronize()
    return out


def _same_windows(a, b, what):
    for s, (x, y) in enumerate(zip(a, b), 1):
        for f, (p, q) in enumerate(zip(x, y)):
            np.testing.assert_array_equal(p, q, err_msg=f"{what}: output {f} of step {s}")


SEQ_MODES = {"uniform": {}, "cost_sample": dict(cost_sample=True), "start_sampling": dict(start_sampling=True)}


@pytest.mark.parametrize("mode", sorted(SEQ_MODES))
def test_a_sequence_store_grows_to_the_store_of_the_concatenation(mode):
    from osrl_amd.common.replay import SequenceStore
    kw = dict(reward_scale=RS, cost_scale=CS, seed=3, **SEQ_MODES[mode])
    d0, d1 = _episodes(1), _episodes(2)
    n = sum(LENS)
    grown = SequenceStore.from_dataset(d0, T, DEV, capacity_rows=200, capacity_traj=40, **kw)
    fixed = SequenceStore.from_dataset(d0, T, DEV, **kw)
    assert (grown.n_traj, grown.n_rows, grown.capacity_traj, grown.capacity_rows) == (12, n, 40, 200)
    assert grown.obs.shape == (200, OD) and grown.traj_len.shape == (40,) and int(grown._live.item()) == 12
    _same_windows(*_windows((grown, fixed), 3), f"{mode}: before the append")
    ptrs = [t.data_ptr() for t in (grown.obs, grown.traj_start, grown.cdf, grown.start_cdf) if t is not None]
    grown.append(d1)
    both = SequenceStore.from_dataset(_cat(d0, d1), T, DEV, **kw)
    assert grown.n_traj == both.n_traj == 24 and grown.n_rows == 2 * n and grown.n_appended == 12 and grown.n_original == 12
    assert [t.data_ptr() for t in (grown.obs, grown.traj_start, grown.cdf, grown.start_cdf) if t is not None] == ptrs
    a, b = _windows((grown, both), 4)
    _same_windows(a, b, f"{mode}: after the append")
    assert max(int(x[-1][:, 0].max()) for x in a) >= 12  # (64 draws over 24 trajectories: the new ones are reached)


def test_a_chunk_that_does_not_fit_changes_nothing():
    from osrl_amd.common.replay import SequenceStore
    n = sum(LENS)
    d0, d1 = _episodes(1), _episodes(2)
    for caps in (dict(capacity_rows=n + 5, capacity_traj=40), dict(capacity_rows=200, capacity_traj=23)):
        s = SequenceStore.from_dataset(d0, T, DEV, cost_sample=True, **caps)
        before = [t.clone() for t in (s.obs, s.act, s.ret, s.cret, s.cost, s.traj_start, s.traj_len, s.cdf)]
        with pytest.raises(ValueError):
            s.append(d1)
        assert (s.n_traj, s.n_rows, s.n_appended, int(s._live.item())) == (12, n, 0, 12)
        for x, y in zip(before, (s.obs, s.act, s.ret, s.cret, s.cost, s.traj_start, s.traj_len, s.cdf)):
            assert torch.equal(x, y)
    with pytest.raises(ValueError):
        SequenceStore.from_dataset(d0, T, DEV).append(d1)  # a fixed store
    with pytest.raises(ValueError):
        SequenceStore.from_dataset(d0, T, DEV, capacity_rows=n - 1)
    s = SequenceStore.from_dataset(d0, T, DEV, capacity_rows=200, capacity_traj=40)
    s.set_sample_prob(np.arange(1.0, 13.0))
    with pytest.raises(ValueError):
        s.append(d1)  # explicit weights: the new trajectories need theirs
    s.append(d1, weights=np.arange(13.0, 25.0))
    both = SequenceStore.from_dataset(_cat(d0, d1), T, DEV)
    both.set_sample_prob(np.arange(1.0, 25.0))
    _same_windows(*_windows((s, both), 2), "explicit weights")


def test_the_cdt_step_follows_an_append_with_the_graph_it_has():
    """2 + 2 ``step_store`` calls around an append, on the graph captured before it, against the fixed-store run that
    re-attaches the store of the concatenation: the same windows, and bit-equal parameters, moments and statistics.
    ``time_emb=False``: the gradient of the time-step embedding is an fp32 atomic scatter (csrc/cdt.hip
    ``te_scatter_kernel``) whose order of additions differs from run to run wherever two windows of a batch share a time
    step, so with it two runs of the SAME store already differ in the last bit of those rows (seen here: 287 of 14192
    parameters, the 9 time steps' rows, by <= 3e-8).  The window sampler does not depend on it."""
    from osrl_amd.algorithms import CDT, CDTTrainer
    from osrl_amd.common.logger import DummyLogger
    from osrl_amd.common.replay import SequenceStore
    d0, d1 = _episodes(1), _episodes(2)
    kw = dict(reward_scale=RS, cost_scale=CS, seed=3)

    def engine():
        torch.manual_seed(0)
        m = CDT(OD, AD, 1.0, seq_len=T, episode_len=16, embedding_dim=32, num_layers=1, num_heads=2, time_emb=False,
                use_rew=True, use_cost=True, device=DEV)
        tr = CDTTrainer(m, None, DummyLogger(), learning_rate=1e-3, lr_warmup_steps=3, reward_scale=RS, cost_scale=CS,
                        device=DEV, stats_mode="none")
        return m, m.engine(8, tr.cfg)

    ma, ea = engine()
    grown = SequenceStore.from_dataset(d0, T, DEV, capacity_rows=200, capacity_traj=40, **kw)
    ea.attach_store(grown)
    ea.step_store()
    ea.step_store()
    g = ea.graph
    assert g is not None
    grown.append(d1)
    ea.step_store()
    ea.step_store()
    torch.cuda.synchronize()
    assert ea.graph is g
    mb, eb = engine()
    eb.attach_store(SequenceStore.from_dataset(d0, T, DEV, **kw))
    eb.step_store()
    eb.step_store()
    eb.attach_store(SequenceStore.from_dataset(_cat(d0, d1), T, DEV, **kw))
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


# ---- 6. collect(into=) ---------------------------------------------------------------------------------------------------
def test_collect_into_a_store():
    from osrl_amd.algorithms import BC, FQE, BCTrainer, FQETrainer
    from osrl_amd.common.logger import DummyLogger
    from osrl_amd.common.replay import ReplayStore
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv, VecSyntheticSafeEnv
    E, EL = 5, 7
    torch.manual_seed(0)
    m = BC(OD, AD, 1.0, HID, EL, device=DEV)
    tr = BCTrainer(m, None, DummyLogger(), actor_lr=1e-3, device=DEV)
    tr.env = VecSyntheticSafeEnv(SyntheticSafeEnv(OD, AD, 50, seed=3, init_noise=0.5), E, DEV, base_seed=100)
    first = tr.collect(0.3, seed=1)
    store = ReplayStore(first.dataset, DEV, state_init=True, capacity=128)
    assert store.n_rows == E * EL
    torch.manual_seed(11)
    fqe = FQE(m, HID, gamma=0.9, tau=0.05, num_q=2, device=DEV)
    ftr = FQETrainer(fqe, critic_lr=1e-3, stats_mode="none")
    assert ftr.estimate(store).n_init == E
    ref = tr.collect(0.3, gamma=0.9, seed=2)
    got = tr.collect(0.3, gamma=0.9, seed=2, into=store)
    assert got.dataset is None and ref.dataset is not None
    for name, x, y in zip(ref._fields[1:], ref[1:], got[1:]):
        np.testing.assert_array_equal(x, y, err_msg=name)
    assert store.n_rows == 2 * E * EL and int(store._live.item()) == 2 * E * EL and store.version == 1
    new = slice(E * EL, 2 * E * EL)
    d = {k: v.cpu().numpy() for k, v in ref.dataset.items()}
    for i, k in enumerate(KEYS):
        np.testing.assert_array_equal(store.tables[i][new].cpu().numpy(), d[k].reshape(E * EL, -1), err_msg=k)
    done = _done(d)
    np.testing.assert_array_equal(store.tables[5][new].reshape(-1).cpu().numpy(), done)
    np.testing.assert_array_equal(store.tables[6][new].reshape(-1).cpu().numpy(), np.concatenate([[1.0], done[:-1]]))
    assert ftr.estimate(store).n_init == 2 * E  # (the cached initial-state index follows the store's version)
    # a store of other widths (BC multi-task appends the cost return) is refused before the run
    wide = ReplayStore(_data(20, 1, od=OD + 1), DEV, capacity=128)
    disc = tr._collector[1].disc.clone()
    with pytest.raises(ValueError):
        tr.collect(0.3, seed=3, into=wide)
    with pytest.raises(ValueError):
        tr.collect(0.3, seed=3, into=ReplayStore(first.dataset, DEV))  # a fixed store
    assert wide.n_rows == 20 and torch.equal(disc, tr._collector[1].disc)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals():
    from osrl_amd.common.replay import ReplayStore
    d = _data(50, 1)
    with pytest.raises(ValueError):
        ReplayStore(d, DEV, capacity=49)
    with pytest.raises(ValueError):
        ReplayStore(d, DEV, capacity=100, rank=1, world=2)
    s = _store(d, capacity=100)
    with pytest.raises(ValueError):
        s.append(_data(5, 2, od=OD + 1))
    with pytest.raises(ValueError):
        s.append(_data(5, 2, ad=AD + 1))
    miss = _data(5, 2)
    del miss["costs"]
    with pytest.raises(ValueError):
        s.append(miss)
    miss = _data(5, 2)
    del miss["terminals"]
    with pytest.raises(ValueError):
        s.append(miss)
    sw = _store(d, capacity=100, sample_prob=np.ones(50))
    with pytest.raises(ValueError):
        sw.append(_data(5, 2))
    with pytest.raises(ValueError):
        sw.append(_data(5, 2), sample_prob=np.ones(4))
    with pytest.raises(ValueError):
        sw.append(_data(5, 2), sample_prob=-np.ones(5))
    with pytest.raises(ValueError):
        sw.set_sample_prob(np.ones(100))  # one weight per LIVE row
    assert s.n_rows == sw.n_rows == 50 and s.version == sw.version == 0
    sw.append(_data(5, 2), sample_prob=np.ones(5))
    sw.set_sample_prob(np.ones(55))
    assert sw.n_rows == 55
