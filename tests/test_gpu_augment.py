"""Pareto-frontier augmentation on device (csrc/augment.hip, common/ingest.py, SequenceStore.from_dataset) against
the reference's own outputs (tests/golden/augment.npz) with its recorded draws injected, against the numpy
restatement (tests/augment_oracle.py) at scale, and for determinism across runs and data-parallel ranks."""
import numpy as np
import pytest
import torch

from augment_cases import BC_COST_LIMIT, BC_KINDS, SEQ_CASES, make_augment_dataset, make_bc_frontier_dataset
import augment_oracle as AO
from oracle import ingest_oracle as IO
from oracle_util import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLES = ("observations", "actions", "rewards", "costs", "returns", "cost_returns")


def _np(t):
    return t.detach().cpu().numpy()


def golden_draws(g, name):
    return {k: g[f"{name}_{k}"] for k in ("pick", "u_rew", "u_part", "u_cr", "noise_c", "noise_r")
            if f"{name}_{k}" in g.files}


def store_tables(st):
    return dict(observations=st.obs, actions=st.act, rewards=None, costs=st.cost, returns=st.ret,
                cost_returns=st.cret)


def check_against_golden(g, name, st, n_rows):
    assert st.n_original == int(g[f"{name}_n_original"])
    assert np.array_equal(_np(st.traj_len), g[f"{name}_len"])
    assert np.array_equal(_np(st.traj_start), np.concatenate([[0], np.cumsum(g[f"{name}_len"])[:-1]]))
    for k, t in (("observations", st.obs), ("actions", st.act), ("costs", st.cost)):
        got = _np(t)[n_rows:]
        assert np.array_equal(got, g[f"{name}_aug_{k}"].reshape(got.shape)), k  # copied bit for bit
    for k, t in (("returns", st.ret), ("cost_returns", st.cret)):
        np.testing.assert_array_max_ulp(_np(t)[n_rows:], g[f"{name}_aug_{k}"], maxulp=1)


@pytest.mark.parametrize("name", [n for n, (_, kw) in SEQ_CASES.items() if "random_aug" not in kw and
                                  not kw.get("pf_only")])
def test_augmentation_matches_reference_golden(name):
    from osrl_amd.common.ingest import compute_cost_sample_prob, process_sequence_dataset
    from osrl_amd.common.replay import SequenceStore
    g = load_golden("augment")
    dkw, skw = SEQ_CASES[name]
    data = make_augment_dataset(**dkw)
    n_rows = int(process_sequence_dataset(data, False, DEV)["returns"].shape[0])
    st = SequenceStore.from_dataset(data, 10, DEV, cost_sample=True, draws=golden_draws(g, name), **skw)
    info = st.aug_info
    assert np.array_equal(st.indices, g[f"{name}_indices"])
    assert np.array_equal(st.idx, g[f"{name}_idx"])  # nearest + partner lists, exact
    assert np.array_equal(np.sort(_np(info["frontier"].pareto_idx)), g[f"{name}_pareto"])
    np.testing.assert_allclose(st.pareto_frontier.coeffs, g[f"{name}_coef"], rtol=1e-9, atol=0)
    assert st.n_augmented == len(g[f"{name}_len"]) - st.n_original
    check_against_golden(g, name, st, n_rows)
    tb = dict(cost_returns=st.cret, traj_start=st.traj_start)
    np.testing.assert_allclose(_np(compute_cost_sample_prob(tb, ("affine", -1.0, 50.0))), g[f"{name}_prob50"],
                               rtol=2e-6, atol=1e-9)
    assert st.cdf is not None and abs(float(st.cdf[-1]) - 1.0) < 1e-6
    c = np.linspace(5.0, 60.0, 7)
    np.testing.assert_allclose(st.compute_pareto_return(c), np.poly1d(g[f"{name}_coef"])(c), rtol=1e-8, atol=1e-6)


def test_random_augmentation_matches_reference_golden():
    from osrl_amd.common.ingest import process_sequence_dataset
    from osrl_amd.common.replay import SequenceStore
    g = load_golden("augment")
    dkw, skw = SEQ_CASES["rand_aug"]
    data = make_augment_dataset(**dkw)
    n_rows = int(process_sequence_dataset(data, False, DEV)["returns"].shape[0])
    st = SequenceStore.from_dataset(data, 10, DEV, draws=golden_draws(g, "rand_aug"), **skw)
    assert np.array_equal(st.idx, g["rand_aug_idx"])
    assert st.pareto_frontier is None
    check_against_golden(g, "rand_aug", st, n_rows)


def test_pf_only_suppresses_augmentation_and_pf_sample_raises():
    from osrl_amd.common.replay import SequenceStore
    g = load_golden("augment")
    dkw, skw = SEQ_CASES["pf_only"]
    st = SequenceStore.from_dataset(make_augment_dataset(**dkw), 10, DEV, **skw)
    assert st.n_augmented == 0 and st.n_traj == int(g["pf_only_n_original"])
    assert np.array_equal(_np(st.traj_len), g["pf_only_len"])
    with pytest.raises(NotImplementedError, match="pf_sample"):
        SequenceStore.from_dataset(make_augment_dataset(), 10, DEV, augment_percent=0.2, pf_sample=True)


def test_augmentation_defaults_keep_plain_ingestion():
    from osrl_amd.common.replay import SequenceStore
    data = make_augment_dataset(seed=9)
    a = SequenceStore.from_dataset(data, 10, DEV, cost_sample=True)
    b = SequenceStore.from_dataset(data, 10, DEV, cost_sample=True, deg=3, augment_percent=0, random_aug=0)
    for x, y in ((a.obs, b.obs), (a.ret, b.ret), (a.cret, b.cret), (a.traj_len, b.traj_len), (a.cdf, b.cdf)):
        assert torch.equal(x, y)
    assert a.n_augmented == 0 and a.idx is None and a.pareto_frontier is None


@pytest.mark.parametrize("kind", BC_KINDS)
def test_bc_frontier_matches_reference_golden(kind):
    from osrl_amd.common.ingest import process_bc_dataset
    g = load_golden("augment")
    for gamma in (1.0, 0.99):
        out = process_bc_dataset(make_bc_frontier_dataset(kind), BC_COST_LIMIT, gamma, "frontier", DEV)
        tag = f"bc_{kind}_{gamma}"
        assert np.array_equal(_np(out["index"]), g[f"{tag}_index"]), tag
        for k in ("observations", "cost_returns", "rew_returns"):
            assert np.array_equal(_np(out[k]), g[f"{tag}_{k}"]), (tag, k)


def test_bad_inputs_raise_value_error():
    from osrl_amd.common.ingest import augmentation, process_sequence_dataset
    data = make_augment_dataset(seed=3, n_traj=200)
    data["costs"][:] = 0.0  # every cost return equal: a zero-width cost bin
    with pytest.raises(ValueError):
        augmentation(process_sequence_dataset(data, False, DEV), augment_percent=0.2)


def test_seeded_tables_are_deterministic_and_rank_independent():
    from osrl_amd.common.replay import SequenceStore
    data = make_augment_dataset(seed=11)
    mk = lambda rank, seed=5, **kw: SequenceStore.from_dataset(data, 10, DEV, augment_percent=0.3, seed=seed,  # noqa
                                                               rank=rank, cost_sample=True, **kw)
    a, b, c = mk(0), mk(0), mk(1)
    for s in (b, c):
        for x, y in ((a.obs, s.obs), (a.act, s.act), (a.ret, s.ret), (a.cret, s.cret), (a.cost, s.cost),
                     (a.traj_start, s.traj_start), (a.traj_len, s.traj_len), (a.cdf, s.cdf)):
            assert torch.equal(x, y)
    assert a.n_augmented > 0 and np.unique(a.idx).size < a.idx.size  # partner draws ran
    d = mk(0, seed=6)
    assert not torch.equal(a.ret, d.ret) if a.ret.shape == d.ret.shape else True
    r1, r2 = (SequenceStore.from_dataset(data, 10, DEV, random_aug=0.2, aug_cmax=75, seed=4, rank=r) for r in (0, 1))
    assert torch.equal(r1.ret, r2.ret) and torch.equal(r1.cret, r2.cret)


def _flat(trajs):
    out = {k: np.concatenate([t[k] for t in trajs]) for k in TABLES}
    lens = np.array([len(t["costs"]) for t in trajs], np.int64)
    out["traj_len"], out["traj_start"] = lens, np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return out


def test_large_dataset_matches_restatement():
    """~1 M transitions, injected draws from a fixed numpy stream, against tests/augment_oracle.py."""
    from osrl_amd.common.ingest import augmentation, process_sequence_dataset, random_augmentation
    data = make_augment_dataset(seed=21, n_traj=4000, max_len=500, od=4)
    assert data["rewards"].shape[0] > 900_000
    tb = process_sequence_dataset(data, False, DEV)
    ref_t = _flat(IO.process_sequence_dataset(data, False))
    rs = np.random.RandomState(3)
    draws = dict(pick=np.tile(np.arange(10, dtype=np.int32)[::-1], 600), u_rew=rs.uniform(size=6000),
                 u_part=rs.uniform(size=6000))
    out, info = augmentation(tb, deg=3, augment_percent=0.4, min_reward=5, draws=draws)
    want, winfo = AO.augmentation(ref_t, deg=3, augment_percent=0.4, min_reward=5, draws=draws)
    assert np.array_equal(_np(info["indices"]), winfo["indices"])
    assert np.array_equal(_np(info["idx"]), winfo["idx"])
    np.testing.assert_allclose(_np(info["frontier"].coef_dev[:4]), winfo["coef"], rtol=1e-9)
    n = ref_t["returns"].shape[0]
    for k in TABLES:
        if k in ("returns", "cost_returns"):
            np.testing.assert_array_max_ulp(_np(out[k]), want[k], maxulp=1)
        else:
            assert np.array_equal(_np(out[k]), want[k]), k
    assert np.array_equal(_np(out["traj_len"]), want["traj_len"])
    assert out["returns"].shape[0] > n
    S = int(0.1 * ref_t["traj_len"].shape[0])
    rows = int(ref_t["traj_len"].max()) * S
    rd = dict(u_cr=rs.uniform(size=2 * S), noise_c=rs.normal(0, 0.2, rows), noise_r=rs.normal(0, 1.0, rows))
    out, info = random_augmentation(tb, 0.1, 0, 600, 5, 75, 5, 1.0, 0.2, draws=rd)
    want, winfo = AO.random_augmentation(ref_t, 0.1, 0, 600, 5, 75, 5, draws=rd)
    assert np.array_equal(_np(info["idx"]), winfo["idx"])
    for k in ("returns", "cost_returns"):
        np.testing.assert_array_max_ulp(_np(out[k]), want[k], maxulp=1)


def test_windows_from_augmented_trajectories_match_oracle():
    from oracle.osrl_oracle import prepare_sequence_sample
    from osrl_amd.common.replay import SequenceStore
    from osrl_amd.engine.core import StepState
    g = load_golden("augment")
    dkw, skw = SEQ_CASES["d3_p20"]
    T, RS, CS = 10, 0.1, 2.0
    st = SequenceStore.from_dataset(make_augment_dataset(**dkw), T, DEV, reward_scale=RS, cost_scale=CS,
                                    draws=golden_draws(g, "d3_p20"), **skw)
    # the reference's trajectories: process_sequence_dataset's, then its augmented copies (the golden)
    trajs = IO.process_sequence_dataset(make_augment_dataset(**dkw), False)
    ln = _np(st.traj_len)
    off = np.concatenate([[0], np.cumsum(g["d3_p20_len"][st.n_original:])])
    for a in range(len(off) - 1):
        trajs.append({k: g[f"d3_p20_aug_{k}"][off[a]:off[a + 1]] for k in TABLES})
    assert len(trajs) == st.n_traj
    picks = [(t, p) for t in range(st.n_original, st.n_traj, 7) for p in {0, int(ln[t]) - 1}]
    B = len(picks)
    idx_in = torch.tensor(picks, dtype=torch.int32, device=DEV)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    bufs = [z(B, T, st.od), z(B, T, st.ad), z(B, T), z(B, T), z(B, T, dt=torch.int64), z(B, T), z(B), z(B, T)]
    sst = StepState(DEV, ["x"])
    st.gather(*bufs, sst.ptr, idx_in=idx_in)
    torch.cuda.synchronize()
    for b, (t, p) in enumerate(picks):
        want = prepare_sequence_sample(trajs[t], p, T, RS, CS)
        for got, w in zip(bufs, want):
            np.testing.assert_allclose(_np(got[b]).astype(np.float64), np.asarray(w, np.float64), rtol=1e-6, atol=1e-6)



def test_bc_frontier_needs_complete_episodes():
    """Transitions after the last done flag belong to no episode: the reference compares their zero returns with the
    frontier at cost 0, so "frontier" refuses such a dataset; cut at the last done flag it matches the restatement."""
    from cases import make_ingest_dataset
    from osrl_amd.common.ingest import process_bc_dataset
    data = make_ingest_dataset()
    with pytest.raises(NotImplementedError, match="complete episode"):
        process_bc_dataset(data, 6.0, 1.0, "frontier", DEV)
    st, ln = IO.episode_segments(IO.done_flags(data))
    n = int(st[-1] + ln[-1])
    cut = {k: v[:n] for k, v in data.items()}
    for gamma in (1.0, 0.99):
        out = process_bc_dataset(cut, 6.0, gamma, "frontier", DEV)
        cs = [IO.discounted_cumsum(cut["costs"][s:s + m], gamma)[0] for s, m in zip(st, ln)]
        rs_ = [IO.discounted_cumsum(cut["rewards"][s:s + m], gamma)[0] for s, m in zip(st, ln)]
        cr, rr = np.zeros_like(cut["costs"]), np.zeros_like(cut["rewards"])
        for s, m, c, r in zip(st, ln, cs, rs_):
            cr[s:s + m], rr[s:s + m] = c, r
        with np.errstate(all="ignore"):
            keep, _ = AO.bc_frontier(cs, rs_, cr, rr)
        assert np.array_equal(_np(out["index"]), np.flatnonzero(keep)), gamma
        assert np.array_equal(_np(out["observations"]), cut["observations"][keep])
