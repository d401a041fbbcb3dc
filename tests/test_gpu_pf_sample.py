"""Frontier-distance trajectory sampling on device (csrc/pf_dist.h, csrc/augment.hip osrl_pf_sample_prob,
common.ingest.compute_sample_prob, SequenceStore.enable_pf_sampling / set_sample_prob) against the numpy restatement
(tests/pf_sample_oracle.py) and against the reference's recorded solves (tests/golden/pf_sample.npz).

Gates: prob rtol 2e-6 / atol 1e-9 (the project's gate for compute_cost_sample_prob), dist rtol 1e-7, |cdf[-1] - 1| <
1e-6; against the golden the CPU test's gates (tests/test_pf_sample_oracle_cpu.py, where the reference solver's path
dependence on ``d4_p20`` / ``single_pf`` is described).

One class of trajectories cannot meet a RELATIVE distance gate whatever computes them: a trajectory ON the fitted
curve (a Pareto point of a fit that interpolates: ``d2_p50`` fits 3 points with a parabola, ``d4_p20`` 5 with a
quartic).  Its true distance is 0, and what fp64 returns is the rounding error of evaluating p(x) - r (1e-13 at
deg 2, 1e-8 at deg 4 where Horner's terms reach 1e7), of which two correct evaluations at two neighbouring x share no
digit.  Measured on a host build of the kernel's solver: 1 trajectory of d2_p50 (dist 9e-13, relative difference
0.23) and 1 of d4_p20 (dist 9e-9, 0.83); none in the other cases or in 600 k synthetic ones.  For those trajectories
only -- distance below 4 x the textbook rounding bound of that evaluation, pf_sample_oracle.evaluation_noise -- the
gate is that bound, absolute, instead of 1e-7 relative; every other trajectory is held to rtol 1e-7.  4 x: p(x) - r
and, through the position of the root, x - c are each uncertain by one bound, on each of the two sides compared.
On the MI355X: d2_p50 3 trajectories on the curve, largest difference 8.0e-13 (bound 1.05e-11); d4_p20 1, 9.5e-10
(bound 2.5e-7); single_pf 3, 0; off the curve the largest relative difference is 2.0e-11 on the six cases and 9.1e-10
at 200 k trajectories (deg 7).
"""
import numpy as np
import pytest
import torch

import pf_sample_oracle as PO
from augment_cases import SEQ_CASES, make_augment_dataset
from oracle_util import load_golden
from pf_sample_oracle import EXACT_CASES, PATH_DEPENDENT, golden_case, outside

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PF_CASES = EXACT_CASES + tuple(sorted(PATH_DEPENDENT))


def _np(t):
    return t.detach().cpu().numpy()


def golden_draws(g, name):
    return {k: g[f"{name}_{k}"] for k in ("pick", "u_rew", "u_part") if f"{name}_{k}" in g.files}


def flat_tables(c, r):
    """One-row trajectories: the first (cost return, return) of trajectory i is row i."""
    n = len(c)
    return dict(returns=torch.as_tensor(np.asarray(r, np.float32), device=DEV),
                cost_returns=torch.as_tensor(np.asarray(c, np.float32), device=DEV),
                traj_start=torch.arange(n, dtype=torch.int64, device=DEV))


def frontier_of(coef):
    from osrl_amd.common.ingest import Frontier
    cf = torch.zeros(8, dtype=torch.float64, device=DEV)
    cf[:len(coef)] = torch.as_tensor(np.asarray(coef, np.float64), device=DEV)
    return Frontier(cf, torch.tensor([len(coef) - 1], dtype=torch.int32, device=DEV), None, None, None)


def check_dist(tag, got, coef, c, r):
    x, want = PO.solve(coef, c, r)
    noise = 4.0 * PO.evaluation_noise(coef, x, r)
    err = np.abs(got - want)
    on_curve = want <= noise
    rel = err / np.maximum(want, np.finfo(np.float64).tiny)
    print(tag, "dist: max rel err off the curve", rel[~on_curve].max(initial=0.0), "| trajectories on the curve",
          int(on_curve.sum()), "max err there", err[on_curve].max(initial=0.0), "bound", noise[on_curve].max(initial=0.0))
    assert np.all(err[~on_curve] <= 1e-7 * want[~on_curve])
    assert np.all(err[on_curve] <= noise[on_curve])
    assert on_curve.sum() <= len(np.atleast_1d(coef))  # an interpolating fit passes through at most deg + 1 points
    return want


def check_against_oracle(tag, tables, frontier, beta=1.0):
    from osrl_amd.common.ingest import compute_sample_prob
    prob, cdf, dist = compute_sample_prob(tables, frontier, beta, with_cdf=True, with_dist=True)
    coef = _np(frontier.coef_dev)[:frontier.deg + 1]
    c = _np(tables["cost_returns"][tables["traj_start"]]).astype(np.float64)
    r = _np(tables["returns"][tables["traj_start"]]).astype(np.float64)
    want = check_dist(tag, _np(dist), coef, c, r)
    w = 1.0 / (want + beta)
    np.testing.assert_allclose(_np(prob), w / w.sum(), rtol=2e-6, atol=1e-9)
    np.testing.assert_allclose(_np(cdf), np.cumsum(w) / w.sum(), rtol=0, atol=2e-6)
    assert abs(float(cdf[-1]) - 1.0) < 1e-6
    return prob, cdf, dist


def augmented_store(name, **kw):
    from osrl_amd.common.replay import SequenceStore
    dkw, skw = SEQ_CASES[name]
    return SequenceStore.from_dataset(make_augment_dataset(**dkw), 10, DEV, draws=golden_draws(load_golden("augment"), name),
                                      **skw, **kw)


@pytest.mark.parametrize("name", PF_CASES)
def test_device_matches_restatement_on_augmented_stores(name):
    st = augmented_store(name)
    tables = dict(returns=st.ret, cost_returns=st.cret, traj_start=st.traj_start)
    _, cdf, _ = check_against_oracle(name, tables, st.aug_info["frontier"])
    st.enable_pf_sampling()
    assert torch.equal(st.cdf, cdf)


@pytest.mark.parametrize("deg", [3, 5, 7])
def test_device_matches_restatement_at_200k_trajectories(deg):
    rs = np.random.RandomState(40 + deg)
    xs = np.linspace(0.0, 80.0, 40)
    coef = np.polyfit(xs, 100.0 + 7.0 * xs + 30.0 * np.sin(xs / 9.0) + rs.normal(0.0, 8.0, 40), deg)
    n = 200_000
    tables = flat_tables(rs.uniform(0.0, 80.0, n), rs.uniform(0.0, 700.0, n))
    check_against_oracle(f"synthetic deg {deg}", tables, frontier_of(coef))


@pytest.mark.parametrize("name", PF_CASES)
def test_device_matches_reference_golden(name):
    from osrl_amd.common.ingest import compute_sample_prob
    g = load_golden("pf_sample")
    coef, c, r = golden_case(g, name)
    prob, dist = compute_sample_prob(flat_tables(c, r), frontier_of(coef), 1.0, with_dist=True)
    ref = g[f"{name}_dist"]
    bad = outside(_np(dist), ref)
    print(name, "max |dist - ref|", np.abs(_np(dist) - ref).max(), "share outside", float(bad.mean()))
    if name in PATH_DEPENDENT:
        assert float(bad.mean()) <= PATH_DEPENDENT[name]
    else:
        assert not bad.any()
        np.testing.assert_allclose(_np(prob), g[f"{name}_prob"], rtol=2e-6, atol=1e-9)


def test_beta_and_leading_zero_coefficients():
    g = load_golden("pf_sample")
    coef, c, r = golden_case(g, "d3_p20")
    check_against_oracle("beta 2", flat_tables(c, r), frontier_of(coef), beta=2.0)
    from osrl_amd.common.ingest import compute_sample_prob
    a = compute_sample_prob(flat_tables(c, r), frontier_of(coef), with_dist=True)[1]
    b = compute_sample_prob(flat_tables(c, r), frontier_of(np.concatenate([[0.0, 0.0], coef])), with_dist=True)[1]
    assert torch.equal(a, b)  # np.poly1d strips leading zeros
    with pytest.raises(ValueError):
        compute_sample_prob(flat_tables(c, r), frontier_of(coef), beta=0.0)


def test_two_runs_are_bit_identical():
    from osrl_amd.common.ingest import compute_sample_prob
    rs = np.random.RandomState(7)
    coef = np.polyfit(np.linspace(0, 80, 30), 50 + 6 * np.linspace(0, 80, 30) + rs.normal(0, 10, 30), 5)
    tables = flat_tables(rs.uniform(0, 80, 100_000), rs.uniform(0, 700, 100_000))
    a = compute_sample_prob(tables, frontier_of(coef), with_cdf=True, with_dist=True)
    b = compute_sample_prob(tables, frontier_of(coef), with_cdf=True, with_dist=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _draw(st, B=512):
    from osrl_amd.engine.core import StepState
    sst = StepState(DEV, ["x"])
    sst.tick()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    T = st.T
    outs = (z(B, T, st.od), z(B, T, st.ad), z(B, T), z(B, T), z(B, T, dt=torch.int64), z(B, T), z(B), z(B, T))
    idx = z(B, 2, dt=torch.int32)
    st.gather(*outs, sst.ptr, idx_out=idx)
    torch.cuda.synchronize()
    return idx


def test_store_draws_from_the_frontier_distribution():
    from osrl_amd.common.replay import SequenceStore
    st = augmented_store("d3_p20", seed=11)
    uniform = _draw(st)
    st.enable_pf_sampling()
    tables = dict(observations=st.obs, actions=st.act, returns=st.ret, cost_returns=st.cret, costs=st.cost,
                  traj_start=st.traj_start, traj_len=st.traj_len)
    other = SequenceStore.from_tables(tables, 10, cdf=st.cdf.clone(), seed=11)
    got, want = _draw(st), _draw(other)
    assert torch.equal(got, want)
    assert not torch.equal(got, uniform)
    ii = _np(got)
    assert ii[:, 0].min() >= 0 and ii[:, 0].max() < st.n_traj
    assert np.all(ii[:, 1] < _np(st.traj_len)[ii[:, 0]])
    # a frontier fitted outside the store (no augmentation) gives a store the same distribution
    from osrl_amd.common.ingest import pareto_frontier
    dkw, _ = SEQ_CASES["d3_p20"]
    plain = SequenceStore.from_dataset(make_augment_dataset(**dkw), 10, DEV)
    with pytest.raises(AttributeError):
        plain.enable_pf_sampling()
    c0, r0 = plain.cret[plain.traj_start], plain.ret[plain.traj_start]
    plain.enable_pf_sampling(beta=2.0, frontier=pareto_frontier(c0, r0, deg=2))
    assert plain.cdf is not None and abs(float(plain.cdf[-1]) - 1.0) < 1e-6
    assert torch.all(plain.cdf[1:] >= plain.cdf[:-1])


def test_set_sample_prob_and_callable_cost_transform():
    from osrl_amd.common.ingest import compute_cost_sample_prob
    from osrl_amd.common.replay import SequenceStore
    data = make_augment_dataset(seed=9)
    a = SequenceStore.from_dataset(data, 10, DEV, cost_sample=True)
    b = SequenceStore.from_dataset(data, 10, DEV)
    c0 = _np(b.cret[b.traj_start]).astype(np.float64)
    assert (c0 > 50).any()  # the clamp at 0 is exercised
    b.set_sample_prob(np.maximum(50.0 - c0, 0.0))
    np.testing.assert_allclose(_np(b.cdf), _np(a.cdf), rtol=0, atol=2e-6)
    b.set_sample_prob(torch.as_tensor(np.maximum(50.0 - c0, 0.0), device=DEV))  # device weights
    np.testing.assert_allclose(_np(b.cdf), _np(a.cdf), rtol=0, atol=2e-6)
    for bad in (np.full(b.n_traj, -1.0), np.zeros(b.n_traj), np.ones(b.n_traj - 1)):
        with pytest.raises(ValueError):
            b.set_sample_prob(bad)
    tb = dict(cost_returns=b.cret, traj_start=b.traj_start)
    p_fn, cdf_fn = compute_cost_sample_prob(tb, lambda x: 70 - x, with_cdf=True)
    p_af, cdf_af = compute_cost_sample_prob(tb, ("affine", -1, 70), with_cdf=True)
    np.testing.assert_allclose(_np(cdf_fn), _np(cdf_af), rtol=0, atol=2e-6)
    np.testing.assert_allclose(_np(p_fn), _np(p_af), rtol=2e-6, atol=1e-9)
    s_fn = SequenceStore.from_dataset(data, 10, DEV, cost_sample=True, cost_transform=lambda x: 70 - x)
    s_af = SequenceStore.from_dataset(data, 10, DEV, cost_sample=True, cost_transform=("affine", -1, 70))
    np.testing.assert_allclose(_np(s_fn.cdf), _np(s_af.cdf), rtol=0, atol=2e-6)
    assert torch.equal(s_af.cdf, cdf_af)  # the tuple forms keep their device path
