"""The numpy restatement of the Pareto augmentation (tests/augment_oracle.py) against the reference's own outputs
(tests/golden/augment.npz, tests/golden/make_golden_augment.py) with the reference's recorded draws injected."""
import numpy as np
import pytest

from augment_cases import BC_KINDS, SEQ_CASES, make_augment_dataset, make_bc_frontier_dataset
import augment_oracle as AO
from oracle import ingest_oracle as IO
from oracle_util import load_golden


def flat_tables(trajs):
    """ingest_oracle's list of trajectory dicts -> the flat tables common.ingest.process_sequence_dataset returns."""
    out = {k: np.concatenate([t[k] for t in trajs]) for k in AO.KEYS}
    lens = np.array([len(t["costs"]) for t in trajs], np.int64)
    out["traj_len"] = lens
    out["traj_start"] = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return out


def golden_draws(g, name):
    return {k: g[f"{name}_{k}"] for k in ("pick", "u_rew", "u_part", "u_cr", "noise_c", "noise_r")
            if f"{name}_{k}" in g.files}


def check_combined(g, name, out, n_rows):
    for k in AO.KEYS:
        np.testing.assert_array_equal(out[k][n_rows:], g[f"{name}_aug_{k}"].reshape(out[k][n_rows:].shape), err_msg=k)
    np.testing.assert_array_equal(out["traj_len"], g[f"{name}_len"])


@pytest.mark.parametrize("name", [n for n, (_, kw) in SEQ_CASES.items() if "random_aug" not in kw and
                                  not kw.get("pf_only")])
def test_augmentation_restatement_matches_reference(name):
    g = load_golden("augment")
    dkw, skw = SEQ_CASES[name]
    t = flat_tables(IO.process_sequence_dataset(make_augment_dataset(**dkw), False))
    kw = {k: v for k, v in skw.items() if k != "augment_percent"}
    kw.setdefault("min_reward", 5)  # SequenceDataset's default (augmentation()'s own is 0)
    out, info = AO.augmentation(t, augment_percent=skw["augment_percent"], draws=golden_draws(g, name), **kw)
    np.testing.assert_array_equal(info["indices"], g[f"{name}_indices"])
    np.testing.assert_array_equal(info["pareto"], g[f"{name}_pareto"])
    np.testing.assert_allclose(info["coef"], g[f"{name}_coef"], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(info["idx"], g[f"{name}_idx"])
    check_combined(g, name, out, t["returns"].shape[0])
    np.testing.assert_allclose(IO.compute_cost_sample_prob(
        [dict(cost_returns=out["cost_returns"][s:s + n]) for s, n in zip(out["traj_start"], out["traj_len"])],
        lambda x: 50 - x), g[f"{name}_prob50"], rtol=1e-12)


def test_golden_covers_the_issue_cases():
    g = load_golden("augment")
    assert g["d3_p20_pick"].size > 0  # overfull bins
    assert any(np.unique(g[f"{n}_idx"]).size < g[f"{n}_idx"].size for n in ("d3_p20", "d0_p50"))  # duplicates
    assert g["d0_p50_u_part"].size > 0
    fc = np.array([0])  # single-point Pareto set: one value, tied indices
    t = flat_tables(IO.process_sequence_dataset(make_augment_dataset(**SEQ_CASES["single_pf"][0]), False))
    r0, c0 = AO.first_returns(t)
    ind, par = g["single_pf_indices"], g["single_pf_pareto"]
    assert np.unique(np.stack([c0[ind][par], r0[ind][par]]), axis=1).shape[1] == fc.size
    assert g["pf_only_aug_returns"].size == 0 and g["pf_only_len"].size == g["pf_only_n_original"]


def test_random_augmentation_restatement_matches_reference():
    g = load_golden("augment")
    dkw, skw = SEQ_CASES["rand_aug"]
    t = flat_tables(IO.process_sequence_dataset(make_augment_dataset(**dkw), False))
    kw = {k: v for k, v in skw.items() if k not in ("random_aug", "rstd", "cstd")}
    out, info = AO.random_augmentation(t, skw["random_aug"], draws=golden_draws(g, "rand_aug"), **kw)
    np.testing.assert_array_equal(info["idx"], g["rand_aug_idx"])
    check_combined(g, "rand_aug", out, t["returns"].shape[0])


@pytest.mark.parametrize("kind", BC_KINDS)
@pytest.mark.parametrize("gamma", [1.0, 0.99])
def test_bc_frontier_restatement_matches_reference(kind, gamma):
    g = load_golden("augment")
    d = make_bc_frontier_dataset(kind)
    st, ln = IO.episode_segments(IO.done_flags(d))
    cs = [IO.discounted_cumsum(d["costs"][s:s + n], gamma)[0] for s, n in zip(st, ln)]
    rs_ = [IO.discounted_cumsum(d["rewards"][s:s + n], gamma)[0] for s, n in zip(st, ln)]
    cr, rr = np.zeros_like(d["costs"]), np.zeros_like(d["rewards"])
    for s, n, c, r in zip(st, ln, cs, rs_):
        cr[s:s + n], rr[s:s + n] = c, r
    with np.errstate(all="ignore"):
        keep, deg = AO.bc_frontier(cs, rs_, cr, rr)
    assert deg == {"deg0": 2, "deg1": 1, "deg2": 2}[kind]
    np.testing.assert_array_equal(np.flatnonzero(keep), g[f"bc_{kind}_{gamma}_index"])
