"""What the GPU tests of the dynamics ensemble's bootstrap / holdout / elites rely on, checked without a GPU: the Poisson
table, the host weights, the oracle's weighted gradient (tests/dyn_ensemble_oracle.py), the tie rule, the header against
its ctypes mirror, and the compiled kernel's resources (hipcc cross-compiles gfx950 assembly without a GPU)."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dyn_ensemble_cases as DC
import dyn_ensemble_oracle as DO
import gauss_dynamics_cases as GC
import model_env_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
SRC = os.path.join(ROOT, "osrl_amd", "csrc", "dyn_loss.hip")


def _header():
    return open(os.path.join(ROOT, "include", "osrl_amd.h")).read()


# ---- the table ----------------------------------------------------------------------------------------------------------
def test_poisson_table_against_fp64():
    p = [math.exp(-1.0) / math.factorial(k) for k in range(8)]
    assert abs(math.fsum(p) - 1.0) < 1.1e-5 and math.fsum(p) < 1.0  # the tail P(w >= 8) ~ 1.02e-5 goes to w = 8
    want = [int(math.floor(2.0 ** 32 * math.fsum(p[:k + 1]))) for k in range(8)]
    assert DO.BOOT_T == want and all(a < b for a, b in zip(want, want[1:])) and want[-1] < 2 ** 32
    src = open(SRC).read()
    m = re.search(r"kBootT\[8\]\s*=\s*\{([^}]*)\}", src)
    assert m is not None
    assert [int(x.strip().rstrip("u")) for x in m.group(1).split(",")] == want
    # E[w] from the table itself: sum_k P(word >= T_k) = 1 to ~1e-6
    mean = sum(1.0 - t / 2.0 ** 32 for t in want)
    assert abs(mean - 1.0) < 2e-6, mean
    assert re.search(r"kBootStream\s*=\s*17\b", src) and DO.BOOT_STREAM == 17


def test_weight_mean_over_100000_pairs():
    """4 sigma of the mean of 100 000 draws at variance 1 is 0.0126."""
    w = DO.boot_weights(DC.MEAN_SEED, np.arange(DC.MEAN_ROWS), DC.MEAN_NETS)
    assert w.size == 100000 and w.min() >= 0 and w.max() <= 8 and np.array_equal(w, np.round(w))
    print(f"bootstrap weights: mean {w.mean():.5f}, variance {w.var():.5f}, P(w = 0) {np.mean(w == 0):.5f}")
    assert abs(w.mean() - 1.0) <= 0.013, w.mean()
    assert abs(np.mean(w == 0) - math.exp(-1.0)) < 0.01


def test_weights_depend_on_seed_row_and_member_only():
    idx = np.array([5, 0, DC.IDX_MAX, 5, 77], np.int64)
    w = DO.boot_weights(DC.BOOT_SEED, idx, 8)
    assert np.array_equal(w[:, 0], w[:, 3])  # the same row drawn twice
    assert np.array_equal(w[:5], DO.boot_weights(DC.BOOT_SEED, idx, 5))  # a member's weight does not depend on n_nets
    assert np.array_equal(w[:, ::-1], DO.boot_weights(DC.BOOT_SEED, idx[::-1], 8))  # nor on the position in the batch
    big = DO.boot_weights(DC.BOOT_SEED, np.arange(512), 8)
    assert not np.array_equal(big, DO.boot_weights(DC.BOOT_SEED + 1, np.arange(512), 8))
    assert not np.array_equal(big, DO.boot_weights(DC.BOOT_SEED ^ (1 << 40), np.arange(512), 8))  # the key's high half
    assert not np.array_equal(big[0], big[1])


def test_the_zero_member_batch_is_what_it_says():
    idx = DC.zero_member_idx()
    w = DO.boot_weights(DC.BOOT_SEED, idx, DC.ZERO_NETS)
    assert (w[DC.ZERO_MEMBER] == 0).all() and len(set(idx.tolist())) == DC.ZERO_ROWS
    assert all((w[m] > 0).any() for m in range(DC.ZERO_NETS) if m != DC.ZERO_MEMBER)


def test_kernel_cases_cover_the_edges():
    assert {c[0] for c in DC.KERNEL_CASES} == {1, 17, 40, 333}
    assert {c[1] for c in DC.KERNEL_CASES} == {1, 17, 76, 256}
    assert {c[2] for c in DC.KERNEL_CASES} == {1, 5, 8}
    for rows, od, n in DC.KERNEL_CASES:
        for kind in DC.KINDS:
            assert kind == "mse" or DC.width(od, kind) % 2 == 1  # the Gaussian's 2 od + 3 is odd at every od
            y, t, idx = DC.kernel_inputs(rows, od, n, kind)
            assert idx[0] == 0 and idx.min() >= 0 and idx.max() <= DC.IDX_MAX
            assert rows == 1 or idx[-1] == DC.IDX_MAX
            assert rows < 3 or idx[1] == idx[2]
            if kind == "gauss" and rows * (od + 1) * n >= 7:
                raw = y[:, :, od + 2:]
                for v in (DC.LOGVAR_MIN, DC.LOGVAR_MAX, 50.0, -50.0, 60.0, -60.0):
                    assert (raw == np.float32(v)).any(), (rows, od, n, v)
                assert (raw > DC.LOGVAR_MAX).any() and (raw < DC.LOGVAR_MIN).any()


# ---- the oracle's weighted loss -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", DC.KINDS)
def test_weighted_gradient_against_central_differences(kind):
    rows, od, M = 6, 3, 3
    rs = np.random.RandomState(5)
    y = rs.randn(M, rows, DC.width(od, kind))
    if kind == "gauss":
        y[:, :, od + 2:] = rs.uniform(DC.LOGVAR_MIN - 3.0, DC.LOGVAR_MAX + 3.0, (M, rows, od + 1))
    t = rs.randn(rows, od + 2)
    w = DO.boot_weights(DC.BOOT_SEED, np.arange(rows), M)
    assert (w == 0).any() and (w > 1).any()
    scale = 1.0 / t.size
    lo, hi = DC.LOGVAR_MIN, DC.LOGVAR_MAX
    total = lambda yy: DO.weighted_stat(DO.member_loss(yy, t, kind, scale, w, lo, hi)[0], w, scale)  # noqa: E731
    _, dy = DO.member_loss(y, t, kind, scale, w, lo, hi)
    num = np.zeros_like(y)
    h = 1e-6
    for i in np.ndindex(*y.shape):
        a, b = y.copy(), y.copy()
        a[i] += h
        b[i] -= h
        num[i] = (total(a) - total(b)) / (2 * h)
    assert np.abs(num - dy).max() <= 1e-8 * max(1.0, np.abs(dy).max()), np.abs(num - dy).max()


@pytest.mark.parametrize("kind", DC.KINDS)
def test_zero_weight_rows_contribute_nothing(kind):
    rows, od, M = 8, 4, 2
    rs = np.random.RandomState(6)
    y, t = rs.randn(M, rows, DC.width(od, kind)), rs.randn(rows, od + 2)
    w = np.ones((M, rows))
    w[0, 3] = w[1, 5] = 0.0
    args = (kind, 0.1, w, DC.LOGVAR_MIN, DC.LOGVAR_MAX)
    l0, dy0 = DO.member_loss(y, t, *args)
    y2, t2 = y.copy(), t.copy()
    y2[0, 3] += 100.0
    l1, dy1 = DO.member_loss(y2, t2, *args)
    assert (dy0[0, 3] == 0).all() and (dy1[0, 3] == 0).all() and np.array_equal(dy0, dy1)
    assert DO.weighted_stat(l0, w, 0.1) == DO.weighted_stat(l1, w, 0.1) and l0[0, 3] != l1[0, 3]
    t2[5] += 1.0  # the target of a row member 1 does not see: member 1's gradient stays, member 0's moves
    _, dy2 = DO.member_loss(y, t2, *args)
    assert np.array_equal(dy2[1, 5], dy0[1, 5]) and not np.array_equal(dy2[0, 5], dy0[0, 5])


@pytest.mark.parametrize("gauss", [False, True])
def test_weighted_step_with_unit_weights_is_the_base_oracles_step(gauss):
    c = DC.TRAIN
    sd = (GC.gauss_state_dict if gauss else MC.dyn_state_dict)(c["od"], c["ad"], c["hidden"], c["M"])
    d = DC.transitions(c["B"], c["od"], c["ad"])
    b = [d[k] for k in DC.BATCH_KEYS]
    a, o = DO.make_oracle(sd, c["lr"]), DO.make_oracle(sd, c["lr"])
    sa, so = a.boot_step(*b), o.step(*b)
    assert abs(sa["loss/dynamics_loss"] - so["loss/dynamics_loss"]) <= 1e-12 * abs(so["loss/dynamics_loss"])
    for k in o.train_keys:
        np.testing.assert_allclose(a.p[k], o.p[k], rtol=0, atol=1e-14)
    w = DO.make_oracle(sd, c["lr"], DC.BOOT_SEED)
    w.boot_step(*b, row_ids=np.arange(c["B"]))
    assert any(not np.array_equal(w.p[k], o.p[k]) for k in o.train_keys)
    val = a.validate(*b)
    assert val.shape == (c["M"],) and np.isfinite(val).all()


def test_elite_tie_rule():
    assert DO.elite_indices([0.5, 0.1, 0.1, 0.7, 0.1], 2) == [1, 2]
    assert DO.elite_indices([0.3, 0.3, 0.3], 2) == [0, 1]
    assert DO.elite_indices([3.0, 2.0, 1.0, 0.0], 3) == [1, 2, 3]
    assert DO.elite_indices([1.0, -np.inf, 1.0], 1) == [1]
    from osrl_amd.algorithms.dynamics import elite_indices
    for losses, k in (([0.5, 0.1, 0.1, 0.7, 0.1], 2), ([0.3, 0.3, 0.3], 2), ([3.0, 2.0, 1.0, 0.0], 3), ([2.0, 1.0], 2)):
        assert elite_indices(losses, k) == DO.elite_indices(losses, k)


# ---- header <-> ctypes ------------------------------------------------------------------------------------------------------
def test_prototype_and_enums_match_the_header():
    from osrl_amd import _lib as L
    h = _header()
    assert "osrl_dyn_member_loss" in L.PROTOTYPES and re.search(r"int\s+osrl_dyn_member_loss\s*\(", h)
    assert len(L.PROTOTYPES["osrl_dyn_member_loss"]) == 2
    for name, v in (("OSRL_DYN_LOSS_MSE", L.DYN_LOSS_MSE), ("OSRL_DYN_LOSS_GAUSS_NLL", L.DYN_LOSS_GAUSS_NLL)):
        m = re.search(rf"\b{name}\s*=\s*(\d+)", h)
        assert m is not None and int(m.group(1)) == v
    m = re.search(r"#define\s+OSRL_DYN_LOSS_TILE\s+(\d+)", h)
    assert m is not None and int(m.group(1)) == L.DYN_LOSS_TILE
    from osrl_amd.build import SOURCES
    assert "dyn_loss.hip" in SOURCES


def test_struct_mirror_has_the_headers_field_order():
    import ctypes as C

    from osrl_amd import _lib as L
    body = re.search(r"typedef struct \{([^}]*)\}\s*osrl_dyn_loss_t;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[^A-Za-z0-9_]", "", part.split()[-1]) for part in decl.split(",")]
    assert names == [f for f, _ in L.DynLossT._fields_]
    assert C.sizeof(L.DynLossT) == 10 * 8 + 8 * 4
    assert all(t is C.c_void_p for _, t in L.DynLossT._fields_[:10])
    assert [t for _, t in L.DynLossT._fields_[10:]] == [C.c_int32] * 4 + [C.c_float] * 4


# ---- the compiled kernel ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.fail("hipcc is required to cross-compile the gfx950 listing")
    from osrl_amd.build import FILE_FLAGS, FLAGS
    out = str(tmp_path_factory.mktemp("isa_dyn_loss") / "dyn_loss.s")
    cmd = [HIPCC] + FLAGS + FILE_FLAGS.get("dyn_loss.hip", []) + ["-S", "--cuda-device-only", SRC, "-o", out]
    assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    res, kern = {}, None
    for ln in open(out):
        m = re.match(r'^(_Z\w+):', ln)
        if m:
            kern = m.group(1)
            res[kern] = dict(scratch=-1, lds=-1, fatomic=0)
            continue
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', ln)
        if m:
            kern = m.group(1)
            continue
        if kern is None or kern not in res:
            continue
        r = res[kern]
        if re.search(r'\b(global|flat|buffer)_atomic_\w*(f32|f64|pk_add)', ln):
            r["fatomic"] += 1
        m = re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', ln)
        if m:
            r["scratch"] = int(m.group(1))
        m = re.search(r'\.amdhsa_group_segment_fixed_size\s+(\d+)', ln)
        if m:
            r["lds"] = int(m.group(1))
    return res


@pytest.mark.parametrize("name", ["dyn_loss_kernelE", "dyn_loss_kernel_pE"])
def test_kernel_compiles_without_scratch_or_float_atomics(kernels, name):
    hits = [v for k, v in kernels.items() if name in k]
    assert len(hits) == 1, (name, list(kernels))
    k = hits[0]
    assert k["scratch"] == 0, k
    assert 0 <= k["lds"] <= 64, k
    assert k["fatomic"] == 0, k
