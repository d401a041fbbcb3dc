"""The "bf16x3" projections (csrc/linear_split.hip, CDTTrainer(matmul="bf16x3")) without a GPU: a numpy restatement of
the truncation split and of the six-product sum, compile-time guards on the kernel's gfx950 listing, the ABI mirrors
and the argument checks that run before any device work."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
SRC = os.path.join(ROOT, "osrl_amd", "csrc", "linear_split.hip")
HI = np.uint32(0xFFFF0000)


def split3(a):
    """split3 of csrc/linear_split.hip on float32 arrays: h = a with its low 16 bits cleared, m = the same of a - h, l =
    the high half of (a - h) - m, which is what pack_hi keeps.  All three are bf16 values held in fp32."""
    a = np.asarray(a, np.float32)
    h = (a.view(np.uint32) & HI).view(np.float32)
    r1 = (a - h).astype(np.float32)
    m = (r1.view(np.uint32) & HI).view(np.float32)
    l = ((r1 - m).astype(np.float32).view(np.uint32) & HI).view(np.float32)
    return h, m, l


def is_bf16(x):
    return (np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF)) == 0


def _samples():
    rs = np.random.RandomState(7)
    bits = rs.randint(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32)
    rnd = bits.view(np.float32)
    rnd = rnd[np.isfinite(rnd)]
    fmax = np.finfo(np.float32).max
    edge = np.array([0.0, -0.0, 1.0, -1.0, fmax, -fmax, np.nextafter(np.float32(fmax), np.float32(0)), 3.0e38, -3.3e38,
                     2.0 ** -110, -(2.0 ** -110) * 1.9999999, 2.0 ** -126, 1.1754942e-38], np.float32)
    return np.concatenate([rnd, edge, (rs.randn(50000) * 4).astype(np.float32), -np.abs(rs.randn(1000)).astype(np.float32)])


def test_split_is_exact_and_every_piece_is_bf16():
    """h + m + l == a bit for bit wherever three bf16 numbers CAN hold a: every finite fp32 with |a| >= 2^-110 (the third
    piece sits 16 bits below a's exponent and bf16's exponent range ends where fp32's does), zeros and both signs, up to
    the largest finite value.  The pieces carry the sign of a (so |h| + |m| + |l| = |a|)."""
    a = _samples()
    a = a[(np.abs(a) >= 2.0 ** -110) | (a == 0)]
    assert a.size > 150000 and (a < 0).any() and (a == 0).any() and (np.abs(a) > 3e38).any()
    h, m, l = split3(a)
    for p in (h, m, l):
        assert is_bf16(p).all()
        assert ((p == 0) | (np.signbit(p) == np.signbit(a))).all()
    s = ((h + m).astype(np.float32) + l).astype(np.float32)
    assert (s.view(np.uint32) == a.view(np.uint32))[a != 0].all()
    assert (s[a == 0] == 0).all()
    assert (h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64) == a.astype(np.float64)).all()


def test_split_of_tiny_and_subnormal_values():
    """Below 2^-110 the low bits of an fp32 lie under bf16's smallest subnormal (2^-133): no three bf16 numbers hold them.
    The pieces are still bf16 values, the split is exact for every subnormal that is a multiple of 2^-133, and what is
    lost otherwise is less than 2^-133 absolute -- 2^-23 relative to the smallest NORMAL fp32, i.e. below the unit
    roundoff of any product with a normal-range result."""
    rs = np.random.RandomState(8)
    sub = rs.randint(1, 2 ** 23, size=20000, dtype=np.uint64).astype(np.uint32)        # every fp32 subnormal pattern
    sub = np.concatenate([sub, sub | np.uint32(0x80000000)]).view(np.float32)
    tiny = (rs.rand(20000).astype(np.float32) * np.float32(2.0 ** -111)).astype(np.float32)
    for a in (sub, tiny):
        h, m, l = split3(a)
        assert is_bf16(h).all() and is_bf16(m).all() and is_bf16(l).all()
        err = np.abs(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64) - a.astype(np.float64))
        assert err.max() < 2.0 ** -133
    grid = (np.arange(1, 128, dtype=np.float64) * 2.0 ** -133).astype(np.float32)      # subnormals bf16 can hold
    h, m, l = split3(grid)
    assert (h == grid).all() and (m == 0).all() and (l == 0).all()


def test_non_finite_values_stay_non_finite():
    """The split of +-Inf is (Inf, NaN, NaN) and a NaN keeps a NaN piece: a product with them is NaN, never finite."""
    with np.errstate(invalid="ignore"):
        for v in (np.inf, -np.inf, np.nan, np.uint32(0x7F800001).view(np.float32)):
            h, m, l = split3(np.array([v], np.float32))
            assert not np.isfinite(h[0] * 1.0 + m[0] * 1.0 + l[0] * 1.0)
            assert np.isnan(m[0]) or np.isnan(h[0])


PA, PB = (2, 0, 1, 1, 0, 0), (0, 2, 1, 0, 1, 0)  # (A piece, W piece) of the six kept products, the kernel's order


def six_term_dot(a, w):
    """Rows of a [R,K] times w [K] the way the kernel sums them: per 16-deep block the six piece products in the kernel's
    order, every term exact (16-bit product), one fp32 rounding per addition (sequential: the matrix unit's own order
    inside a block is not specified, and the bound below holds for any order)."""
    ap, wp = split3(a), split3(w)
    acc = np.zeros(a.shape[0], np.float32)
    for k0 in range(0, a.shape[1], 16):
        for t in range(6):
            for k in range(k0, k0 + 16):
                term = ap[PA[t]][:, k].astype(np.float64) * float(wp[PB[t]][k])
                assert (term == term.astype(np.float32)).all()  # exact in fp32
                acc = (acc.astype(np.float64) + term).astype(np.float32)
    return acc


@pytest.mark.parametrize("K", [256, 1024])
def test_six_term_sum_obeys_the_bound(K):
    """|y - y64| <= ((6K + 2) 2^-24 1.01 + 2^-23 + 2^-32) sum_k |a_k||w_k|: 6K exact terms accumulated in fp32 (each of
    the 6K - 1 additions rounds by 2^-24 of a partial sum that is at most sum |a||w|, since the pieces keep their
    parent's sign; the 1.01 covers the second-order terms) plus the three dropped products m l + l m + l l <=
    (2^-8 2^-16 + 2^-16 2^-8 + 2^-32) |a||w| < (2^-23 + 2^-32) |a||w|.  The bound is a worst case over
    every order of summation; the typical error is far inside it."""
    rs = np.random.RandomState(K)
    a = (rs.rand(48, K).astype(np.float32) - 0.5) * 4
    w = ((rs.rand(K).astype(np.float32) - 0.5) * 0.25).astype(np.float32)
    y = six_term_dot(a, w).astype(np.float64)
    y64 = a.astype(np.float64) @ w.astype(np.float64)
    s = np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64))
    bound = ((6 * K + 2) * 2.0 ** -24 * 1.01 + 2.0 ** -23 + 2.0 ** -32) * s
    assert (np.abs(y - y64) <= bound).all()


# ---- ISA guards ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if HIPCC is None:
        pytest.fail("hipcc is required to cross-compile the gfx950 listing")
    from osrl_amd.build import FILE_FLAGS, FLAGS, SOURCES
    assert "linear_split.hip" in SOURCES
    out = str(tmp_path_factory.mktemp("isa_split") / "linear_split.s")
    cmd = [HIPCC] + FLAGS + FILE_FLAGS.get("linear_split.hip", []) + ["-S", "--cuda-device-only", SRC, "-o", out]
    assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    res, kern = {}, None
    for ln in open(out):
        m = re.match(r'^(_Z\w+):', ln)
        if m:
            kern = m.group(1)
            res[kern] = dict(mfma=0, other_mfma=0, scratch=-1, lds=-1, vgpr=-1, agpr=0)
            continue
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', ln)
        if m:
            kern = m.group(1)
            continue
        if kern is None or kern not in res:
            continue
        r = res[kern]
        if re.search(r'\bv_mfma_f32_32x32x16_bf16\b', ln):
            r["mfma"] += 1
        elif re.search(r'\bv_mfma_', ln):
            r["other_mfma"] += 1
        for key, pat in (("scratch", r'\.amdhsa_private_segment_fixed_size\s+(\d+)'),
                         ("lds", r'\.amdhsa_group_segment_fixed_size\s+(\d+)'),
                         ("vgpr", r';\s*TotalNumVgprs:\s*(\d+)')):
            m = re.search(pat, ln)
            if m:
                r[key] = int(m.group(1))
    return res


def _kern(listing, name):
    hits = [v for k, v in listing.items() if name in k]
    assert len(hits) == 1, (name, list(listing))
    return hits[0]


def test_gemm_kernel_runs_on_the_bf16_matrix_cores_without_scratch(listing):
    k = _kern(listing, "linear_split_kernel")
    # 2 k16 steps x 6 products x 2 x 2 blocks per staged slab, and no f32-input MFMA beside them
    assert k["mfma"] == 48 and k["other_mfma"] == 0, k
    assert k["scratch"] == 0, k
    assert _kern(listing, "split_planes_kernel")["scratch"] == 0


def test_lds_and_registers_allow_the_claimed_occupancy(listing):
    """__launch_bounds__(256, kWgPerCu): kWgPerCu workgroups of 4 waves per CU = kWgPerCu waves per SIMD, each of which
    gets 512 / kWgPerCu registers (in blocks of 8) and 1 / kWgPerCu of the CU's 160 KB of LDS."""
    from osrl_amd import _lib as L
    src = open(SRC).read()
    wg = int(re.search(r'constexpr int kWgPerCu = (\d+);', src).group(1))
    assert re.search(r'__launch_bounds__\(kThreads, kWgPerCu\)\s+void linear_split_kernel', src)
    k = _kern(listing, "linear_split_kernel")
    lds = k["lds"] + int(L.load().osrl_linear_split_lds_bytes())
    assert 0 < lds <= 160 * 1024 and wg * lds <= 160 * 1024, (wg, lds)
    assert 0 < k["vgpr"] <= (512 // wg) // 8 * 8, (wg, k)


def test_kernels_read_no_launch_dimensions():
    src = open(SRC).read()
    assert "blockDim" not in src and "gridDim" not in src


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_prototypes_match_the_header():
    from osrl_amd import _lib as L
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, "include", "osrl_amd.h")).read(), flags=re.S)
    for name in ("osrl_linear_split", "osrl_linear_split_supported", "osrl_linear_split_lds_bytes", "osrl_split_planes"):
        m = re.search(r'\b(int|int64_t)\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
        assert m, name
        args = [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
        assert len(args) == len(L.PROTOTYPES[name]), name
        assert (m.group(1) == "int64_t") == (name in L.RESTYPES), name
    lib = L.load()
    for M, K, N, want in ((333, 256, 1024, 1), (333, 256, 768, 1), (81920, 1024, 256, 1), (1, 256, 256, 1), (7, 768, 256, 1),
                          (160, 128, 384, 1), (160, 128, 512, 1), (160, 512, 128, 1), (160, 128, 128, 1),
                          (160, 256, 6, 0), (160, 16, 128, 0), (160, 40, 128, 0), (160, 256, 192, 0), (0, 256, 256, 0)):
        assert int(lib.osrl_linear_split_supported(M, K, N)) == want, (M, K, N)
    # bad arguments are -1 before any launch (no device is touched)
    assert lib.osrl_linear_split(None, 256, 4, 256, None, 256 * 256, 256, None, None, 0, None, 256, None) == -1
    assert lib.osrl_linear_split(16, 256, 4, 256, 16, 256 * 256, 6, None, None, 0, 16, 6, None) == -1      # N
    assert lib.osrl_linear_split(16, 255, 4, 256, 16, 256 * 256, 256, None, None, 0, 16, 256, None) == -1  # lda < K
    assert lib.osrl_linear_split(20, 256, 4, 256, 16, 256 * 256, 256, None, None, 0, 16, 256, None) == -1  # A alignment
    assert lib.osrl_split_planes(None, None, None, None, 1, 1, None) == -1


def test_pack_entry_mirror_matches_the_header(tmp_path):
    """osrl_split_planes takes osrl_pack_entry_t entries (no new struct): its ctypes mirror against the C header."""
    import ctypes as C
    from osrl_amd import _lib as L
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src, exe = str(tmp_path / "sz.c"), str(tmp_path / "sz")
    names = {"in_": "in"}
    with open(src, "w") as f:
        f.write('#include "osrl_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n')
        f.write('  printf("%zu", sizeof(osrl_pack_entry_t));\n')
        for fname, _ in L.PackEntryT._fields_:
            f.write(f'  printf(" %zu", offsetof(osrl_pack_entry_t, {names.get(fname, fname)}));\n')
        f.write('  printf("\\n");\n  return 0;\n}\n')
    subprocess.run([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    want = [C.sizeof(L.PackEntryT)] + [getattr(L.PackEntryT, fname).offset for fname, _ in L.PackEntryT._fields_]
    assert [int(x) for x in out] == want


# ---- public interface ----------------------------------------------------------------------------------------------
def test_unknown_matmul_raises_before_any_device_work():
    from types import SimpleNamespace
    from osrl_amd.algorithms import CDTTrainer
    from osrl_amd.engine.cdt import CDTEngine
    with pytest.raises(ValueError, match="nope"):
        CDTTrainer(None, matmul="nope")          # (no model, no device: the check comes first)
    with pytest.raises(ValueError, match="nope"):
        CDTEngine(SimpleNamespace(), 4, dict(matmul="nope"))
    import inspect
    params = list(inspect.signature(CDTTrainer.__init__).parameters.values())
    assert params[-1].name == "matmul" and params[-1].default == "f32"  # trailing keyword, default f32


def test_matmul_plan_choice_and_lab_knob(monkeypatch):
    from osrl_amd.engine import plan
    monkeypatch.delenv("OSRL_CDT_MATMUL", raising=False)
    assert plan.cdt_matmul() == "f32" and plan.cdt_matmul("bf16x3") == "bf16x3"
    assert "OSRL_CDT_MATMUL" in plan.KNOBS
    monkeypatch.setenv("OSRL_CDT_MATMUL", "bf16x3")
    monkeypatch.delenv("OSRL_LAB", raising=False)
    assert plan.cdt_matmul("f32") == "f32"       # a production run ignores lab switches
    monkeypatch.setenv("OSRL_LAB", "1")
    assert plan.cdt_matmul("f32") == "bf16x3"
    monkeypatch.setenv("OSRL_CDT_MATMUL", "fp8")
    with pytest.raises(ValueError):
        plan.cdt_matmul("f32")
    p = plan.CDTPlan(matmul="f32")
    assert vars(p)["matmul"] == "f32" and p.split_fwd == 0 and p.split_dx == 0
