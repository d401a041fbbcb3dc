"""Compile-time guards for the long-sequence / wide-embedding CDT kernels (CPU only: hipcc cross-compiles gfx950
assembly without a GPU): every instantiation of the tiled attention kernels, the chunked-K linear kernel and the
16-features-per-lane row kernels runs without scratch, the GEMM-shaped ones on fp32 MFMA, and the dynamic LDS the
launchers request (queried from the library: these kernels have no static LDS) stays within 160 KB per workgroup.
Also: the CDT constructor's new limits (no GPU needed to be refused)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def _kernels(path):
    """{mangled name: dict(mfma, scratch)} of an assembly listing."""
    res, kern = {}, None
    for ln in open(path):
        m = re.match(r'^(_Z\w+):', ln)
        if m:
            kern = m.group(1)
            res[kern] = dict(mfma=0, scratch=-1)
            continue
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', ln)
        if m:
            kern = m.group(1)
            continue
        if kern is None or kern not in res:
            continue
        r = res[kern]
        if re.search(r'\bv_mfma_f32_(16x16x4|32x32x2)', ln):
            r["mfma"] += 1
        m = re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', ln)
        if m:
            r["scratch"] = int(m.group(1))
    return res


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if HIPCC is None:
        pytest.fail("hipcc is required to cross-compile the gfx950 listings")
    from osrl_amd.build import FILE_FLAGS, FLAGS
    d = tmp_path_factory.mktemp("isa_long")
    procs = {}
    for name in ("cdt", "mlp", "env"):
        out = str(d / f"{name}.s")
        cmd = [HIPCC] + FLAGS + FILE_FLAGS.get(f"{name}.hip", []) + \
            ["-S", "--cuda-device-only", os.path.join(ROOT, "osrl_amd", "csrc", f"{name}.hip"), "-o", out]
        procs[name] = (subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL), out)
    res = {}
    for name, (p, out) in procs.items():
        assert p.wait() == 0, f"hipcc -S failed on {name}.hip"
        res.update(_kernels(out))
    return res


ATTN = [f"{k}ILi{dp}E" for k in ("attn_fwd_t_kernel", "attn_bwd_dq_t_kernel", "attn_bwd_dkv_t_kernel")
        for dp in (16, 32, 64, 128)]
LINEAR = [f"linear_kchunk_kernelILi{c}E" for c in (1, 2, 4, 7)]
ROWS = ["embed_ln_kernelILi16E", "ln_fwd_kernelILb0ELi16E", "ln_fwd_kernelILb1ELi16E", "ln_bwd_kernelILb0ELi16E",
        "ln_bwd_kernelILb1ELi16E", "attn_rowdot_kernel", "cdt_push_kernelILb0E"]


def _find(listings, needle):
    hits = [k for k in listings if needle in k]
    assert len(hits) == 1, (needle, hits)
    return listings[hits[0]]


@pytest.mark.parametrize("needle", ATTN + LINEAR + ROWS)
def test_new_kernels_fit(listings, needle):
    r = _find(listings, needle)
    assert r["scratch"] == 0, (needle, r)


def test_dynamic_lds_of_the_new_launches_fits_a_workgroup():
    """The tiled attention kernels and the chunked linear kernel take all their LDS dynamically (the listing's static
    size is 0): the sizes their launchers request, by head width and pass, are <= 160 KB -- and they are what the
    layout needs (two [64, DP + 8] tiles or K + V^T, plus 64-128 row values), so the check is not vacuous."""
    from osrl_amd import _lib as L
    lib = L.load()
    for d in range(1, 129):
        dp = 16 if d <= 16 else 32 if d <= 32 else 64 if d <= 64 else 128
        want = [4 * (64 * (dp + 8) + dp * 72 + 64), 4 * (2 * 64 * (dp + 8) + 64), 4 * (2 * 64 * (dp + 8) + 128)]
        for ps in range(3):
            got = int(lib.osrl_attention_tiled_lds_bytes(d, ps))
            assert got == want[ps] and got <= 160 * 1024, (d, ps, got)
    assert lib.osrl_attention_tiled_lds_bytes(129, 0) == 0
    assert int(lib.osrl_linear_kchunk_lds_bytes()) == 4 * 16 * (1024 + 8) <= 160 * 1024


@pytest.mark.parametrize("needle", ATTN + LINEAR)
def test_attention_and_linear_kernels_run_on_fp32_mfma(listings, needle):
    assert _find(listings, needle)["mfma"] > 0, needle


@pytest.mark.parametrize("kw,what", [
    (dict(seq_len=256, use_rew=True, use_cost=True, cost_prefix=True), "1025 tokens"),  # 4 * 256 + 1
    (dict(seq_len=513), "1026 tokens"),
    (dict(embedding_dim=1040, num_heads=16), "embedding_dim 1040 > 1024"),
    (dict(embedding_dim=512, num_heads=2), "head_dim 256 > 128"),
    (dict(embedding_dim=130, num_heads=8), "not divisible"),
])
def test_constructor_refuses_past_the_limits(kw, what):
    from osrl_amd.algorithms import CDT
    with pytest.raises(NotImplementedError, match=what):
        CDT(5, 2, 1.0, device="cuda", **kw)


def test_constructor_limits_accept_the_new_range():
    """The limit check itself (before any device work): S = 1024 and E = 1024 / head_dim 128 are not refused for their
    size -- on a machine without a GPU the constructor gets as far as asking for the device."""
    from osrl_amd.algorithms import CDT
    for kw in (dict(seq_len=256, use_rew=True, use_cost=True), dict(embedding_dim=1024, num_heads=8),
               dict(embedding_dim=768, num_heads=6, seq_len=40, use_rew=True, use_cost=True)):
        try:
            CDT(5, 2, 1.0, device="cuda", **kw)
        except RuntimeError as e:  # a machine without a GPU: the size check passed, the device request failed
            assert "no HIP device visible" in str(e), e
