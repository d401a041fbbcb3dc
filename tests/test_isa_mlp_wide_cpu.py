"""Compile-time and host-side guards of the wide MLP path (CPU only: hipcc cross-compiles gfx950 assembly without a
GPU): every instantiation of the per-layer kernel runs without scratch on fp32 MFMA and requests at most 160 KB of
dynamic LDS at every width up to OSRL_MAX_WIDTH, the act() GEMV kernel's wide form fits the LDS without scratch, the
constructors refuse what stays unsupported without a device, and the plan chooser gives wide shapes only forms that
exist for them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def _kernels(path):
    """{mangled name: dict(mfma, scratch, lds)} of an assembly listing."""
    res, kern = {}, None
    for ln in open(path):
        m = re.match(r'^(_Z\w+):', ln)
        if m:
            kern = m.group(1)
            res[kern] = dict(mfma=0, scratch=-1, lds=-1)
            continue
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', ln)
        if m:
            kern = m.group(1)
            continue
        if kern is None or kern not in res:
            continue
        r = res[kern]
        if re.search(r'\bv_mfma_f32_16x16x4_?f32', ln):
            r["mfma"] += 1
        m = re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', ln)
        if m:
            r["scratch"] = int(m.group(1))
        m = re.search(r'\.amdhsa_group_segment_fixed_size\s+(\d+)', ln)
        if m:
            r["lds"] = int(m.group(1))
    return res


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if HIPCC is None:
        pytest.fail("hipcc is required to cross-compile the gfx950 listings")
    from osrl_amd.build import FILE_FLAGS, FLAGS
    d = tmp_path_factory.mktemp("isa_wide")
    procs = {}
    for name in ("mlp", "act"):
        out = str(d / f"{name}.s")
        cmd = [HIPCC] + FLAGS + FILE_FLAGS.get(f"{name}.hip", []) + \
            ["-S", "--cuda-device-only", os.path.join(ROOT, "osrl_amd", "csrc", f"{name}.hip"), "-o", out]
        procs[name] = (subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL), out)
    res = {}
    for name, (p, out) in procs.items():
        assert p.wait() == 0, f"hipcc -S failed on {name}.hip"
        res.update(_kernels(out))
    return res


WIDE = [f"wide_layer_kernelILi{r}ELi{c}E" for r in (1, 2) for c in (1, 2, 4)]
ACT = [f"policy_act_kernelILi{r}ELi{w}E" for r in (1, 4) for w in (512, 1024)]


def _find(listings, needle):
    hits = [k for k in listings if needle in k]
    assert len(hits) == 1, (needle, hits)
    return listings[hits[0]]


@pytest.mark.parametrize("needle", WIDE + ["wide_dy_kernel"])
def test_wide_kernels_have_no_scratch(listings, needle):
    assert _find(listings, needle)["scratch"] == 0, needle


@pytest.mark.parametrize("needle", WIDE)
def test_wide_layer_kernels_run_on_fp32_mfma(listings, needle):
    r = _find(listings, needle)
    assert r["mfma"] > 0 and r["lds"] == 0, (needle, r)  # (all of its LDS is dynamic: checked below)


@pytest.mark.parametrize("needle", ACT)
def test_act_gemv_kernels_fit(listings, needle):
    r = _find(listings, needle)
    assert r["scratch"] == 0 and 0 < r["lds"] <= 160 * 1024, (needle, r)


def test_wide_layer_launches_request_at_most_160_kb():
    """The LDS the wide path's launcher asks for, at every (K, N) up to OSRL_MAX_WIDTH: one [16 or 32, K + 8] A tile."""
    from osrl_amd import _lib as L
    lib = L.load()
    worst = 0
    for K in range(1, L.MAX_WIDTH + 1):
        for N in (1, 16, 17, 200, 256, 257, 750, 1024):
            got = int(lib.osrl_mlp_wide_lds_bytes(K, N))
            gcols = 256 if N > 255 else ((N + 15) // 16) * 16
            lda = max(max((K + 15) // 16 * 16, gcols), 64) + 8
            assert got == 4 * (16 if K > 512 else 32) * lda, (K, N, got)
            worst = max(worst, got)
    assert worst <= 160 * 1024
    assert lib.osrl_mlp_wide_lds_bytes(L.MAX_WIDTH + 1, 16) == 0


def test_limits_of_the_python_layer():
    from osrl_amd import _lib as L
    from osrl_amd.engine import plan as P
    assert L.MAX_WIDTH == 1024 and L.TILE_MAX_WIDTH == P.TILE_MAX_WIDTH == 448 and L.MAX_LAYERS == 4
    hdr = open(os.path.join(ROOT, "include", "osrl_amd.h")).read()
    assert re.search(r"#define OSRL_MAX_WIDTH 1024\b", hdr)


def _ctors():
    from osrl_amd.algorithms import BC, BCQL, BEARL, CPQ, COptiDICE
    import numpy as np
    s = np.ones(5, np.float32)
    return {
        "BC": lambda a: BC(5, 2, 1.0, a_hidden_sizes=a, device="cuda"),
        "CPQ": lambda a: CPQ(5, 2, 1.0, a_hidden_sizes=a, c_hidden_sizes=[64, 64], device="cuda"),
        "CPQ.critic": lambda a: CPQ(5, 2, 1.0, c_hidden_sizes=a, device="cuda"),
        "CPQ.vae": lambda a: CPQ(5, 2, 1.0, vae_hidden_sizes=a[0], device="cuda"),
        "BCQL": lambda a: BCQL(5, 2, 1.0, c_hidden_sizes=a, device="cuda"),
        "BEARL": lambda a: BEARL(5, 2, 1.0, a_hidden_sizes=a, device="cuda"),
        "COptiDICE": lambda a: COptiDICE(5, 2, 1.0, "softchi", 0.1, s, s[:2], c_hidden_sizes=a, device="cuda"),
    }


@pytest.mark.parametrize("which", ["BC", "CPQ", "CPQ.critic", "CPQ.vae", "BCQL", "BEARL", "COptiDICE"])
def test_constructors_refuse_width_1025_and_five_layers_without_a_device(which):
    make = _ctors()[which]
    with pytest.raises(ValueError, match="1025 wide; at most 1024"):
        make([1025, 64])
    if which != "CPQ.vae":  # (the VAE's depth is fixed: its hidden size is one number)
        with pytest.raises(ValueError, match="5 Linear layers; at most 4"):
            make([64, 64, 64, 64])


@pytest.mark.parametrize("which", ["BC", "CPQ", "CPQ.critic", "CPQ.vae", "BCQL", "BEARL", "COptiDICE"])
def test_constructors_accept_width_1024(which):
    """The limit check passes at 1024 units and 4 layers; without a GPU the constructor then stops at the device request."""
    try:
        _ctors()[which]([1024, 1024, 1024] if which != "CPQ.vae" else [1024])
    except RuntimeError as e:
        assert "no HIP device visible" in str(e), e


def test_the_engines_net_descriptors_take_1024_and_refuse_1025():
    import torch
    from osrl_amd.engine import core
    from osrl_amd.engine.core import FlatGroup, LayerRef, NetDesc
    old = core.LAYOUT_ONLY_OK
    core.LAYOUT_ONLY_OK = True
    try:
        for w, ok in ((1024, True), (1025, False)):
            g = FlatGroup("t", "cpu")
            g.add("w0", (w, 8)); g.mark_weight("w0"); g.add("b0", (w,))
            g.add("w1", (1, w)); g.mark_weight("w1"); g.add("b1", (1,))
            g.finalize()
            refs = [[LayerRef(g.view("w0"), g.view("b0"), g, "w0", "b0"), LayerRef(g.view("w1"), g.view("b1"), g, "w1", "b1")]]
            if ok:
                d = NetDesc(refs, ["relu", "id"])
                assert d.wide and d.c.dims[1] == 1024
            else:
                with pytest.raises(ValueError, match="1025 > 1024"):
                    NetDesc(refs, ["relu", "id"])
    finally:
        core.LAYOUT_ONLY_OK = old
    del torch


WIDE_ROWS = [
    # (chooser, shape) -- C2's shape with a [1024, 1024] critic and 750 / 800 VAEs, C3's BCQ-Lag with [512, 512] / 750
    ("cpq", dict(od=76, ad=2, B=2048, vae_hidden=750, N=10, c_hidden=[1024, 1024])),
    ("cpq", dict(od=76, ad=2, B=2048, vae_hidden=800, N=10, c_hidden=[1024, 1024])),
    ("cpq", dict(od=76, ad=2, B=2048, vae_hidden=400, N=10, c_hidden=[512, 512])),
    ("cpq", dict(od=17, ad=6, B=2048, vae_hidden=1024, N=10, c_hidden=[1024, 1024])),
    ("bcql", dict(od=33, ad=8, B=4096, vae_hidden=750, N=10)),
    ("bcql", dict(od=33, ad=8, B=4096, vae_hidden=800, N=10)),
]


@pytest.mark.parametrize("chooser,kw", WIDE_ROWS)
def test_plan_rows_for_wide_shapes_give_forms_that_exist(chooser, kw):
    """The fused-kernel-only forms (all-CU VAE launches, OOD row sets, shared-observation tiles) are off wherever a net they
    run on is wider than 448; what stays on (action draws as tails, 80 x 80 dW tiles, pipelined graphs) exists on the wide
    path: tails as launches behind it, the dW tile kernels at any width."""
    from osrl_amd.engine import plan as P
    if chooser == "cpq":
        p = P.cpq_plan(**kw)
        c_wide = not P.tile_widths(*kw["c_hidden"])
        assert not p.vae_ns or P.tile_widths(kw["vae_hidden"])
        assert not p.ood_rows or not c_wide
        assert not p.ood_share or (P.tile_widths(kw["vae_hidden"]) and not c_wide)
        if not P.tile_widths(kw["vae_hidden"]):
            assert not p.vae_ns and not p.ood_share
        if c_wide:
            assert not p.ood_rows and not p.ood_share
        assert p.vae_dw_tile == (5 if kw["vae_hidden"] % 80 == 0 else 0)
        assert p.head_tails == (kw["N"] * kw["ad"] <= 32)
    else:
        p = P.bcql_plan(**kw)
        assert not p.vae_ns
        assert p.vae_dw_tile == (5 if kw["vae_hidden"] % 80 == 0 else 0)


def test_bc_one_launch_is_a_tile_shape_rule():
    from osrl_amd.engine import plan as P
    assert P.bc_one_launch_shape([8, 256, 256, 2]) and P.bc_one_launch_shape([8, 448, 2])
    assert not P.bc_one_launch_shape([8, 1024, 1024, 1024, 2]) and not P.bc_one_launch_shape([8, 449, 2])


def test_pinned_rows_are_unchanged():
    from osrl_amd.engine import plan as P
    for name, (fn, kw, want) in P.PINNED.items():
        assert fn(**kw) == want, name
