"""Compile-time guards for the CDT act latency path (csrc/cdt_act.hip; CPU only: hipcc cross-compiles gfx950 assembly
without a GPU): every kernel runs without scratch, its LDS (all static: the launches request no dynamic LDS) stays
within 160 KB per workgroup, and the row-tile projection kernel runs on fp32 MFMA.  Also: the ctypes mirrors of the
new descriptor structs match the C header, and the domain check names its limits without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
SRC = os.path.join(ROOT, "osrl_amd", "csrc", "cdt_act.hip")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.fail("hipcc is required to cross-compile the gfx950 listing")
    from osrl_amd.build import FILE_FLAGS, FLAGS
    out = str(tmp_path_factory.mktemp("isa_cdt_act") / "cdt_act.s")
    cmd = [HIPCC] + FLAGS + FILE_FLAGS.get("cdt_act.hip", []) + ["-S", "--cuda-device-only", SRC, "-o", out]
    assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    res, kern = {}, None
    for ln in open(out):
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
        if re.search(r'\bv_mfma_f32_16x16x4', ln):
            r["mfma"] += 1
        m = re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', ln)
        if m:
            r["scratch"] = int(m.group(1))
        m = re.search(r'\.amdhsa_group_segment_fixed_size\s+(\d+)', ln)
        if m:
            r["lds"] = int(m.group(1))
    return res


NAMES = ["cdt_act_ingest_kernel", "cdt_act_linear_kernel", "cdt_act_attn_kernel", "cdt_act_head_kernel"]


def test_every_kernel_present(kernels):
    for n in NAMES:
        assert sum(n in k for k in kernels) == 1, (n, list(kernels))


@pytest.mark.parametrize("name", NAMES)
def test_no_scratch_and_lds_within_160k(kernels, name):
    k = next(v for kk, v in kernels.items() if name in kk)
    assert k["scratch"] == 0, (name, k)
    assert 0 <= k["lds"] <= 160 * 1024, (name, k)


def test_row_tile_projection_on_fp32_mfma(kernels):
    k = next(v for kk, v in kernels.items() if "cdt_act_linear_kernel" in kk)
    assert k["mfma"] >= 4, k


def test_descriptor_mirrors_match_the_header(tmp_path):
    import ctypes as C
    from osrl_amd import _lib as L
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src, exe = str(tmp_path / "sz.c"), str(tmp_path / "sz")
    pairs = [("osrl_cdt_policy_t", L.CdtPolicyT), ("osrl_cdt_layer_t", L.CdtLayerT)]
    with open(src, "w") as f:
        f.write('#include "osrl_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n')
        for cname, cls in pairs:
            f.write(f'  printf("%zu", sizeof({cname}));\n')
            for fname, _ in cls._fields_:
                f.write(f'  printf(" %zu", offsetof({cname}, {fname}));\n')
            f.write('  printf("\\n");\n')
        f.write("  return 0;\n}\n")
    subprocess.run([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True,
                   capture_output=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line, (cname, cls) in zip(out, pairs):
        want = [C.sizeof(cls)] + [getattr(cls, fname).offset for fname, _ in cls._fields_]
        assert [int(x) for x in line.split()] == want, cname


def test_domain_limits_are_named():
    from types import SimpleNamespace
    from osrl_amd.engine.cdt_act import unsupported
    base = dict(seq_repeat=4, seq_len=20, cost_prefix=False, embedding_dim=256, num_heads=8, action_head_layers=1,
                action_dim=3)
    assert unsupported(SimpleNamespace(**base)) is None
    assert unsupported(SimpleNamespace(**dict(base, seq_len=64))) is None  # S = 256
    assert "257 tokens" in unsupported(SimpleNamespace(**dict(base, seq_len=64, cost_prefix=True)))
    assert unsupported(SimpleNamespace(**dict(base, embedding_dim=512, num_heads=4))) is None
    assert "embedding_dim 640" in unsupported(SimpleNamespace(**dict(base, embedding_dim=640)))
    assert "head_dim 256" in unsupported(SimpleNamespace(**dict(base, embedding_dim=512, num_heads=2)))
