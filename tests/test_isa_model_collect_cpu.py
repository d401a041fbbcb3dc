"""Compile-time budgets of the recording step and the branch-start kernel (csrc/model_env.hip; CPU only: hipcc
cross-compiles gfx950 assembly without a GPU), read from the listing the way tests/test_isa_model_env_cpu.py reads it: the
recording kernel and its descriptor-pointer twin keep the step's 64 member outputs per thread in registers (no scratch),
stay within 160 KB of static LDS and run their layers on fp32 MFMA; the two evaluating kernels beside them keep their
names and their budgets.  Register and LDS budgets only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
SRC = os.path.join(ROOT, "osrl_amd", "csrc", "model_env.hip")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.fail("hipcc is required to cross-compile the gfx950 listing")
    from osrl_amd.build import FILE_FLAGS, FLAGS, SOURCES
    assert "model_env.hip" in SOURCES
    out = str(tmp_path_factory.mktemp("isa_model_collect") / "model_env.s")
    cmd = [HIPCC] + FLAGS + FILE_FLAGS.get("model_env.hip", []) + ["-S", "--cuda-device-only", SRC, "-o", out]
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


NEW = ["model_rec_kernelE", "model_rec_kernel_pE", "model_branch_kernelE"]
OLD = ["model_env_kernelE", "model_env_kernel_pE"]


def test_every_kernel_present_once(kernels):
    for n in NEW + OLD:
        assert sum(n in k for k in kernels) == 1, (n, list(kernels))
    for n in NEW:  # the names the evaluating kernels are found by match none of the new ones
        assert not any(o in n for o in OLD)


@pytest.mark.parametrize("name", NEW + OLD)
def test_no_scratch_and_lds_within_160k(kernels, name):
    k = next(v for kk, v in kernels.items() if name in kk)
    assert k["scratch"] == 0, (name, k)
    assert 0 <= k["lds"] <= 160 * 1024, (name, k)


@pytest.mark.parametrize("name", NEW[:2])
def test_recording_layers_on_fp32_mfma(kernels, name):
    k = next(v for kk, v in kernels.items() if name in kk)
    assert k["mfma"] >= 4, k
    assert k["lds"] >= 3 * 16 * 512 * 4, k  # the input tile and the two activation tiles are in LDS
