"""Compile-time budgets of the Gaussian environment step and recording step (csrc/model_env.hip; CPU only: hipcc
cross-compiles gfx950 assembly without a GPU): the four kernels -- by-value and descriptor-pointer twins of
model_env_gauss_kernel and model_rec_gauss_kernel -- are present once each, keep the 64 member outputs per thread plus the
running maximum of the predicted standard deviation in registers (no scratch), stay within 160 KB of static LDS with the
extra variance tile, and run their layers on fp32 MFMA."""
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
    out = str(tmp_path_factory.mktemp("isa_gauss_model_env") / "model_env.s")
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


NEW = ["model_env_gauss_kernelE", "model_env_gauss_kernel_pE", "model_rec_gauss_kernelE", "model_rec_gauss_kernel_pE"]
OLD = ["model_env_kernelE", "model_env_kernel_pE", "model_rec_kernelE", "model_rec_kernel_pE", "model_branch_kernelE",
       "dyn_prepare_kernel"]


def test_every_kernel_present_once(kernels):
    for n in NEW + OLD:
        assert sum(n in k for k in kernels) == 1, (n, list(kernels))
    for n in OLD:  # the names the existing kernels are found by match none of the new ones
        assert not any(n in k for k in kernels if "gauss" in k), n


@pytest.mark.parametrize("name", NEW)
def test_no_scratch_lds_within_160k_fp32_mfma(kernels, name):
    k = next(v for kk, v in kernels.items() if name in kk)
    assert k["scratch"] == 0, (name, k)
    assert 0 <= k["lds"] <= 160 * 1024, (name, k)
    assert k["mfma"] >= 4, k
    assert k["lds"] >= 3 * 16 * 512 * 4 + 16 * 256 * 4, k  # the three activation tiles and the variance tile are in LDS
