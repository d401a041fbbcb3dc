"""Compile-time budgets of the pessimistic environment step (csrc/model_env.hip, flag kPess) and of the compaction
(csrc/compact.hip); CPU only: hipcc cross-compiles gfx950 assembly without a GPU.  The eight new kernels -- by-value and
descriptor-pointer twins of halt_env_kernel, halt_rec_kernel, halt_env_gauss_kernel and halt_rec_gauss_kernel -- are
present once each, use no scratch, stay within 160 KB of static LDS and run their layers on fp32 MFMA; the two
compaction kernels are present."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
CSRC = os.path.join(ROOT, "osrl_amd", "csrc")


def listing(tmp, source):
    if HIPCC is None:
        pytest.fail("hipcc is required to cross-compile the gfx950 listing")
    from osrl_amd.build import FILE_FLAGS, FLAGS, SOURCES
    assert source in SOURCES
    out = str(tmp / source.replace(".hip", ".s"))
    cmd = [HIPCC] + FLAGS + FILE_FLAGS.get(source, []) + ["-S", "--cuda-device-only", os.path.join(CSRC, source), "-o", out]
    assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    res, kern = {}, None
    for ln in open(out):
        m = re.match(r'^(_Z\w+):', ln)
        if m:
            kern = m.group(1)
            res[kern] = dict(mfma=0, scratch=-1, lds=-1, vgpr=-1)
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
        for key, pat in (("scratch", r'\.amdhsa_private_segment_fixed_size\s+(\d+)'),
                         ("lds", r'\.amdhsa_group_segment_fixed_size\s+(\d+)'), ("vgpr", r'^;\s*NumVgprs:\s*(\d+)')):
            m = re.search(pat, ln)
            if m:
                r[key] = int(m.group(1))
    return res


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return listing(tmp_path_factory.mktemp("isa_halt_model_env"), "model_env.hip")


NEW = ["halt_env_kernelE", "halt_env_kernel_pE", "halt_rec_kernelE", "halt_rec_kernel_pE", "halt_env_gauss_kernelE",
       "halt_env_gauss_kernel_pE", "halt_rec_gauss_kernelE", "halt_rec_gauss_kernel_pE"]
OLD = ["model_env_kernelE", "model_env_kernel_pE", "model_rec_kernelE", "model_rec_kernel_pE", "model_env_gauss_kernelE",
       "model_env_gauss_kernel_pE", "model_rec_gauss_kernelE", "model_rec_gauss_kernel_pE", "model_branch_kernelE"]


def test_every_kernel_present_once(kernels):
    for n in NEW + OLD:
        assert sum(n in k for k in kernels) == 1, (n, list(kernels))
    for n in OLD:  # the names the existing kernels are found by match none of the new ones
        assert not any(n in k for k in kernels if "halt_" in k), n


@pytest.mark.parametrize("name", NEW)
def test_no_scratch_lds_within_160k_fp32_mfma(kernels, name):
    k = next(v for kk, v in kernels.items() if name in kk)
    print(name, k)
    assert k["scratch"] == 0, (name, k)
    assert 0 <= k["lds"] <= 160 * 1024, (name, k)
    assert k["mfma"] >= 4, k


def test_compaction_kernels_present(tmp_path):
    res = listing(tmp_path, "compact.hip")
    for n in ("compact_scan_kernelE", "compact_copy_kernelE"):
        k = [v for kk, v in res.items() if n in kk]
        assert len(k) == 1, (n, list(res))
        assert k[0]["scratch"] == 0, (n, k[0])
