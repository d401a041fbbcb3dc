"""CPU-side checks of the lockstep CDT act path: the five ``osrl_cdt_policy_*_n`` entry points are declared in the
header, mirrored in ``_lib.PROTOTYPES`` and exported by the library; the extended kernels still compile for gfx950
without scratch and within the LDS bound, one symbol each; CDTVecFastPolicy's argument checks raise before any
device call."""
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["osrl_cdt_policy_create_n", "osrl_cdt_policy_io_n", "osrl_cdt_policy_reset_n", "osrl_cdt_policy_step_n",
       "osrl_cdt_policy_window_n"]


def test_header_prototypes_and_library_agree_on_the_new_entry_points():
    import ctypes as C
    from osrl_amd import _lib as L
    from osrl_amd import build as b
    hdr = open(os.path.join(ROOT, "include", "osrl_amd.h")).read()
    want_args = {"osrl_cdt_policy_create_n": 4, "osrl_cdt_policy_io_n": 5, "osrl_cdt_policy_reset_n": 2,
                 "osrl_cdt_policy_step_n": 3, "osrl_cdt_policy_window_n": 9}
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/osrl_amd.h"
        assert len(m.group(1).split(",")) == want_args[name] == len(L.PROTOTYPES[name]), name
    m = re.search(r"#define\s+OSRL_CDT_POLICY_MAX_ENVS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == L.CDT_POLICY_MAX_ENVS == 64
    lib = C.CDLL(b.build())
    for name in NEW + ["osrl_cdt_policy_destroy"]:
        assert hasattr(lib, name), f"libosrl_amd.so does not export {name}"


def test_header_stays_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is required to compile the header as C")
    src = str(tmp_path / "h.c")
    with open(src, "w") as f:
        f.write('#include "osrl_amd.h"\nint (*p)(void*, int32_t, void*) = osrl_cdt_policy_step_n;\n'
                "int n = OSRL_CDT_POLICY_MAX_ENVS;\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                    str(tmp_path / "h.o")], check=True, capture_output=True)


def test_extended_kernels_one_symbol_no_scratch_lds_bound(tmp_path):
    from osrl_amd.build import FILE_FLAGS, FLAGS
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.fail("hipcc is required to cross-compile the gfx950 listing")
    out = str(tmp_path / "cdt_act.s")
    cmd = [hipcc] + FLAGS + FILE_FLAGS.get("cdt_act.hip", []) + \
        ["-S", "--cuda-device-only", os.path.join(ROOT, "osrl_amd", "csrc", "cdt_act.hip"), "-o", out]
    assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    text = open(out).read()
    kern = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    assert len(kern) == 4, kern  # the episode dimension added no kernel: a step stays 2 + 5 * layers launches
    for name in ("cdt_act_ingest_kernel", "cdt_act_linear_kernel", "cdt_act_attn_kernel", "cdt_act_head_kernel"):
        assert sum(name in k for k in kern) == 1, (name, kern)
    blocks = re.findall(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    assert len(blocks) == 4
    for name, body in blocks:
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0, name
        assert 0 <= int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", body).group(1)) <= 160 * 1024, name
    # the projections stay on fp32 MFMA and the device side neither polls nor sleeps
    assert len(re.findall(r"\bv_mfma_f32_16x16x4", text)) >= 4
    assert not re.search(r"\bs_sleep\b", text)


def _stub_policy(N=3, od=4, ad=2):
    """A CDTVecFastPolicy without a device: every C call, and the model's repack(), fail the test."""
    from osrl_amd.engine.cdt_act import CDTVecFastPolicy

    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"device call {name} before the argument checks")

    p = object.__new__(CDTVecFastPolicy)
    p.num_envs, p.od, p.ad, p.T = N, od, ad, 5
    p._h, p._lib, p.model = None, Boom(), Boom()
    p._t, p._episode_len = 0, 10
    p._raw_stream, p._dev_index = None, 0
    return p


def test_num_envs_range_is_checked_first():
    from osrl_amd.engine.cdt_act import MAX_ENVS, CDTVecFastPolicy
    stub = SimpleNamespace()  # nothing of the model may be touched before num_envs is checked
    assert MAX_ENVS == 64
    for bad in (0, -1, 65):
        with pytest.raises(ValueError, match="1 .. 64"):
            CDTVecFastPolicy(stub, bad)
    for bad in (2.0, "4", None, True):
        with pytest.raises(ValueError, match="integer"):
            CDTVecFastPolicy(stub, bad)
    # inside the range, the domain check names its limit as the one-episode class does
    far = SimpleNamespace(seq_repeat=4, seq_len=64, cost_prefix=True, embedding_dim=256, num_heads=8,
                          action_head_layers=1, action_dim=3)
    with pytest.raises(NotImplementedError, match="257 tokens"):
        CDTVecFastPolicy(far, 8)


def test_shapes_are_checked_before_any_device_call():
    p = _stub_policy()
    N, od, ad = 3, 4, 2
    obs, rew, cost = np.zeros((N, od), np.float32), np.zeros(N), np.zeros(N)
    p._h = object()  # open
    for bad in (np.zeros(od), np.zeros((N + 1, od)), np.zeros((N, od + 1)), 0.0):
        with pytest.raises(ValueError, match="obs of shape"):
            p.reset(bad, 1.0, 1.0)
        with pytest.raises(ValueError, match="obs of shape"):
            p.step(bad, rew, cost)
    for bad in (np.zeros(N + 1), np.zeros((N, 1)), [1.0, 2.0]):
        with pytest.raises(ValueError, match="target_return"):
            p.reset(obs, bad, 1.0)
        with pytest.raises(ValueError, match="target_cost"):
            p.reset(obs, 1.0, bad)
    for bad in (0.0, np.zeros(N - 1), np.zeros((N, 1))):
        with pytest.raises(ValueError, match="reward of shape"):
            p.step(obs, bad, cost)
        with pytest.raises(ValueError, match="cost of shape"):
            p.step(obs, rew, bad)
    for bad in (np.zeros(ad), np.zeros((N, ad + 1)), np.zeros((N - 1, ad))):
        with pytest.raises(ValueError, match="action of shape"):
            p.step(obs, rew, cost, action=bad)
    for bad in (True, np.ones(N + 1, bool), np.ones((N, 1), bool)):
        with pytest.raises(ValueError, match="active of shape"):
            p.step(obs, rew, cost, active=bad)
    with pytest.raises(ValueError, match="booleans"):
        p.step(obs, rew, cost, active=np.ones(N))
    with pytest.raises(ValueError, match="outside 0 .. 2"):
        p.window(3)
    p._t = -1
    with pytest.raises(RuntimeError, match="reset"):
        p.step(obs, rew, cost)
    p._t = 9
    with pytest.raises(RuntimeError, match="episode is over"):
        p.step(obs, rew, cost)
    p._h = None
    with pytest.raises(RuntimeError, match="closed"):
        p.reset(obs, 1.0, 1.0)
    p.close()  # closing a closed policy is a no-op


def test_vector_policy_is_not_copyable():
    import copy
    import pickle
    p = _stub_policy()
    assert copy.deepcopy(p) is None
    assert pickle.loads(pickle.dumps(p)) is None
