"""CPU-side checks of the on-device collection: the new descriptor's layout, the header as C99, the numpy restatement
(tests/collect_oracle.py) against the chained scalar environment, ``merge_datasets``, and ``collect``'s refusal."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gcc():
    import shutil
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    return gcc


def test_collect_descriptor_layout_matches_the_compiled_header():
    """sizeof / offsets of ``osrl_collect_t`` as gcc sees include/osrl_amd.h == the ctypes mirror ``_lib.CollectT``."""
    import ctypes as C
    import subprocess
    import tempfile
    from osrl_amd import _lib as L
    gcc = _gcc()
    cls = L.CollectT
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sz.c"), os.path.join(d, "sz")
        with open(src, "w") as f:
            f.write('#include "osrl_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n')
            f.write('  printf("%zu", sizeof(osrl_collect_t));\n')
            for fname, _ in cls._fields_:
                f.write(f'  printf(" %zu", offsetof(osrl_collect_t, {fname}));\n')
            f.write('  printf("\\n");\n  return 0;\n}\n')
        subprocess.run([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True,
                       capture_output=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(cls)] + [getattr(cls, fname).offset for fname, _ in cls._fields_]
    assert got == want and got[0] == 12 * 8 + 2 * 4, (got, want)
    assert L.PROTOTYPES["osrl_env_collect"][1]._type_ is cls


def test_header_with_collect_entry_point_is_plain_c():
    import subprocess
    import tempfile
    gcc = _gcc()
    hdr = os.path.join(ROOT, "include", "osrl_amd.h")
    assert re.search(r"\bint\s+osrl_env_collect\s*\(", open(hdr).read())
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "use.c")
        with open(src, "w") as f:
            f.write('#include "osrl_amd.h"\n'
                    "int (*const collect_fn)(const osrl_env_t*, const osrl_collect_t*, const float*, float*, float*, "
                    "int32_t, float*, int32_t, void*) = &osrl_env_collect;\n"
                    "int main(void) { osrl_collect_t c; c.eps_in = 0; c.stream_id = 13u; return c.eps_in != 0; }\n")
        r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-Wno-pedantic",
                            "-I", os.path.dirname(hdr), "-c", src, "-o", os.path.join(d, "use.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_oracle_collection_without_noise_is_the_chained_scalar_env():
    from collect_oracle import collect
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    od, ad, E, EL, base = 5, 3, 4, 7, 20
    mk = lambda: SyntheticSafeEnv(od, ad, EL, seed=3, init_noise=0.5)  # noqa: E731
    W = np.random.RandomState(0).randn(od, ad)
    pol = lambda o: 2.0 * np.tanh(o[:, :od] @ W)  # noqa: E731  (acts beyond the clip in places)
    nan = np.full((EL, E, ad), np.nan)
    got = collect(mk, pol, base, E, EL, sigma=0.0, eps=nan, gamma=0.9, cost_scale=2.0)
    d = got.dataset
    assert d["observations"].shape == (E * EL, od) and d["actions"].shape == (E * EL, ad)
    assert all(v.dtype == np.float32 for v in d.values()) and (np.abs(d["actions"]) <= 1.0).all()
    assert (np.abs(d["actions"]) == 1.0).any()
    for e in range(E):
        env = mk()
        o, _ = env.reset(seed=base + e)
        ret = cost = dret = dcost = 0.0
        for t in range(EL):
            row = e * EL + t
            np.testing.assert_array_equal(d["observations"][row], o)
            a = np.clip(pol(o[None].astype(np.float64))[0].astype(np.float32), -1, 1)
            np.testing.assert_array_equal(d["actions"][row], a)
            o, r, term, trunc, info = env.step(a)
            np.testing.assert_array_equal(d["next_observations"][row], o)
            assert d["rewards"][row] == np.float32(r) and d["costs"][row] == info["cost"]
            assert d["terminals"][row] == 0 and d["timeouts"][row] == float(trunc) == float(t == EL - 1)
            r32 = float(np.float32(r))
            ret, cost = ret + r32, cost + 2.0 * info["cost"]
            dret, dcost = dret + 0.9 ** t * r32, dcost + 0.9 ** t * 2.0 * info["cost"]
        assert got.lengths[e] == EL and abs(got.returns[e] - ret) < 1e-12 and got.cost_returns[e] == cost
        assert abs(got.disc_returns[e] - dret) < 1e-12 and abs(got.disc_cost_returns[e] - dcost) < 1e-12
    # noise: sigma_e * eps is added before the clip, and only where sigma_e != 0
    eps = np.random.RandomState(1).randn(EL, E, ad)
    eps[:, 0] = np.nan
    noisy = collect(mk, pol, base, E, EL, sigma=[0.0, 0.3, 0.3, 0.3], eps=eps)
    np.testing.assert_array_equal(noisy.dataset["actions"][:EL], d["actions"][:EL])
    s1 = noisy.dataset["observations"][EL:2 * EL].astype(np.float64)
    want = np.clip((pol(s1) + 0.3 * eps[:, 1]).astype(np.float32), -1, 1)
    np.testing.assert_array_equal(noisy.dataset["actions"][EL:2 * EL], want)
    with pytest.raises(ValueError):
        collect(mk, pol, base, E, EL, sigma=0.1)


def test_merge_datasets_on_cpu_tensors():
    from osrl_amd.engine.collect import KEYS, merge_datasets
    mk = lambda n, v: {k: torch.full((n, 3) if k.endswith("observations") else (n, 2) if k == "actions" else (n,),  # noqa: E731
                                     float(v)) for k in KEYS}
    a, b = mk(4, 1), mk(6, 2)
    m = merge_datasets([a, b])
    assert set(m) == set(KEYS)
    for k in KEYS:
        assert m[k].shape[0] == 10 and m[k].shape[1:] == a[k].shape[1:]
        assert (m[k][:4] == 1).all() and (m[k][4:] == 2).all()
        assert m[k].data_ptr() not in (a[k].data_ptr(), b[k].data_ptr())
    with pytest.raises(ValueError):
        merge_datasets([])


def test_collect_refuses_other_environments_before_touching_a_device():
    import osrl_amd.engine.core as core
    from osrl_amd.algorithms import BC, BCTrainer, CDTTrainer
    from osrl_amd.common.logger import DummyLogger
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    core.LAYOUT_ONLY_OK = True
    try:
        m = BC(6, 2, 1.0, [16, 16], 10, device="cpu")
        tr = BCTrainer(m, SyntheticSafeEnv(6, 2, 10), DummyLogger(), device="cpu")
        with pytest.raises(TypeError, match="VecSyntheticSafeEnv"):
            tr.collect(0.1)
        tr.env = [SyntheticSafeEnv(6, 2, 10)]
        with pytest.raises(TypeError, match="VecSyntheticSafeEnv"):
            tr.collect()
    finally:
        core.LAYOUT_ONLY_OK = False
    assert not hasattr(CDTTrainer, "collect")  # CDT as a behaviour policy is out of scope


@pytest.mark.parametrize("shape", [(6, 2, 5), (70, 5, 33)])
def test_trajectory_test_env_keeps_its_margin_at_the_cost_threshold(shape):
    """tests/test_gpu_collect.py compares costs only on rows farther from the threshold than its rounding bound and caps
    the rows left out at 1 %: the numpy environment alone, with that test's env seed and policy, must meet the cap (and
    produce both cost values, or the comparison would be empty)."""
    import test_gpu_collect as T
    from collect_oracle import collect
    from fqe_oracle import policy_action
    od, ad, E = shape
    sd = T.CC.bc_state_dict(od, ad, T.HID, 3)
    pol = policy_action("bc", {k: v.numpy().astype(np.float64) for k, v in sd.items()}, 1.0)
    eps = np.random.RandomState(0).randn(T.EL, E, ad)
    c = collect(lambda: T.make_env(od, ad), lambda o: pol(o, None), T.BASE_SEED, E, T.EL, sigma=0.3, eps=eps)
    d = c.dataset
    env = T.make_env(od, ad)
    b, rb, wb = T.step_bounds(env, d["observations"], d["actions"], d["next_observations"])
    sw = d["next_observations"].astype(np.float64) @ env.w.astype(np.float64)
    near = np.abs(sw - env.COST_THRESHOLD) <= wb
    assert near.mean() <= 0.01 and 0.05 < d["costs"].mean() < 0.95, (near.mean(), d["costs"].mean())
    assert wb.max() < 1e-2 and rb.max() < 1e-2  # (worst-case rounding bounds: far below the spread of s'.w and of the rewards)


def test_collect_kernel_resources():
    """The collecting kernel's code-object metadata (hipcc -S, nothing but the resource fields): no scratch, and few
    enough registers for eight waves per SIMD -- it runs between the policy's launches, one small workgroup per episode."""
    import shutil
    import subprocess
    import tempfile
    from osrl_amd.build import FLAGS
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "collect.s")
        subprocess.run([hipcc] + FLAGS + ["-S", "--cuda-device-only", os.path.join(ROOT, "osrl_amd", "csrc", "collect.hip"),
                        "-o", out], check=True, capture_output=True)
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    blocks = [b for b in meta.split("  - .agpr_count:") if "env_collect_kernel" in b]
    assert len(blocks) == 1
    field = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blocks[0]).group(1))  # noqa: E731
    assert field("private_segment_fixed_size") == 0 and field("vgpr_count") <= 64 and field("sgpr_count") <= 104
    assert field("group_segment_fixed_size") == (256 + 64 + 8) * 4
