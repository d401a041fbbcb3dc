"""CPU-side checks of the planner's CEM refinement (csrc/plan_refine.hip ``osrl_plan_refit``, engine/mpc.py
``check_refine``): every refusal before any device work (stubs: no device here), the C ABI, and the compile-time budgets
of the two kernels."""
import os
import re
import shutil
import subprocess

import pytest

from test_plan_cpu import _stub_menv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = (dict(refine_rounds=-1), dict(num_elites=0), dict(num_elites=21), dict(refine_momentum=1.0),
       dict(refine_momentum=-0.1), dict(refine_momentum=float("nan")), dict(min_std=-0.1), dict(min_std=float("inf")))


def test_check_refine():
    from osrl_amd.engine.mpc import check_refine
    assert check_refine(20) == 2 and check_refine(5) == 1 and check_refine(1024, refine_rounds=3, num_elites=1024) == 1024
    assert check_refine(2) == 1 and check_refine(20, "bcql") == 2  # (without rounds nothing is refused for K or BCQ-L)
    assert check_refine(20, "bcql", z=object(), refine_rounds=1) == 2
    for kw in BAD:
        with pytest.raises(ValueError):
            check_refine(20, **kw)
    for K, kind in ((2, "bc"), (1, "cpq"), (20, "bcql")):
        with pytest.raises(ValueError):
            check_refine(K, kind, refine_rounds=1)


@pytest.mark.parametrize("kw", BAD + (dict(refine_rounds=1, num_elites=6),))
def test_the_planner_and_the_trainers_refuse_before_they_build_anything(kw):
    """A stub model without attributes: anything past the checks would be an AttributeError."""
    from osrl_amd.algorithms import BCQLTrainer, BCTrainer
    from osrl_amd.engine.mpc import ModelPlanner
    E = 20  # 4 slots of 5 candidates
    with pytest.raises(ValueError):
        ModelPlanner(object(), _stub_menv(E), "bc", num_envs=4, horizon=3, **kw)
    with pytest.raises(ValueError):
        BCTrainer.__new__(BCTrainer).planner(_stub_menv(E), 4, 3, **kw)
    with pytest.raises(ValueError):
        ModelPlanner(object(), _stub_menv(8), "bc", num_envs=4, horizon=3, refine_rounds=1)  # K = 2
    with pytest.raises(ValueError, match="BCQ-L"):
        BCQLTrainer.__new__(BCQLTrainer).planner(_stub_menv(20), 4, 3, refine_rounds=1)


def test_the_header_declares_the_entry_and_it_refuses_bad_arguments():
    from osrl_amd import _lib as L
    from osrl_amd.build import SOURCES
    assert "plan_refine.hip" in SOURCES
    hdr = open(os.path.join(ROOT, "include", "osrl_amd.h")).read()
    m = re.search(r"\bint\s+osrl_plan_refit\s*\((.*?)\)\s*;", hdr, re.S)
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    assert len(params) == 18 == len(L.PROTOTYPES["osrl_plan_refit"])
    one = 0x1000  # (never dereferenced: every call below fails a check first)
    ok = [one, one, one, one, one, 2, 5, 3, 2, 1, 0.0, 0.05, 1, one, 0, None, one, None]
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, 0), (6, 0), (6, 1025), (7, 0), (7, 65537),
                   (8, 0), (9, 0), (10, 1.0), (10, -0.5), (10, float("nan")), (11, -1.0), (11, float("inf")), (12, -1),
                   (12, 65536), (13, None), (16, None), (5, 1 << 30)):
        args = list(ok)
        args[i] = bad
        assert L.load().osrl_plan_refit(*args) == -1, (i, bad)


def test_no_scratch_and_the_lds_of_design_md(tmp_path):
    from osrl_amd.build import FILE_FLAGS, FLAGS
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.fail("hipcc is required to cross-compile the gfx950 listing")
    out = str(tmp_path / "plan_refine.s")
    cmd = [hipcc] + FLAGS + FILE_FLAGS["plan_refine.hip"] + ["-S", "--cuda-device-only",
                                                             os.path.join(ROOT, "osrl_amd", "csrc", "plan_refine.hip"), "-o", out]
    assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    res, kern = {}, None
    for ln in open(out):
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', ln)
        if m:
            kern = res.setdefault(m.group(1), {})
            continue
        for key, field in (("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size")):
            m = re.search(r'\.amdhsa_' + field + r'\s+(\d+)', ln)
            if m and kern is not None:
                kern[key] = int(m.group(1))
    refit = next(v for k, v in res.items() if "plan_refit_kernel" in k)
    redraw = next(v for k, v in res.items() if "plan_redraw_kernel" in k)
    assert len(res) == 2, list(res)
    assert refit["scratch"] == 0 and redraw["scratch"] == 0
    # J, C and the index list (4 KB each), the classes (1 KB), and the few words of the counting barrier
    assert redraw["lds"] == 0 and 13312 <= refit["lds"] <= 13312 + 256
