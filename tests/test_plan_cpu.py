"""CPU-side checks of planning at act time (csrc/plan.hip, engine/mpc.py ``ModelPlanner``, ``Trainer.planner`` /
``evaluate_planned``): the oracle's select rule on hand-worked cases, every refusal raised before a launch (stubs: no
device here), the C ABI of the two entry points, and the compile-time budgets of the two kernels (hipcc cross-compiles
gfx950 assembly without a GPU)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import plan_cases as P
import plan_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ---- the rule, by hand -----------------------------------------------------------------------------------------------
A0 = np.array([[0.1], [0.2], [0.3], [0.4]])


def test_argmax_over_the_feasible_set_ties_to_the_lowest_k():
    a, k, n, copied = O.select_slot([1.0, 5.0, 5.0, 9.0], [0.0, 0.25, 0.0, 1.25], A0, 1.125, 0.0)
    assert (k, n, copied) == (1, 3, True) and a[0] == 0.2  # (k = 3 has the best return and costs too much)


def test_the_budget_is_inclusive():
    assert O.select_slot([1.0, 2.0], [0.5, 0.5], A0[:2], 0.5, 0.0)[1:3] == (1, 2)
    assert O.select_slot([1.0, 2.0], [0.5, 0.75], A0[:2], 0.5, 0.0)[1:3] == (0, 1)


def test_empty_feasible_set_takes_the_cheapest_then_the_better_return_then_the_lower_k():
    a, k, n, copied = O.select_slot([9.0, 1.0, 2.0, 2.0], [1.5, 1.25, 1.25, 1.25], A0, 1.125, 0.0)
    assert (k, n, copied) == (2, 0, True) and a[0] == 0.3
    assert O.select_slot([9.0, 1.0, 2.0, 2.0], [1.5, 1.25, 1.25, 1.25], A0, 1.125, 3.0)[1] == 2  # (no MPPI without F)


def test_mppi_is_the_softmax_mean_of_the_feasible_rows():
    J, C = [0.0, np.log(3.0), 50.0, 0.0], [0.0, 0.0, 2.0, 0.0]
    a, k, n, copied = O.select_slot(J, C, A0, 1.125, 1.0)
    w = np.array([1.0 / 3.0, 1.0, 0.0, 1.0 / 3.0])
    assert (k, n, copied) == (1, 3, False)
    assert abs(a[0] - float((w * A0[:, 0]).sum() / w.sum())) <= 1e-7  # (the weights are kept in fp32)
    # a spread of 200: every weight but the best one's underflows, the denominator is the best one's 1
    a, k, n, _ = O.select_slot([-200.0, 0.0, -150.0, -199.0], [0.0] * 4, A0, 1.125, 1.0)
    assert k == 1 and n == 4 and a[0] == 0.2


def test_a_nan_is_infeasible_and_never_chosen_unless_all_are():
    a, k, n, _ = O.select_slot([NAN, 1.0, 7.0], [0.0, 0.0, NAN], A0[:3], 1.125, 0.0)
    assert (k, n) == (1, 1)
    a, k, n, _ = O.select_slot([NAN, 1.0, 7.0], [0.0, 2.0, NAN], A0[:3], 1.125, 0.0)
    assert (k, n) == (1, 0)  # (F is empty: the cheapest VALID candidate)
    a, k, n, copied = O.select_slot([NAN, 1.0, NAN], [0.0, NAN, NAN], A0[:3], 1.125, 0.5)
    assert (k, n, copied) == (0, 0, True) and a[0] == 0.1


@pytest.mark.parametrize("name", P.SELECT_CASES)
def test_the_gpu_cases_are_what_they_claim(name):
    for K in P.KS:
        c = P.select_case(name, K, 3)
        assert np.all(c["C"][~np.isnan(c["C"])] * 4 == np.round(c["C"][~np.isnan(c["C"])] * 4))
        assert np.all(c["budget"] - np.floor(c["budget"]) == 0.125)
        _, k, n, copied = O.select(c["J"], c["C"], c["a0"], c["budget"], 0.0)
        assert copied.all()
        if name == "all_feasible":
            assert (n == K).all()
        elif name == "one_feasible_last":
            assert (n == 1).all() and (k == K - 1).all()
        elif name == "none_feasible":
            assert (n == 0).all()
            if K >= 5:
                assert [int(x) for x in k] == [2, 1, 0] and (c["C"].min(1) == 1.25).all()
                assert (c["J"].max(1) == 9.0).all()  # (better returns exist, at a higher cost)
        elif name == "equal_j":
            assert (n >= 1).all() and all(c["C"][s, :k[s]].min(initial=9.0) > c["budget"][s] for s in range(P.N))
        elif name == "spread_200":
            assert (k == K - 1).all() and float(c["J"].max() - c["J"].min()) == (200.0 if K > 1 else 0.0)
        elif name == "all_nan":
            assert (n == 0).all() and (k == 0).all()


def test_the_fanout_oracle():
    s = P.fan_states()
    before = np.full((P.FAN_N * P.FAN_K, P.OD + 1), 7.5, np.float32)
    f = O.fanout(s, P.FAN_K, before, halting=True)
    assert (f["state"][7] == s[1]).all() and (f["obs"][7, :P.OD] == s[1]).all() and f["obs"][7, P.OD] == 7.5
    assert not f["acc"].any() and not f["unc"].any() and (f["disc"] == [0, 0, 1, 0]).all() and (f["halt_step"] == -1).all()
    assert O.fanout(s, P.FAN_K, before, halting=False)["halt_step"] is None


# ---- refusals, before any launch -------------------------------------------------------------------------------------
def _stub_menv(E):
    """A ``ModelVecEnv`` that never saw a device: the checks read ``E`` alone."""
    from osrl_amd.common.model_env import ModelVecEnv
    v = ModelVecEnv.__new__(ModelVecEnv)
    v.E = E
    return v


class _NotAModel:
    E = 20


def test_check_plan():
    from osrl_amd import _lib as L
    from osrl_amd.engine.mpc import check_plan
    assert check_plan(_stub_menv(20), 4, 3) == 5 and check_plan(_stub_menv(1024), 1, 1) == 1024
    assert L.PLAN_MAX_CANDIDATES == 1024
    with pytest.raises(TypeError):
        check_plan(_NotAModel(), 4, 3)
    with pytest.raises(TypeError):
        check_plan(None, 4, 3)
    for E, n, h, kw in ((21, 4, 3, {}),                 # E is not N * K
                        (3, 4, 3, {}),
                        (20, 0, 3, {}),
                        (20, 4, 0, {}),                  # H < 1
                        (20, 4, -2, {}),
                        (1025, 1, 3, {}),                # K > 1024
                        (4100, 4, 3, {}),
                        (20, 4, 3, dict(noise_std=-0.1)),
                        (20, 4, 3, dict(temperature=-1.0)),
                        (20, 4, 3, dict(temperature=NAN))):
        with pytest.raises(ValueError):
            check_plan(_stub_menv(E), n, h, **kw)


def test_the_planner_and_the_trainers_refuse_before_they_build_anything():
    """The constructor and ``Trainer.planner`` judge the shape first: with a stub model (no attributes at all) anything
    past the check would be an AttributeError."""
    from osrl_amd.algorithms import BCTrainer, CDTTrainer
    from osrl_amd.engine.mpc import ModelPlanner
    with pytest.raises(ValueError):
        ModelPlanner(object(), _stub_menv(21), "bc", num_envs=4, horizon=3)
    with pytest.raises(TypeError):
        ModelPlanner(object(), _NotAModel(), "bc", num_envs=4, horizon=3)
    with pytest.raises(ValueError):
        ModelPlanner(object(), _stub_menv(2048), "bc", num_envs=1, horizon=3)
    with pytest.raises(ValueError):
        ModelPlanner(object(), _stub_menv(20), "bc", num_envs=4, horizon=0)
    tr = BCTrainer.__new__(BCTrainer)  # (no model: the refusal comes first)
    with pytest.raises(ValueError):
        tr.planner(_stub_menv(21), 4, 3)
    with pytest.raises(TypeError):
        tr.planner(_NotAModel(), 4, 3)
    cdt = CDTTrainer.__new__(CDTTrainer)
    with pytest.raises(TypeError, match="CDT"):
        cdt.planner(_stub_menv(20), 4, 3)


def test_budget_and_states_are_checked_on_the_host():
    import torch
    from osrl_amd.engine.mpc import check_budget, check_states
    assert check_budget(2.5, 3).tolist() == [2.5] * 3 and check_budget(2.5, 3).dtype == np.float32
    assert check_budget(torch.tensor([1.0, 2.0, 3.0]), 3).tolist() == [1.0, 2.0, 3.0]
    assert check_budget(np.float64(0.0), 1).shape == (1,)
    for bad in ([1.0, 2.0], np.zeros(4), torch.zeros(2)):
        with pytest.raises(ValueError):
            check_budget(bad, 3)
    assert check_states(np.zeros((3, 5)), 3, 5).dtype == np.float32
    for bad in (np.zeros((2, 5)), np.zeros((3, 4)), np.zeros(15)):
        with pytest.raises(ValueError):
            check_states(bad, 3, 5)


class _StubPlanner:
    """``PlanRefillAdapter`` needs ``num_envs``, ``venv.state_dim`` and ``act``: the budgets are host arithmetic."""

    def __init__(self, n, od, ad):
        self.num_envs, self.venv, self.ad, self.seen = n, type("V", (), {"state_dim": od})(), ad, []

    def act(self, states, budget):
        self.seen.append((np.array(states, copy=True), np.array(budget, copy=True)))
        return np.zeros((self.num_envs, self.ad), np.float32)


def test_the_refill_adapter_keeps_each_slots_remaining_budget():
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    from osrl_amd.engine.act import PlanRefillAdapter, evaluate_planned
    ad_ = PlanRefillAdapter(_StubPlanner(2, 3, 1), cost_limit=2.0, cost_scale=1.5)
    assert ad_.limit == 3.0 and ad_.costs({"cost": 1.0}) == (1.5, 1.5)
    obs, z = np.zeros((2, 3), np.float32), np.zeros(2)
    on, off = np.array([True, True]), np.array([False, False])
    ad_.act(obs, z, z, off, on, [0, 1])
    ad_.act(obs, z, np.array([1.5, 0.0]), on, off, [None, None])
    ad_.act(obs, z, np.array([1.5, 1.5]), on, off, [None, None])
    ad_.act(obs, z, np.array([1.5, 9.0]), np.array([True, False]), np.array([False, True]), [None, 2])  # slot 1 restarts
    assert [b.tolist() for b in ad_.budgets] == [[3.0, 3.0], [1.5, 3.0], [0.0, 1.5], [0.0, 3.0]]
    # through the loop, on host environments: shapes and the schedule
    envs = [SyntheticSafeEnv(3, 1, 4, seed=s) for s in (1, 2)]
    pl = _StubPlanner(2, 3, 1)
    (r, c, n), adapter = evaluate_planned(pl, envs, 3, 1.0, episode_len=4)
    assert n == 4.0 and np.isfinite([r, c]).all() and len(pl.seen) == 8 and pl.seen[0][0].shape == (2, 3)
    with pytest.raises(ValueError):
        evaluate_planned(pl, envs[:1], 3, 1.0, episode_len=4)


def test_the_mlp_trainers_have_the_two_methods():
    from osrl_amd.algorithms import BCQLTrainer, BCTrainer, BEARLTrainer, COptiDICETrainer, CPQTrainer
    for t in (BCTrainer, CPQTrainer, BCQLTrainer, BEARLTrainer, COptiDICETrainer):
        assert callable(getattr(t, "planner")) and callable(getattr(t, "evaluate_planned"))


# ---- the C ABI -------------------------------------------------------------------------------------------------------
PROTOS = {"osrl_plan_fanout": 12, "osrl_plan_select": 12}


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_the_header_declares_the_symbol_in_plain_c(name, tmp_path):
    from osrl_amd import _lib as L
    from osrl_amd.build import SOURCES
    assert "plan.hip" in SOURCES
    hdr = open(os.path.join(ROOT, "include", "osrl_amd.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, re.S)
    assert m, name
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    assert len(params) == PROTOS[name] == len(L.PROTOTYPES[name])
    assert hasattr(L.load(), name)
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "a C compiler is required"
    src = str(tmp_path / "use.c")
    with open(src, "w") as f:  # (C99, not C++: the header must do without either language's extras)
        f.write(f'#include "osrl_amd.h"\nint (*p)() = (int (*)()){name};\nint k = OSRL_PLAN_MAX_CANDIDATES;\n')
    subprocess.run([gcc, "-std=c99", "-c", "-I", os.path.join(ROOT, "include"), src, "-o", str(tmp_path / "use.o")],
                   check=True, capture_output=True)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from osrl_amd import _lib as L
    lib = L.load()
    one = 0x1000  # (never dereferenced: every call below fails a check first)
    ok = [one, 3, 5, 4, one, one, 4, one, one, one, None, None]
    for i, bad in ((0, None), (1, 0), (2, 0), (2, 1025), (3, 0), (4, None), (5, None), (6, 3), (7, None), (8, None),
                   (9, None), (1, 1 << 30)):
        args = list(ok)
        args[i] = bad
        assert lib.osrl_plan_fanout(*args) == -1, (i, bad)
    ok = [one, 2, one, one, one, 3, 5, 2, one, one, one, None]
    for i, bad in ((0, None), (1, 0), (2, None), (3, None), (4, None), (5, 0), (6, 0), (6, 1025), (7, 0), (8, None),
                   (9, None), (10, None), (5, 1 << 30)):
        args = list(ok)
        args[i] = bad
        assert lib.osrl_plan_select(*args) == -1, (i, bad)


# ---- compile-time budgets ----------------------------------------------------------------------------------------------
def test_no_scratch_and_the_lds_of_design_md(tmp_path):
    from osrl_amd.build import FILE_FLAGS, FLAGS
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.fail("hipcc is required to cross-compile the gfx950 listing")
    out = str(tmp_path / "plan.s")
    cmd = [hipcc] + FLAGS + FILE_FLAGS.get("plan.hip", []) + ["-S", "--cuda-device-only",
                                                              os.path.join(ROOT, "osrl_amd", "csrc", "plan.hip"), "-o", out]
    assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    res, kern = {}, None
    for ln in open(out):
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', ln)
        if m:
            kern = res.setdefault(m.group(1), {})
            continue
        for key, field in (("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"),
                           ("vgpr", "next_free_vgpr")):
            m = re.search(r'\.amdhsa_' + field + r'\s+(\d+)', ln)
            if m and kern is not None:
                kern[key] = int(m.group(1))
    fan = next(v for k, v in res.items() if "plan_fanout_kernel" in k)
    sel = next(v for k, v in res.items() if "plan_select_kernel" in k)
    assert len(res) == 2, list(res)
    assert fan["scratch"] == 0 and sel["scratch"] == 0
    assert fan["lds"] == 0 and 4096 <= sel["lds"] <= 4096 + 256  # the 1024 weights, and the reduction's few words
    assert fan["vgpr"] <= 32 and sel["vgpr"] <= 32
