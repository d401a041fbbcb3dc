"""CPU-side checks of the recording refill loop (engine/act.py ``collect_refill``) and of what reaches it: a stub adapter
with a fixed action function over ``SyntheticSafeEnv``s of unequal ``episode_len`` -- 4 environments truncating at 5 / 3 /
3 / 3 steps, 8 jobs -- gives the job-major layout, the ``terminals`` / ``timeouts`` placement, the true lengths, the fp64
discounted sums of a direct loop, and one result for 1, 2 and 4 environments; the ``SequenceStore`` refusal comes before
the run; the four new C entry points are in the header (as C99), the prototypes and the library."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OD, AD, EL, J = 5, 2, 4, 8
LENS = (5, 3, 3, 3)  # the environments' own episode_len; model episode_len EL = 4 cuts the first one
GAMMA, CS = 0.9, 2.0
W = np.random.RandomState(0).randn(OD, AD)


def _envs(n):
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    # one dynamics (seed 3) for every environment: a job's trajectory depends on its actions alone, not on its slot
    return [SyntheticSafeEnv(OD, AD, LENS[e], seed=3) for e in range(n)]


def _action(o, q, t):
    return np.tanh(o.astype(np.float64) @ W).astype(np.float32) * np.float32(0.5 + 0.05 * q) + np.float32(0.01 * t)


class StubAdapter:
    """The action of a slot is a fixed function of (its observation, its job, the job's step)."""

    obs_dim = OD + 1

    def __init__(self, N, envs=None, job_lens=None):
        self.N, self.job, self.t, self.calls = N, [None] * N, [0] * N, 0
        self.envs, self.job_lens = envs, job_lens  # (optional: a job's own length, whatever slot it runs in)

    def observe(self, o):
        return np.append(o, 7.0)  # (BC multi-task's appended value: must not reach the dataset)

    def costs(self, info):
        return 0.0, info["cost"] * CS

    def act(self, obs, reward, cost, step, restart, jobs):
        self.calls += 1
        out = np.zeros((self.N, AD), np.float32)
        for e in range(self.N):
            if restart[e]:
                self.job[e], self.t[e] = jobs[e], 0
                if self.envs is not None:
                    self.envs[e].episode_len = self.job_lens[jobs[e]]
            elif step[e]:
                self.t[e] += 1
            if restart[e] or step[e]:
                assert obs[e][OD] == 7.0
                out[e] = _action(obs[e][:OD], self.job[e], self.t[e])
        return out


def _run(n):
    from osrl_amd.engine.act import collect_refill
    ad = StubAdapter(n)
    return collect_refill(ad, _envs(n), list(range(J)), EL, gamma=GAMMA, cost_scale=CS), ad


def _slot_of(n):
    """Job -> slot of the list schedule with these lengths (every environment ends every episode after the same number
    of steps): tests/test_rollout_refill_cpu.py checks the scheduler itself."""
    lens = [min(LENS[e], EL) for e in range(n)]
    free, slot = [0] * n, []
    for q in range(J):
        e = q if q < n else min(range(n), key=lambda i: (free[i], i))
        slot.append(e)
        free[e] += lens[e]
    return slot


def test_job_major_layout_flags_lengths_and_sums():
    got, ad = _run(4)
    slot = _slot_of(4)
    np.testing.assert_array_equal(got.refill.slots, slot)
    lens = np.array([min(LENS[e], EL) for e in slot])
    assert set(lens) == {3, 4}  # unequal lengths, and one environment cut by episode_len
    np.testing.assert_array_equal(got.lengths, lens)
    np.testing.assert_array_equal(got.refill.lengths, lens)
    d = got.dataset
    n = int(lens.sum())
    assert d["observations"].shape == (n, OD) and d["next_observations"].shape == (n, OD)
    assert d["actions"].shape == (n, AD)
    for k in ("rewards", "costs", "terminals", "timeouts"):
        assert d[k].shape == (n,), k
    assert all(v.dtype == np.float32 for v in d.values())
    # a direct loop per job, on a fresh environment of the job's slot
    row = 0
    for q in range(J):
        env = _envs(4)[slot[q]]
        o, _ = env.reset()
        ret = cret = dret = dcret = 0.0
        for t in range(lens[q]):
            a = _action(o, q, t)
            np.testing.assert_array_equal(d["observations"][row], o)
            np.testing.assert_array_equal(d["actions"][row], a)
            o, r, term, trunc, info = env.step(a)
            np.testing.assert_array_equal(d["next_observations"][row], o)
            assert d["rewards"][row] == np.float32(r) and d["costs"][row] == np.float32(info["cost"])
            assert d["terminals"][row] == 0.0
            assert d["timeouts"][row] == float(t == lens[q] - 1) == float(trunc or t + 1 == EL)
            ret, cret = ret + r, cret + info["cost"] * CS
            dret, dcret = dret + GAMMA ** t * r, dcret + GAMMA ** t * info["cost"] * CS
            row += 1
        assert got.returns[q] == ret and got.cost_returns[q] == cret
        assert abs(got.disc_returns[q] - dret) <= 1e-12 * max(1.0, abs(dret))
        assert abs(got.disc_cost_returns[q] - dcret) <= 1e-12 * max(1.0, abs(dcret))
    assert row == n
    assert got.returns.dtype == got.disc_returns.dtype == got.lengths.dtype == np.float64
    # the sums are the schedule's own (rollout_refill's accumulation)
    np.testing.assert_array_equal(got.returns, got.refill.returns)
    np.testing.assert_array_equal(got.cost_returns, got.refill.costs)


def test_terminated_episodes_set_terminals():
    from osrl_amd.engine.act import collect_refill
    from test_rollout_refill_cpu import ScriptedEnv  # episodes end terminated / truncated alternately

    class One:
        obs_dim = 2
        observe = staticmethod(lambda o: o)
        costs = staticmethod(lambda info: (0.0, info["cost"]))

        def act(self, obs, reward, cost, step, restart, jobs):
            return np.ones(len(obs))

    got = collect_refill(One(), [ScriptedEnv([2, 3, 9])], [0, 1, 2], episode_len=4)
    np.testing.assert_array_equal(got.lengths, [2, 3, 4])
    np.testing.assert_array_equal(got.dataset["terminals"], [0, 1, 0, 0, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(got.dataset["timeouts"], [0, 0, 0, 0, 1, 0, 0, 0, 1])
    assert got.dataset["actions"].shape == (9,)


def test_result_does_not_depend_on_the_number_of_environments():
    """Jobs of unequal length (5 / 3 / 3 / 3 / 4 / ..., a property of the job here: the adapter sets its slot's
    environment to truncate there; episode_len 4 cuts the longest) on environments that share their dynamics: the dataset
    and the sums are the same arrays for 1, 2 and 4 environments, although the jobs run in other slots at other calls."""
    from osrl_amd.engine.act import collect_refill
    job_lens = [5, 3, 3, 3, 4, 3, 5, 3]
    outs = []
    for n in (1, 2, 4):
        envs = _envs(n)
        ad = StubAdapter(n, envs, job_lens)
        outs.append(collect_refill(ad, envs, list(range(J)), EL, gamma=GAMMA, cost_scale=CS))
    np.testing.assert_array_equal(outs[0].lengths, [min(x, EL) for x in job_lens])
    assert len({tuple(o.refill.slots) for o in outs}) == 3  # the jobs did run in other slots
    assert len({o.refill.calls for o in outs}) == 3
    for o in outs[1:]:
        for k in outs[0].dataset:
            np.testing.assert_array_equal(o.dataset[k], outs[0].dataset[k], err_msg=k)
        for name in ("returns", "cost_returns", "lengths", "disc_returns", "disc_cost_returns"):
            np.testing.assert_array_equal(getattr(o, name), getattr(outs[0], name), err_msg=name)


def test_rollout_refill_is_unchanged_by_the_recorder():
    from osrl_amd.engine.act import collect_refill, rollout_refill
    plain = rollout_refill(StubAdapter(4), _envs(4), list(range(J)), EL)
    got = collect_refill(StubAdapter(4), _envs(4), list(range(J)), EL, cost_scale=CS)
    for a, b in zip(plain, got.refill):
        np.testing.assert_array_equal(a, b)


def test_sequence_store_is_refused_before_the_run():
    from osrl_amd.common.replay import SequenceStore
    from osrl_amd.engine.act import check_jobs_store

    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"{name}: the run started before the store was checked")

    st = object.__new__(SequenceStore)
    st._live, st._dist, st.od, st.ad = object(), None, OD, AD
    st.n_traj, st.n_rows, st.capacity_traj, st.capacity_rows = 2, 10, 10, 10 + J * EL - 1
    with pytest.raises(ValueError, match="does not fit"):  # one row short of J jobs of episode_len rows
        check_jobs_store(st, J, EL, OD, AD)
    st.capacity_rows += 1
    check_jobs_store(st, J, EL, OD, AD)
    st.capacity_traj = J + 1
    with pytest.raises(ValueError, match="does not fit"):
        check_jobs_store(st, J, EL, OD, AD)
    with pytest.raises(ValueError, match="columns"):
        check_jobs_store(st, 1, EL, OD + 1, AD)
    # through the trainer's method: nothing of the model's device side or of the environments is touched first
    from osrl_amd.algorithms.cdt import CDTTrainer
    from types import SimpleNamespace
    t = object.__new__(CDTTrainer)
    t.cost_scale = 1.0
    model = SimpleNamespace(stochastic=False, episode_len=EL, action_dim=AD, state_dim=OD)
    with pytest.raises(ValueError, match="does not fit"):
        t.collect_jobs(model, [Boom()], [1.0] * J, [1.0] * J, into=st)


def test_argument_checks_come_before_any_device_call():
    from osrl_amd.engine.act import check_job_noise
    sg, noise, ids = check_job_noise(3, EL, AD, 0.25, None, None)
    assert sg.dtype == np.float32 and list(sg) == [0.25] * 3 and noise is None and list(ids) == [0, 1, 2]
    sg, noise, ids = check_job_noise(3, EL, AD, [0.0, 0.1, 0.2], np.zeros((3, EL, AD)), [5, 6, 7])
    assert noise.dtype == np.float32 and list(ids) == [5, 6, 7]
    with pytest.raises(ValueError, match="noise_std"):
        check_job_noise(3, EL, AD, [0.1, 0.2], None, None)
    with pytest.raises(ValueError, match="noise must be"):
        check_job_noise(3, EL, AD, 0.1, np.zeros((EL, 3, AD)), None)
    with pytest.raises(ValueError, match="episode_ids"):
        check_job_noise(3, EL, AD, 0.1, None, [1, 2])
    with pytest.raises(ValueError, match="episode_ids"):
        check_job_noise(3, EL, AD, 0.1, None, [1, 2, -3])
    # the policies' own checks
    from test_mlp_act_vec_cpu import _stub_policy
    p = _stub_policy()
    obs = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError, match="explore_std"):
        p.step(obs, explore_std=[0.1, 0.2])
    with pytest.raises(ValueError, match="explore_noise of shape"):
        p.step(obs, explore_std=0.1, explore_noise=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="pass explore_std"):
        p.step(obs, explore_noise=np.zeros((3, 2)))
    # collect / collect_targets still refuse host environments (tests/test_collect_cpu.py, tests/test_cdt_collect_cpu.py)
    from osrl_amd.algorithms._base import RolloutMixin
    from osrl_amd.algorithms.cdt import CDTTrainer
    assert callable(RolloutMixin.collect_jobs) and callable(CDTTrainer.collect_jobs)


def test_finish_jobs_uploads_once_and_hands_views_or_appends():
    """``finish_jobs`` with the host as the "device": the seven tables come back as views of ONE buffer with the host
    rows' bits, an empty run keeps its widths, and ``into=`` gets the tables while the result's dataset is None."""
    from osrl_amd.engine.act import collect_refill, finish_jobs
    from osrl_amd.engine.collect import KEYS, Collected
    got, _ = _run(4)
    res = finish_jobs(got, "cpu", None)
    assert isinstance(res, Collected) and set(res.dataset) == set(KEYS)
    base = {v.untyped_storage().data_ptr() for v in res.dataset.values()}
    assert len(base) == 1
    for k in KEYS:
        np.testing.assert_array_equal(res.dataset[k].numpy(), got.dataset[k], err_msg=k)
        assert res.dataset[k].is_contiguous()
    np.testing.assert_array_equal(res.lengths, got.lengths)

    class Store:
        def append(self, data):
            self.data = data

    st = Store()
    into = finish_jobs(got, "cpu", st)
    assert into.dataset is None and set(st.data) == set(KEYS)
    np.testing.assert_array_equal(into.disc_returns, got.disc_returns)
    empty = collect_refill(None, _envs(2), [], EL)
    assert empty.returns.shape == (0,) and empty.dataset["rewards"].shape == (0,)
    out = finish_jobs(empty, "cpu", None)
    assert all(v.shape[0] == 0 for v in out.dataset.values())


NEW = {"osrl_policy_explore_io_n": 3, "osrl_policy_act_explore_n": 7, "osrl_cdt_policy_explore_io": 5,
       "osrl_cdt_policy_step_slots_explore": 7}


def test_new_entry_points_in_header_prototypes_and_library(tmp_path):
    import ctypes as C
    from osrl_amd import _lib as L
    from osrl_amd import build as b
    hdr = open(os.path.join(ROOT, "include", "osrl_amd.h")).read()
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/osrl_amd.h"
        assert len(m.group(1).split(",")) == nargs == len(L.PROTOTYPES[name]), name
    lib = C.CDLL(b.build())
    for name in NEW:
        assert hasattr(lib, name), f"libosrl_amd.so does not export {name}"
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is required to compile the header as C")
    src = str(tmp_path / "h.c")
    with open(src, "w") as f:
        f.write('#include "osrl_amd.h"\n'
                "int (*a)(void*, float**, float**) = osrl_policy_explore_io_n;\n"
                "int (*b)(void*, int32_t, int32_t, uint64_t, uint64_t, int32_t, void*) = osrl_policy_act_explore_n;\n"
                "int (*c)(void*, float**, float**, int32_t**, float**) = osrl_cdt_policy_explore_io;\n"
                "int (*d)(void*, const int32_t*, int32_t, int32_t, uint64_t, int32_t, void*) = "
                "osrl_cdt_policy_step_slots_explore;\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                    str(tmp_path / "h.o")], check=True, capture_output=True)
