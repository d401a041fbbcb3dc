"""CPU-side checks of the refill schedule (engine/act.py ``rollout_refill``) and of the arguments that reach it: the
scheduler on a stub policy and stub environments of scripted lengths (job-to-slot assignment with the ascending-slot
tie-break, the call count = the list schedule's makespan, every job exactly once, no call after the last job ends), the
``ValueError`` on an unknown ``schedule``, the two new C entry points in the header / prototypes / library, and the
argument checks on ``restart``, ``target_*`` and ``episode_ids``, which raise before any device call."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ScriptedEnv:
    """Episode ``k`` of this environment lasts ``lengths[k]`` steps (terminated or truncated, alternately); the reward
    of a step is the action it was given, the cost 1."""

    def __init__(self, lengths):
        self.lengths, self.episode, self.t = list(lengths), -1, 0

    def reset(self):
        self.episode += 1
        self.t = 0
        return np.array([float(self.episode), 0.0]), {}

    def step(self, action):
        self.t += 1
        end = self.t == self.lengths[self.episode]
        return (np.array([float(self.episode), float(self.t)]), float(action), end and self.episode % 2 == 0,
                end and self.episode % 2 == 1, {"cost": 1.0})


class StubAdapter:
    """Records every policy call; the action of a slot is 1000 * its job + the job's step."""

    obs_dim = 2

    def __init__(self, N):
        self.N, self.calls, self.job, self.k = N, [], [None] * N, [0] * N

    def observe(self, o):
        return o

    def costs(self, info):
        return 0.5 * info["cost"], info["cost"]

    def act(self, obs, reward, cost, step, restart, jobs):
        assert step.dtype == restart.dtype == np.bool_ and not (step & restart).any()
        self.calls.append((step.copy(), restart.copy(), list(jobs), obs.copy(), cost.copy()))
        out = np.zeros(self.N)
        for e in range(self.N):
            assert (jobs[e] is not None) == bool(restart[e])
            if restart[e]:
                self.job[e], self.k[e] = jobs[e], 0
                assert obs[e][1] == 0.0  # a restarting slot shows its environment's reset observation
            elif step[e]:
                self.k[e] += 1
                assert obs[e][1] == self.k[e] and cost[e] == 0.5
            if restart[e] or step[e]:
                out[e] = 1000 * self.job[e] + self.k[e]
        return out


def _list_schedule(lengths_by_slot, J):
    """Job -> (slot, start call) and the makespan of the schedule the issue defines, from the per-slot episode lengths."""
    N = len(lengths_by_slot)
    slot, start, free, taken = {}, {}, [0] * N, [0] * N
    for q in range(J):
        e = q if q < N else min(range(N), key=lambda i: (free[i], i))
        slot[q], start[q] = e, free[e]
        free[e] += lengths_by_slot[e][taken[e]]
        taken[e] += 1
    return slot, start, max(free[e] for e in set(slot.values()))


def test_worked_example_40_calls_against_80_in_waves():
    from osrl_amd.engine.act import rollout_refill
    lengths = [[40] * 8, [10] * 8, [10] * 8, [10] * 8]
    envs, ad = [ScriptedEnv(x) for x in lengths], StubAdapter(4)
    res = rollout_refill(ad, envs, list(range(8)), episode_len=1000)
    assert res.calls == len(ad.calls) == 40
    assert sum(max(lengths[e][w] for e in range(4)) for w in range(2)) == 80  # the same jobs in waves
    np.testing.assert_array_equal(res.slots, [0, 1, 2, 3, 1, 2, 3, 1])
    np.testing.assert_array_equal(res.lengths, [40, 10, 10, 10, 10, 10, 10, 10])
    np.testing.assert_array_equal(res.costs, res.lengths.astype(float))
    for q in range(8):  # the job's own actions came back to its own environment: sum of 1000 q + k over its steps
        L = res.lengths[q]
        assert res.returns[q] == 1000 * q * L + L * (L - 1) // 2
    # the last policy call is the one whose actions end the last job: slots 1 .. 3 idle by then
    step, restart, jobs, _, _ = ad.calls[-1]
    assert list(step) == [True, False, False, False] and not restart.any()
    assert [e.episode for e in envs] == [0, 2, 1, 1]  # every job was started exactly once


def test_assignment_tie_break_and_exactly_once():
    from osrl_amd.engine.act import rollout_refill
    lengths = [[3, 2, 4, 1], [3, 5, 1, 1], [6, 1, 1, 1]]  # slots 0 and 1 finish together: slot 0 takes the earlier job
    J = 9
    envs, ad = [ScriptedEnv(x) for x in lengths], StubAdapter(3)
    res = rollout_refill(ad, envs, list(range(J)), episode_len=1000)
    slot, start, makespan = _list_schedule(lengths, J)
    assert res.calls == makespan == len(ad.calls)
    np.testing.assert_array_equal(res.slots, [slot[q] for q in range(J)])
    assert res.slots[3] == 0 and res.slots[4] == 1  # the tie at call 3
    started = {}
    for c, (step, restart, jobs, _, _) in enumerate(ad.calls):
        assert (step | restart).any()  # no empty call
        for e in np.flatnonzero(restart):
            assert jobs[e] not in started
            started[jobs[e]] = (e, c)
    assert started == {q: (slot[q], start[q]) for q in range(J)}
    assert res.lengths.sum() == sum(step.sum() + restart.sum() for step, restart, _, _, _ in ad.calls)


def test_episode_len_ends_a_job_and_fewer_jobs_than_slots_idle():
    from osrl_amd.engine.act import rollout_refill
    envs, ad = [ScriptedEnv([50, 50]), ScriptedEnv([4, 50]), ScriptedEnv([50])], StubAdapter(3)
    res = rollout_refill(ad, envs, [7, 8], episode_len=6)  # two jobs, three slots: slot 2 never runs
    np.testing.assert_array_equal(res.lengths, [6, 4])
    np.testing.assert_array_equal(res.slots, [0, 1])
    assert res.calls == 6 and envs[2].episode == -1
    assert all(not step[2] and not restart[2] for step, restart, _, _, _ in ad.calls)
    empty = rollout_refill(ad, envs, [], episode_len=6)
    assert empty.calls == 0 and empty.returns.shape == (0,) and res.calls == len(ad.calls)
    with pytest.raises(ValueError, match="empty list of environments"):
        rollout_refill(ad, [], [1], episode_len=6)


def test_unknown_schedule_names_both():
    from osrl_amd.algorithms._base import RolloutMixin
    from osrl_amd.algorithms.cdt import CDTTrainer
    from osrl_amd.engine.act import check_schedule
    assert check_schedule("waves") == "waves" and check_schedule("refill") == "refill"

    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"{name} touched before the schedule was checked")

    t = object.__new__(CDTTrainer)
    t.model, t.env = Boom(), [Boom()]
    for call in (lambda: t.evaluate(2, 1.0, 1.0, schedule="wave"), lambda: t.evaluate_targets(2, [(1.0, 1.0)], "x")):
        with pytest.raises(ValueError, match=r'"waves" or "refill"'):
            call()

    class T(RolloutMixin):
        model, env = Boom(), [Boom()]
    with pytest.raises(ValueError, match=r'"waves" or "refill"'):
        T().evaluate(3, schedule="lockstep")


def test_new_entry_points_in_header_prototypes_and_library(tmp_path):
    from osrl_amd import _lib as L
    from osrl_amd import build as b
    hdr = open(os.path.join(ROOT, "include", "osrl_amd.h")).read()
    for name, nargs in (("osrl_cdt_policy_step_slots", 4), ("osrl_cdt_policy_timesteps", 2)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/osrl_amd.h"
        assert len(m.group(1).split(",")) == nargs == len(L.PROTOTYPES[name]), name
    lib = C.CDLL(b.build())
    assert hasattr(lib, "osrl_cdt_policy_step_slots") and hasattr(lib, "osrl_cdt_policy_timesteps")
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is required to compile the header as C")
    src = str(tmp_path / "h.c")
    with open(src, "w") as f:
        f.write('#include "osrl_amd.h"\n'
                "int (*p)(void*, const int32_t*, int32_t, void*) = osrl_cdt_policy_step_slots;\n"
                "int (*q)(void*, int32_t*) = osrl_cdt_policy_timesteps;\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                    str(tmp_path / "h.o")], check=True, capture_output=True)


class Boom:
    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the argument checks")


def _stub_cdt(N=3, od=4, ad=2):
    """A CDTVecFastPolicy without a device, as tests/test_cdt_act_vec_cpu.py builds it: scalar ``_t`` / ``_episode_len``."""
    from osrl_amd.engine.cdt_act import CDTVecFastPolicy
    p = object.__new__(CDTVecFastPolicy)
    p.num_envs, p.od, p.ad, p.T = N, od, ad, 5
    p._h, p._lib, p.model = object(), Boom(), Boom()
    p._t, p._episode_len = 0, 10
    p._raw_stream, p._dev_index = None, 0
    return p


def test_cdt_restart_and_target_checks_come_before_any_device_call():
    p = _stub_cdt()
    N, od = 3, 4
    obs, rew, cost = np.zeros((N, od), np.float32), np.zeros(N), np.zeros(N)
    one = np.array([False, True, False])
    for bad in (True, np.ones(N + 1, bool), np.ones((N, 1), bool)):
        with pytest.raises(ValueError, match="restart of shape"):
            p.step(obs, rew, cost, restart=bad)
    with pytest.raises(ValueError, match="restart as booleans"):
        p.step(obs, rew, cost, restart=np.ones(N))
    with pytest.raises(ValueError, match="required when a slot restarts"):
        p.step(obs, rew, cost, restart=one)
    with pytest.raises(ValueError, match="required when a slot restarts"):
        p.step(obs, rew, cost, restart=one, target_return=1.0)
    for bad in (np.zeros(N + 1), np.zeros((N, 1)), [1.0, 2.0]):
        with pytest.raises(ValueError, match="target_return"):
            p.step(obs, rew, cost, restart=one, target_return=bad, target_cost=1.0)
        with pytest.raises(ValueError, match="target_cost"):
            p.step(obs, rew, cost, restart=one, target_return=1.0, target_cost=bad)
    with pytest.raises(ValueError, match="obs of shape"):
        p.step(obs[:2], rew, cost, restart=one, target_return=1.0, target_cost=1.0)
    # the scalars stay meaningful: in lockstep they are every slot's timestep and episode length
    np.testing.assert_array_equal(p.timesteps, [0, 0, 0])
    p._t = 9  # a stepping slot past the episode's end is named; an all-False restart mask is the plain step
    with pytest.raises(RuntimeError, match="slot 0: the episode is over: 10 steps"):
        p.step(obs, rew, cost, restart=one, target_return=1.0, target_cost=1.0)
    with pytest.raises(RuntimeError, match="episode is over"):
        p.step(obs, rew, cost, restart=np.zeros(N, bool))
    p._t = -1  # never started: restarting a slot is fine, stepping the others is not, and they are named
    with pytest.raises(RuntimeError, match="slot 0: no episode was started"):
        p.step(obs, rew, cost, restart=one, target_return=1.0, target_cost=1.0)
    with pytest.raises(RuntimeError, match="reset"):
        p.step(obs, rew, cost)
    np.testing.assert_array_equal(p.timesteps, [-1, -1, -1])


def _stub_mlp(N=3, od=4):
    from osrl_amd.engine.act import VecFastPolicy
    p = object.__new__(VecFastPolicy)
    p.num_envs, p.obs_dim, p.act_dim, p.noise_dim, p.kind = N, od, 2, 0, "mlp"
    p._h, p._lib, p._started = object(), Boom(), True
    p._meta = np.zeros((N, 2), np.int32)
    return p


def test_mlp_restart_and_episode_id_checks_come_before_any_device_call():
    p = _stub_mlp()
    N, od = 3, 4
    obs, one = np.zeros((N, od), np.float32), np.array([True, False, False])
    for bad in (True, np.ones(N + 1, bool), np.ones((N, 1), bool)):
        with pytest.raises(ValueError, match="restart of shape"):
            p.step(obs, restart=bad)
    with pytest.raises(ValueError, match="restart as booleans"):
        p.step(obs, restart=np.ones(N, np.int64))
    for bad in (np.arange(N + 1), np.arange(N).reshape(N, 1), 3):
        with pytest.raises(ValueError, match="episode_ids of shape"):
            p.step(obs, restart=one, episode_ids=bad)
    for bad in (np.array([0.0, 1.0, 2.0]), np.array([0, -1, 2]), np.array([0, 1, 2 ** 31])):
        with pytest.raises(ValueError, match="integers in 0"):
            p.step(obs, restart=one, episode_ids=bad)
    with pytest.raises(ValueError, match="pass restart"):
        p.step(obs, episode_ids=np.arange(N))
    with pytest.raises(ValueError, match="obs of shape"):
        p.step(obs[:2], restart=one, episode_ids=np.arange(N))
    assert not p._meta.any()  # nothing was recorded by a refused call
    p._started = False
    with pytest.raises(RuntimeError, match="reset"):
        p.step(obs)
    # rollout_jobs checks its episode ids before it asks the model for a policy
    from osrl_amd.engine.act import rollout_jobs_mlp
    for bad, msg in ((np.arange(4), "episode_ids of shape"), (np.array([0.5, 1, 2]), "integers in 0")):
        with pytest.raises(ValueError, match=msg):
            rollout_jobs_mlp(Boom(), [ScriptedEnv([1])], 3, episode_ids=bad)
