#!/usr/bin/env python3
"""Env-steps/s of CDTTrainer.rollout on a host environment (SyntheticSafeEnv): the act latency path
(fast_rollout=True, csrc/cdt_act.hip) against the existing loop (fast_rollout=False), in one process on one device.
Shapes: C5's CDT (od 11, ad 3, seq_len 20, E 256, 3 layers, 8 heads, all tokens, cost_transform, stochastic) with
100-step episodes, and the reference's default model (E 128, seq_len 10) with 300-step episodes.
Writes profiles/cdt_act_bench.json (--out).  --trace: one fast C5 episode only (for rocprofv3 --kernel-trace).

--envs 1,2,4,...: the lockstep form instead (CDTTrainer.rollout_many over N host environments, CDTVecFastPolicy): per
shape and N the aggregate env-steps/s, the time inside ``pol.step`` alone (the C call: launches + the wait for the
published actions) and the time inside the environments' ``step`` (host numpy), each over --repeats runs, written to
profiles/cdt_act_vec_bench.json (--vec-out) together with the one-episode fast rows of the same process.
--trace --envs N: one lockstep C5 wave of N episodes only.

--slots: slots at independent timesteps and the refill schedule, written to profiles/cdt_act_slots_bench.json
(--slots-out), at C5's shape:
  * lockstep: ``pol.step`` us per call at N = 1, 16, 64 with all slots active, one fresh process per repeat; with
    --ab DIR (another checkout of the project with its library built, e.g. the parent commit) the processes alternate
    between DIR and this tree, so that the two columns come from interleaved pairs of one session;
  * refill: a fixed job set on environments of unequal episode length at N = 4 and 16, ``evaluate_targets`` with
    schedule="waves" against schedule="refill": aggregate env-steps/s and policy calls of each;
  * idle: us per call of a 16-slot policy in the sliding phase with all slots active in lockstep, with all slots active
    at staggered timesteps (the per-call table path), and with half the slots frozen.
--tree DIR: import osrl_amd from DIR instead of this checkout (what --ab starts its children with)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[1:-1] else ROOT  # (see --tree)
sys.path.insert(0, TREE)
from osrl_amd.algorithms import CDT, CDTTrainer  # noqa: E402
from osrl_amd.common.logger import DummyLogger  # noqa: E402
from osrl_amd.common.synthetic_env import SyntheticSafeEnv  # noqa: E402

DEV = "cuda:0"
SHAPES = {"c5": dict(seq_len=20, embedding_dim=256, episode_len=100),
          "ref_default": dict(seq_len=10, embedding_dim=128, episode_len=300)}


def make(shape):
    kw = SHAPES[shape]
    torch.manual_seed(0)
    m = CDT(11, 3, 1.0, seq_len=kw["seq_len"], episode_len=kw["episode_len"], embedding_dim=kw["embedding_dim"],
            num_layers=3, num_heads=8, use_rew=True, use_cost=True, cost_transform=True, stochastic=True,
            target_entropy=-3, device=DEV)
    m.eval()
    return m


def rate(m, fast, episodes):
    env = SyntheticSafeEnv(11, 3, m.episode_len, seed=1)
    tr = CDTTrainer(m, env, DummyLogger(), use_graph=False, fast_rollout=fast)
    tr.rollout(m, env, 300.0, 10.0)  # warm-up: handles, engines, code objects
    torch.cuda.synchronize()
    steps = 0
    t0 = time.perf_counter()
    for _ in range(episodes):
        steps += tr.rollout(m, env, 300.0, 10.0)[1]
    dt = time.perf_counter() - t0
    return steps / dt, steps, dt


class TimedEnv:
    """A host environment whose step() time is accumulated in ``clock[0]``."""

    def __init__(self, env, clock):
        self.env, self.clock = env, clock

    def reset(self):
        return self.env.reset()

    def step(self, action):
        t0 = time.perf_counter()
        out = self.env.step(action)
        self.clock[0] += time.perf_counter() - t0
        return out


def vec_rate(m, n_envs, waves):
    """``waves`` lockstep waves of ``n_envs`` full episodes: (aggregate env steps, wall s, s inside pol.step, calls of
    pol.step, s inside env.step)."""
    env_clock, pol_clock = [0.0], [0.0, 0]
    envs = [TimedEnv(SyntheticSafeEnv(11, 3, m.episode_len, seed=1 + e), env_clock) for e in range(n_envs)]
    tr = CDTTrainer(m, None, DummyLogger(), use_graph=False)
    pol = m.fast_policy(num_envs=n_envs)
    inner = type(pol).step

    def timed_step(*a, **k):
        t0 = time.perf_counter()
        out = inner(pol, *a, **k)
        pol_clock[0] += time.perf_counter() - t0
        pol_clock[1] += 1
        return out

    pol.step = timed_step
    try:
        tr.rollout_many(m, envs, 300.0, 10.0)  # warm-up
        torch.cuda.synchronize()
        env_clock[0], pol_clock[0], pol_clock[1] = 0.0, 0.0, 0
        steps = 0
        t0 = time.perf_counter()
        for _ in range(waves):
            steps += int(tr.rollout_many(m, envs, 300.0, 10.0)[1].sum())
        dt = time.perf_counter() - t0
    finally:
        del pol.step
    return steps, dt, pol_clock[0], pol_clock[1], env_clock[0]


def vec_main(a):
    ns = [int(x) for x in a.envs.split(",")]
    if a.trace:
        m = make("c5")
        steps, dt, ps, pc, es = vec_rate(m, ns[0], 1)
        print(f"traced lockstep C5 wave: {ns[0]} episodes, {steps} env steps in {dt * 1e3:.2f} ms = "
              f"{steps / dt:.0f} env-steps/s; pol.step {ps / pc * 1e6:.1f} us per call")
        return
    res = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, one_episode={}, rows={})
    for shape in SHAPES:
        m = make(shape)
        runs = [rate(m, True, a.fast_episodes)[0] for _ in range(a.repeats)]
        res["one_episode"][shape] = dict(fast_env_steps_per_s=[round(r, 1) for r in runs])
        print(shape, "one episode", json.dumps(res["one_episode"][shape]), flush=True)
        res["rows"][shape] = {}
        for n in ns:
            waves = max(1, a.fast_episodes // n)
            agg, step_us, env_us = [], [], []
            for _ in range(a.repeats):
                steps, dt, ps, pc, es = vec_rate(m, n, waves)
                agg.append(round(steps / dt, 1))
                step_us.append(round(ps / pc * 1e6, 2))
                env_us.append(round(es / steps * 1e6, 2))
            row = dict(envs=n, waves=waves, env_steps_per_s=agg, pol_step_us_per_call=step_us,
                       pol_step_us_per_env_step=[round(x / n, 2) for x in step_us], env_step_us_per_env_step=env_us)
            res["rows"][shape][str(n)] = row
            print(shape, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.vec_out), exist_ok=True)
    with open(a.vec_out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def lockstep_row(a):
    """One process's lockstep row: us per ``pol.step`` call at each N (C5's shape, all slots active), as a JSON line."""
    m = make("c5")
    row = {}
    for n in [int(x) for x in a.envs.split(",")]:
        steps, dt, ps, pc, es = vec_rate(m, n, max(2, a.fast_episodes // n))
        row[str(n)] = round(ps / pc * 1e6, 2)
    print("LOCKSTEP_ROW " + json.dumps(row), flush=True)


def lockstep_ab(a):
    """``a.repeats`` processes per tree, alternating (other tree first): {"parent": {N: [us, ..]}, "branch": {..}}."""
    trees = ([("parent", os.path.abspath(a.ab))] if a.ab else []) + [("branch", ROOT)]
    out = {name: {} for name, _ in trees}
    for _ in range(a.repeats):
        for name, tree in trees:
            cmd = [sys.executable, os.path.abspath(__file__), "--lockstep-row", "--envs", a.envs, "--fast-episodes",
                   str(a.fast_episodes), "--repeats", "1", "--tree", tree]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, check=True)
            line = [x for x in r.stdout.splitlines() if x.startswith("LOCKSTEP_ROW ")][-1]
            for n, us in json.loads(line[len("LOCKSTEP_ROW "):]).items():
                out[name].setdefault(n, []).append(us)
            print(name, line, flush=True)
    for name in out:
        out[name] = {n: dict(us_per_call=v, median=float(np.median(v)), spread=round(max(v) - min(v), 2))
                     for n, v in out[name].items()}
    return out


class CountedPolicy:
    """Counts the calls (and the time) of a lockstep policy's ``reset`` and ``step``."""

    def __init__(self, pol):
        self.pol, self.calls, self.secs = pol, 0, 0.0
        for name in ("reset", "step"):
            setattr(pol, name, self._wrap(getattr(type(pol), name)))

    def _wrap(self, inner):
        def f(*a, **k):
            t0 = time.perf_counter()
            out = inner(self.pol, *a, **k)
            self.secs += time.perf_counter() - t0
            self.calls += 1
            return out
        return f

    def release(self):
        del self.pol.reset, self.pol.step


REFILL_LENGTHS = [100, 25, 40, 10]  # environment e ends its episodes after REFILL_LENGTHS[e % 4] steps


def refill_rows(m, n_envs, repeats):
    """4 * n_envs jobs on n_envs environments of unequal length, both schedules on the same jobs."""
    row = dict(envs=n_envs, jobs=4 * n_envs, episode_lengths=[REFILL_LENGTHS[e % 4] for e in range(n_envs)])
    for schedule in ("waves", "refill"):
        rates, calls, steps = [], 0, 0
        for rep_ in range(repeats + 1):  # (the first run warms up)
            envs = [SyntheticSafeEnv(11, 3, REFILL_LENGTHS[e % 4], seed=1 + e) for e in range(n_envs)]
            tr = CDTTrainer(m, envs, DummyLogger(), use_graph=False)
            cp = CountedPolicy(m.fast_policy(num_envs=n_envs))
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                (_, _, mean_len), = tr.evaluate_targets(4 * n_envs, [(300.0, 10.0)], schedule=schedule)
                dt = time.perf_counter() - t0
            finally:
                cp.release()
            m.eval()
            steps, calls = int(round(mean_len * 4 * n_envs)), cp.calls
            if rep_:
                rates.append(round(steps / dt, 1))
        row[schedule] = dict(env_steps=steps, policy_calls=calls, env_steps_per_s=rates)
    row["call_ratio"] = round(row["waves"]["policy_calls"] / row["refill"]["policy_calls"], 3)
    row["rate_ratio"] = round(float(np.median(row["refill"]["env_steps_per_s"]) /
                                    np.median(row["waves"]["env_steps_per_s"])), 3)
    return row


def idle_rows(m, repeats, N=16, calls=30):
    """us per call in the sliding phase: lockstep, all slots at staggered timesteps, half the slots frozen."""
    pol = m.fast_policy(num_envs=N)
    T = m.seq_len
    obs, z = np.zeros((N, m.state_dim), np.float32), np.zeros(N)
    every, none = np.ones(N, bool), np.zeros(N, bool)
    first, half = none.copy(), every.copy()
    first[0], half[1::2] = True, False

    def timed(active):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            pol.step(obs, z, z, active=active)
        return round((time.perf_counter() - t0) / calls * 1e6, 2)

    out = dict(envs=N, lockstep_all_active=[], staggered_all_active=[], half_frozen=[])
    for _ in range(repeats):
        pol.reset(obs, 300.0, 10.0)
        for _ in range(T + 2):
            pol.step(obs, z, z)
        out["lockstep_all_active"].append(timed(None))
        # slot 0 one timestep ahead of the others: every call takes the per-call table
        pol.step(obs, z, z, active=first, restart=first, target_return=300.0, target_cost=10.0)
        pol.step(obs, z, z, active=every, restart=~first, target_return=300.0, target_cost=10.0)
        for _ in range(T + 2):
            pol.step(obs, z, z)
        assert len(set(pol.timesteps)) == 2
        out["staggered_all_active"].append(timed(every))
        out["half_frozen"].append(timed(half))
    return out


def slots_main(a):
    res = dict(device=torch.cuda.get_device_name(0), shape=SHAPES["c5"], repeats=a.repeats)
    res["lockstep_pol_step_us_per_call"] = lockstep_ab(a)
    m = make("c5")
    res["refill"] = {}
    for n in (4, 16):
        res["refill"][str(n)] = refill_rows(m, n, a.repeats)
        print("refill", json.dumps(res["refill"][str(n)]), flush=True)
    res["idle"] = idle_rows(m, a.repeats)
    print("idle", json.dumps(res["idle"]), flush=True)
    os.makedirs(os.path.dirname(a.slots_out), exist_ok=True)
    with open(a.slots_out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdt_act_bench.json"))
    ap.add_argument("--fast-episodes", type=int, default=20)
    ap.add_argument("--loop-episodes", type=int, default=2)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--envs", default=None, help="comma-separated episode counts: the lockstep rows")
    ap.add_argument("--vec-out", default=os.path.join(ROOT, "profiles", "cdt_act_vec_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slots", action="store_true", help="independent slots and the refill schedule")
    ap.add_argument("--slots-out", default=os.path.join(ROOT, "profiles", "cdt_act_slots_bench.json"))
    ap.add_argument("--ab", default=None, help="another checkout (library built) to alternate the lockstep rows with")
    ap.add_argument("--tree", default=None, help="import osrl_amd from this checkout")
    ap.add_argument("--lockstep-row", action="store_true", help="(child of --slots) one lockstep row as a JSON line")
    a = ap.parse_args()
    if a.lockstep_row:
        a.envs = a.envs or "1,16,64"
        return lockstep_row(a)
    if a.slots:
        a.envs = a.envs or "1,16,64"
        return slots_main(a)
    if a.envs:
        return vec_main(a)
    if a.trace:
        m = make("c5")
        r, n, dt = rate(m, True, 1)
        print(f"traced fast C5 episode: {n} env steps in {dt * 1e3:.2f} ms = {r:.0f} env-steps/s")
        return
    res = dict(device=torch.cuda.get_device_name(0), rows={})
    for shape in SHAPES:
        m = make(shape)
        fr, fn, fdt = rate(m, True, a.fast_episodes)
        lr, ln, ldt = rate(m, False, a.loop_episodes)
        res["rows"][shape] = dict(SHAPES[shape], fast_env_steps_per_s=round(fr, 1), loop_env_steps_per_s=round(lr, 1),
                                  speedup=round(fr / lr, 2), fast_steps=fn, loop_steps=ln,
                                  fast_us_per_step=round(fdt / fn * 1e6, 2), loop_us_per_step=round(ldt / ln * 1e6, 2))
        print(shape, json.dumps(res["rows"][shape]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
