"""Planning at act time (``Trainer.planner`` / engine/mpc.py ``ModelPlanner``) measured: what one ``act`` costs, and what
the feature cost the paths it did not touch.  The shape is C2's: a CPQ policy at (obs, act) = (76, 2), hidden [256, 256],
on a ``ModelVecEnv`` of 5 members with hidden [200, 200, 200].

(a) reported, not gated: microseconds per ``planner.act`` (upload, fan-out, H recorded model steps on N * K episodes,
    select, one host sync) at N in {1, 16} slots, K in {64, 256} candidates, H in {3, 5} steps, beside the microseconds
    per policy call of ``rollout_many`` of the bare policy (``VecFastPolicy``, one launch per call) on the same N host
    ``SyntheticSafeEnv``s.  Both sides run in child processes alternating A B B A (planner, policy, policy, planner);
    medians over every repeat of a side.  The ``rollout_many`` figure includes the host environments' own steps
    (``env_step_us`` is measured beside it and reported).
(b) with ``--parent DIR`` (a built checkout of the parent commit): the untouched ``collect_model(horizon=5)`` (ms per
    call at 1024 episodes) and ``bench.py --gpus 1 --steps 20 --warmup 5`` (its timed region) of this tree against the
    parent's, child processes A B B A.  ``ratio`` = parent median / this tree's median (bench.py: this tree's / the
    parent's, so that above 1 is faster in both); ``parent_spread`` = the parent's own max / min over its repeats;
    ``ok``: the ratio lies inside [1 / parent_spread, parent_spread].

Every repeat is kept.  Writes profiles/plan_bench.json (``--out``).  Needs an MI355X: there is no CPU path."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(od=76, ad=2, hidden=[256, 256], members=5, model_hidden=[200, 200, 200], slots=[1, 16], candidates=[64, 256],
             horizons=[3, 5], episode_len=50, collect_episodes=1024, collect_horizon=5)
BENCH_CMD = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-roofline", "--no-extras"]


def summary(v):
    s = sorted(v)
    return dict(min=round(s[0], 3), median=round(s[len(s) // 2], 3), max=round(s[-1], 3), n=len(s), all=[round(x, 3) for x in v])


def make(episodes, episode_len):
    """(trainer, model environment): only what the parent commit has as well."""
    import numpy as np
    import torch
    from osrl_amd.algorithms import CPQ, CPQTrainer, Dynamics
    from osrl_amd.common.logger import DummyLogger
    from osrl_amd.common.model_env import ModelVecEnv
    from osrl_amd.common.replay import synthetic_transitions
    s = SHAPE
    d = synthetic_transitions(4096, s["od"], s["ad"], seed=1)
    d["next_observations"] = (d["observations"] + 0.1 * d["next_observations"]).astype(np.float32)
    torch.manual_seed(0)
    dyn = Dynamics(s["od"], s["ad"], s["model_hidden"], num_models=s["members"], device="cuda:0")
    dyn.fit_normalizer(d)
    cpq = CPQ(s["od"], s["ad"], 1.0, s["hidden"], s["hidden"], 400, 10, episode_len=s["episode_len"], device="cuda:0")
    menv = ModelVecEnv(dyn, d["observations"][:episodes], episodes, episode_len, reward_penalty=0.5)
    tr = CPQTrainer(cpq, menv, DummyLogger(), 1e-4, 1e-3, 1e-4, 1e-3, device="cuda:0", stats_mode="none")
    return tr, menv


def host_envs(n):
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    s = SHAPE
    return [SyntheticSafeEnv(s["od"], s["ad"], s["episode_len"], seed=3 + e, init_noise=0.5) for e in range(n)]


def worker(tree, what, reps):
    """Runs in a child process with ``tree`` first on the path."""
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    s, out = SHAPE, {}
    if what == "untouched":
        tr, menv = make(s["collect_episodes"], s["collect_horizon"])
        kw = dict(horizon=s["collect_horizon"], noise_std=0.3)
        tr.collect_model(menv, seed=0, **kw)
        ms = []
        for i in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.collect_model(menv, seed=1 + i, **kw)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        out["collect_model_ms"] = ms
    elif what == "plan":
        for n in s["slots"]:
            states = np.stack([e.reset(seed=i)[0] for i, e in enumerate(host_envs(n))]).astype(np.float32)
            for k in s["candidates"]:
                for h in s["horizons"]:
                    tr, menv = make(n * k, h)
                    p = tr.planner(menv, n, h, noise_std=0.3)
                    for _ in range(3):
                        p.act(states, 5.0)
                    us = []
                    for _ in range(reps * 10):
                        t0 = time.perf_counter()
                        p.act(states, 5.0)
                        us.append((time.perf_counter() - t0) * 1e6)
                    out[f"N{n}_K{k}_H{h}"] = us
                    del p, tr, menv
    else:  # "policy": rollout_many of the bare policy on the same N host environments
        tr, _ = make(16, 5)
        for n in s["slots"]:
            envs = host_envs(n)
            tr.rollout_many(envs)
            us = []
            for _ in range(reps):
                t0 = time.perf_counter()
                tr.rollout_many(envs)
                us.append((time.perf_counter() - t0) * 1e6 / s["episode_len"])
            a = np.zeros(s["ad"], np.float32)
            for e in envs:
                e.reset()
            t0 = time.perf_counter()
            for _ in range(s["episode_len"]):
                for e in envs:
                    e.step(a)
            out[f"N{n}"] = dict(per_call_us=us, env_step_us=(time.perf_counter() - t0) * 1e6 / s["episode_len"])
    print("RESULT " + json.dumps(out))


def child(tree, what, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--tree", tree, "--reps", str(reps)]
    env = dict(os.environ)
    lib = os.path.join(tree, "osrl_amd", "lib", "libosrl_amd.so")
    if os.path.exists(lib):  # each tree measures the library it was built with, whatever the files' times say
        env["OSRL_LIB"] = lib
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tree, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"worker {what} failed in {tree}: {r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def bench_child(tree):
    """'value' of one ``bench.py`` process of ``tree`` (its own library, its own bench.py)."""
    env = dict(os.environ)
    lib = os.path.join(tree, "osrl_amd", "lib", "libosrl_amd.so")
    if os.path.exists(lib):
        env["OSRL_LIB"] = lib
    r = subprocess.run([sys.executable] + BENCH_CMD, capture_output=True, text=True, timeout=900, cwd=tree, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py failed in {tree}: {r.stderr[-2000:]}")
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{") and '"value"' in ln]
    return float(rows[-1]["value"])


def gate(here, there, higher_is_better=False):
    h, t = summary(here), summary(there)
    ratio = h["median"] / t["median"] if higher_is_better else t["median"] / h["median"]
    spread = t["max"] / t["min"]
    return dict(this_tree=h, parent=t, ratio=round(ratio, 4), parent_spread=round(spread, 4),
                ok=bool(1.0 / spread <= ratio <= spread))


def against_parent(parent, reps, rounds):
    ch, ct, bh, bt = [], [], [], []
    for _ in range(rounds):  # A B B A
        for tree, c, b in ((ROOT, ch, bh), (parent, ct, bt), (parent, ct, bt), (ROOT, ch, bh)):
            c += child(tree, "untouched", reps)["collect_model_ms"]
            b.append(bench_child(tree))
            print(f"{'this tree' if tree == ROOT else 'parent'}: bench {b[-1]}", file=sys.stderr, flush=True)
    return dict(collect_model_horizon5_ms=gate(ch, ct),
                bench=dict(command="python " + " ".join(BENCH_CMD), unit="grad-steps/s", **gate(bh, bt, higher_is_better=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_bench.json"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part b)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1, help="A B B A rounds")
    ap.add_argument("--worker", default=None, choices=["untouched", "plan", "policy"])
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.tree), args.worker, args.reps)
    plan, pol, env_us = {}, {}, {}
    for _ in range(args.rounds):  # A B B A: planner, policy, policy, planner
        for what in ("plan", "policy", "policy", "plan"):
            got = child(ROOT, what, args.reps)
            for k, v in got.items():
                if what == "plan":
                    plan.setdefault(k, []).extend(v)
                else:
                    pol.setdefault(k, []).extend(v["per_call_us"])
                    env_us.setdefault(k, []).append(v["env_step_us"])
    rows = {}
    for k, v in plan.items():
        n = k.split("_")[0]
        a, b = summary(v), summary(pol[n])
        rows[k] = dict(act_us=a, rollout_many_per_call_us=b, env_step_us=round(sorted(env_us[n])[len(env_us[n]) // 2], 3),
                       ratio=round(a["median"] / b["median"], 3))
    out = dict(shape=SHAPE, act_vs_rollout_many=rows, vs_parent=None)
    if args.parent:
        out["vs_parent"] = against_parent(os.path.abspath(args.parent), args.reps, args.rounds)
    import torch  # (after the children: this process never opens the device before them)
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
