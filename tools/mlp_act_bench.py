#!/usr/bin/env python3
"""Env-steps/s of the MLP trainers' rollouts on N host environments (SyntheticSafeEnv), two ways in one process on one
device: in lockstep through ``rollout_many`` (VecFastPolicy, csrc/act_vec.hip: one C call per environment step for all
N) and the way available without it, N sequential ``rollout()`` calls (FastPolicy, csrc/act.hip: one C call per
environment step of one environment).  N = 1, 2, 4, 16, 64 for three shapes: CPQ at C2's shape (od 76, ad 2, actor
256-256), BCQ-Lag at C3's shape (od 33, ad 8, decoder 400-400, perturbation net 256-256) and a CPQ actor 1024-1024.

Per shape, N and way: one warm-up, then --repeats repetitions of the same number of environment steps; min / median /
max env-steps/s go to profiles/mlp_act_vec_bench.json (--out), with ``lockstep_ahead`` = the lockstep median exceeds
the sequential median by more than the larger of the two min-max spreads.

Each shape is measured in a child process of its own under a time limit (--limit seconds); the first child that fails
or runs out of time ends the run with its exit status, and nothing further is started."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
EPISODE_LEN = 100
SHAPES = {
    "cpq_c2": dict(algo="cpq", od=76, ad=2, hidden=[256, 256], vae_hidden=400),
    "bcql_c3": dict(algo="bcql", od=33, ad=8, hidden=[256, 256], vae_hidden=400),
    "cpq_1024": dict(algo="cpq", od=76, ad=2, hidden=[1024, 1024], vae_hidden=64),
}
ENVS = [1, 2, 4, 16, 64]


def make(shape):
    import torch
    from osrl_amd.algorithms import BCQL, CPQ, BCQLTrainer, CPQTrainer
    from osrl_amd.common.logger import DummyLogger
    kw = SHAPES[shape]
    torch.manual_seed(0)
    if kw["algo"] == "cpq":
        m = CPQ(kw["od"], kw["ad"], 1.0, kw["hidden"], kw["hidden"], kw["vae_hidden"], episode_len=EPISODE_LEN,
                device=DEV)
        return m, CPQTrainer(m, None, DummyLogger(), use_graph=False)
    m = BCQL(kw["od"], kw["ad"], 1.0, kw["hidden"], kw["hidden"], kw["vae_hidden"], episode_len=EPISODE_LEN, device=DEV)
    return m, BCQLTrainer(m, None, DummyLogger(), use_graph=False)


def lockstep(tr, envs, waves):
    steps = 0
    t0 = time.perf_counter()
    for _ in range(waves):
        steps += int(tr.rollout_many(envs)[1].sum())
    return steps / (time.perf_counter() - t0)


def sequential(tr, envs, waves):
    steps = 0
    t0 = time.perf_counter()
    for _ in range(waves):
        for env in envs:
            tr.env = env
            steps += tr.rollout()[1]
    dt = time.perf_counter() - t0
    tr.env = None
    return steps / dt


def stats(runs):
    runs = sorted(runs)
    return dict(min=round(runs[0], 1), median=round(runs[len(runs) // 2], 1), max=round(runs[-1], 1))


def child(a):
    import torch
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    kw = SHAPES[a.shape]
    m, tr = make(a.shape)
    rows = {}
    for n in ENVS:
        envs = [SyntheticSafeEnv(kw["od"], kw["ad"], EPISODE_LEN, seed=1 + e) for e in range(n)]
        waves = max(1, a.episodes // n)  # the same number of environment steps for every N and both ways
        row = dict(envs=n, waves=waves, env_steps=waves * n * EPISODE_LEN)
        for name, fn in (("lockstep", lockstep), ("sequential", sequential)):
            fn(tr, envs, 1)  # warm-up: handles, code objects
            torch.cuda.synchronize()
            row[name] = stats([fn(tr, envs, waves) for _ in range(a.repeats)])
        lo, se = row["lockstep"], row["sequential"]
        spread = max(lo["max"] - lo["min"], se["max"] - se["min"])
        row["spread"] = round(spread, 1)
        row["lockstep_ahead"] = bool(lo["median"] - se["median"] > spread)
        row["sequential_ahead"] = bool(se["median"] - lo["median"] > spread)
        rows[str(n)] = row
        print(a.shape, json.dumps(row), flush=True)
    with open(a.child_out, "w") as f:
        json.dump(dict(SHAPES[a.shape], episode_len=EPISODE_LEN, device=torch.cuda.get_device_name(0), rows=rows), f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_act_vec_bench.json"))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=128, help="episodes per repetition (rounded down to waves of N)")
    ap.add_argument("--limit", type=int, default=240, help="seconds one shape's child process may take")
    ap.add_argument("--shape", default=None, help=argparse.SUPPRESS)  # child mode
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.shape:
        return child(a)
    res = dict(repeats=a.repeats, unit="env-steps/s", shapes={})
    with tempfile.TemporaryDirectory() as d:
        for shape in a.shapes.split(","):
            out = os.path.join(d, shape + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--child-out", out, "--repeats",
                   str(a.repeats), "--episodes", str(a.episodes)]
            try:
                rc = subprocess.run(cmd, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"{shape}: exit status {rc}; stopping, nothing written", file=sys.stderr)
                sys.exit(rc if 0 < rc < 256 else 1)
            with open(out) as f:
                res["shapes"][shape] = json.load(f)
    res["device"] = next(iter(res["shapes"].values())).pop("device") if res["shapes"] else None
    for v in res["shapes"].values():
        v.pop("device", None)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
