#!/usr/bin/env python3
"""Env-steps/s of CDTTrainer.rollout on a host environment (SyntheticSafeEnv): the act latency path
(fast_rollout=True, csrc/cdt_act.hip) against the existing loop (fast_rollout=False), in one process on one device.
Shapes: C5's CDT (od 11, ad 3, seq_len 20, E 256, 3 layers, 8 heads, all tokens, cost_transform, stochastic) with
100-step episodes, and the reference's default model (E 128, seq_len 10) with 300-step episodes.
Writes profiles/cdt_act_bench.json (--out).  --trace: one fast C5 episode only (for rocprofv3 --kernel-trace)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdt_act_bench.json"))
    ap.add_argument("--fast-episodes", type=int, default=20)
    ap.add_argument("--loop-episodes", type=int, default=2)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
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
