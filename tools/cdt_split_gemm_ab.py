#!/usr/bin/env python3
"""A/B of the "bf16x3" projections (osrl_linear_split, csrc/linear_split.hip) against the f32-MFMA path (osrl_linear).

Per C5 projection shape (M = 81920 token rows): device-event times of osrl_linear and osrl_linear_split on the same
inputs, taken as interleaved pairs (A B A B ...: both sides of a pair see the same clocks and neighbours), the time of
the osrl_split_planes refresh of that weight, and the rms / max error of both kernels and of fp32
torch.nn.functional.linear on the CPU against an fp64 product of the same inputs (first --err-rows rows).
Whole step: CDTTrainer(matmul="f32") against CDTTrainer(matmul="bf16x3") at C5 (B 1024, T 20, E 256, 8 heads, 3
layers, dropout 0.1) on replayed graphs, interleaved pairs of --steps steps each.  osrl_linear and the f32 step are
untouched by the bf16x3 work (csrc/mlp.hip is not part of it), so the "f32" side IS the baseline path.
Writes profiles/cdt_split_gemm_ab.json (--out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cases import CDTCase, make_cdt_batch  # noqa: E402
from osrl_amd import _lib as L  # noqa: E402
from osrl_amd.algorithms import CDT, CDTTrainer  # noqa: E402
from osrl_amd.common.logger import DummyLogger  # noqa: E402
from osrl_amd.engine.core import FlatGroup, cur_stream  # noqa: E402

DEV = "cuda:0"
C5 = CDTCase("c5", od=11, ad=3, B=1024, T=20, E=256, heads=8, layers=3, episode_len=1000, dropout=0.1, seed=6)
# (name, K, N, residual): the five projection shapes of a C5 block step (forward and dX forms)
SHAPES = [("K256_N1024", 256, 1024, False), ("K256_N768", 256, 768, False), ("K1024_N256_resid", 1024, 256, True),
          ("K256_N256_resid", 256, 256, True), ("K768_N256", 768, 256, False)]


def r16(x):
    return (x + 15) // 16 * 16


def ev_time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per call


def shape_ab(name, K, N, resid, M, pairs, reps, err_rows):
    lib = L.load()
    rs = np.random.RandomState(K * 7 + N)
    A = (rs.randn(M, K) * 1.5).astype(np.float32)
    W = (rs.randn(N, K) * 0.05).astype(np.float32)
    b = (rs.randn(N) * 0.1).astype(np.float32)
    R = rs.randn(M, N).astype(np.float32) if resid else None
    g = FlatGroup("ab", DEV)
    g.add("w", (N, K))
    g.add("b", (N,))
    g.mark_weight("w")
    g.finalize()
    g.view("w").copy_(torch.from_numpy(W))
    g.view("b").copy_(torch.from_numpy(b))
    g.repack()
    g.enable_planes(["w"], [])
    At = torch.from_numpy(A).to(DEV)
    Rt = None if R is None else torch.from_numpy(R).to(DEV)
    Yf, Ys = torch.zeros(M, N, device=DEV), torch.zeros(M, N, device=DEV)
    rp = None if Rt is None else Rt.data_ptr()

    def f32():
        L.check(lib.osrl_linear(At.data_ptr(), K, M, K, g.pf.data_ptr(), r16(N), 0, N, g.view("b").data_ptr(), rp, N,
                                Yf.data_ptr(), N, cur_stream()), "osrl_linear")

    def split():
        L.check(lib.osrl_linear_split(At.data_ptr(), K, M, K, g.planes_w.data_ptr(), N * K, N, g.view("b").data_ptr(), rp, N,
                                      Ys.data_ptr(), N, cur_stream()), "osrl_linear_split")

    for _ in range(3):  # warm both
        f32()
        split()
        g.refresh_planes()
    torch.cuda.synchronize()
    pr = []
    for _ in range(pairs):
        pr.append((ev_time(f32, reps), ev_time(split, reps)))
    planes_us = ev_time(g.refresh_planes, reps)
    n = min(err_rows, M)
    y64 = A[:n].astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    yc = torch.nn.functional.linear(torch.from_numpy(A[:n]), torch.from_numpy(W), torch.from_numpy(b))
    if R is not None:
        y64 += R[:n].astype(np.float64)
        yc = yc + torch.from_numpy(R[:n])
    err = lambda y: np.asarray(y, np.float64) - y64  # noqa: E731
    stat = lambda e: dict(rms=float(np.sqrt(np.mean(e ** 2))), max=float(np.abs(e).max()))  # noqa: E731
    gf = 2.0 * M * K * N * 1e-9
    f_med, s_med = float(np.median([p[0] for p in pr])), float(np.median([p[1] for p in pr]))
    row = dict(shape=name, M=M, K=K, N=N, resid=resid, gflop=gf, pairs_us=[[round(a, 2), round(c, 2)] for a, c in pr],
               osrl_linear_us=f_med, osrl_linear_split_us=s_med, split_over_f32=s_med / f_med,
               osrl_linear_tflops=gf * 1e3 / f_med, osrl_linear_split_tflops_equiv=gf * 1e3 / s_med,
               split_planes_us=planes_us,
               err_vs_fp64=dict(rows=n, osrl_linear_split=stat(err(Ys[:n].cpu().numpy())),
                                cpu_f32_linear=stat(err(yc.numpy())),
                                osrl_linear_not_gated=stat(err(Yf[:n].cpu().numpy()))))
    print(json.dumps({k: v for k, v in row.items() if k != "pairs_us"}), flush=True)
    return row


def make_trainer(matmul):
    c = C5
    m = CDT(c.od, c.ad, 1.0, seq_len=c.T, episode_len=c.episode_len, embedding_dim=c.E, num_layers=c.layers,
            num_heads=c.heads, attention_dropout=c.dropout, residual_dropout=c.dropout, embedding_dropout=c.dropout,
            use_rew=True, use_cost=True, cost_transform=True, stochastic=True, target_entropy=-c.ad, device=DEV)
    tr = CDTTrainer(m, None, DummyLogger(), loss_cost_weight=0.02, device=DEV, stats_mode="none", use_graph=True,
                    matmul=matmul)
    return m, tr


def step_ab(pairs, steps):
    b = {k: torch.as_tensor(v, device=DEV) for k, v in make_cdt_batch(C5).items()}
    args = (b["states"], b["actions"], b["returns"], b["costs_return"], b["time_steps"], b["mask"], b["episode_cost"],
            b["costs"])
    torch.manual_seed(0)
    side = {k: make_trainer(k) for k in ("f32", "bf16x3")}

    def run(k):
        tr = side[k][1]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.train_one_step(*args)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps  # ms per step

    for k in side:  # capture + warm
        for _ in range(3):
            side[k][1].train_one_step(*args)
    pr = [(run("f32"), run("bf16x3")) for _ in range(pairs)]
    plans = {k: vars(side[k][0]._engine.plan) for k in side}
    f_med, s_med = float(np.median([p[0] for p in pr])), float(np.median([p[1] for p in pr]))
    row = dict(config="c5", steps_per_sample=steps, pairs_ms=[[round(a, 4), round(c, 4)] for a, c in pr], f32_ms=f_med,
               bf16x3_ms=s_med, bf16x3_over_f32=s_med / f_med, plans=plans)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=81920)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--err-rows", type=int, default=2048)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdt_split_gemm_ab.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cdt_split_gemm_ab: needs the GPU (no CPU timing)")
    res = dict(device=torch.cuda.get_device_name(0), lease="one process, one device lease; A/B pairs interleaved",
               method="device events around `reps` back-to-back launches per sample (kernels); host clock around "
                      "`steps` replayed graphs ending in a device synchronise (step); medians over the pairs",
               reps=a.reps, shapes=[shape_ab(n, K, N, r, a.rows, a.pairs, a.reps, a.err_rows) for n, K, N, r in SHAPES])
    torch.cuda.empty_cache()
    if not a.no_step:
        res["step"] = step_ab(a.pairs, a.steps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
