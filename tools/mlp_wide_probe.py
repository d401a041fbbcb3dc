"""Wide-MLP measurements (not part of bench.py): train-step rate of CPQ / BCQ-Lag with reference-sized hidden widths
(the per-layer wide path of include/osrl_amd.h), and the wide layer launches' fraction of the fp32 MFMA roof.
python tools/mlp_wide_probe.py [--steps N] [--skip-train]
Prints one JSON line per measurement.  Layer FLOPs: 2 * M * K * N (algorithmic, no padding)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP32_MFMA_TFLOPS = 157.3  # MI355X dense fp32 matrix peak


def train_rate(algo, od, ad, B, N, hidden, vae_hidden, steps):
    from osrl_amd.algorithms import BCQL, CPQ, BCQLTrainer, CPQTrainer
    from osrl_amd.common.replay import ReplayStore, synthetic_transitions
    dev = "cuda:0"
    torch.manual_seed(0)
    if algo == "cpq":
        m = CPQ(od, ad, 1.0, hidden, hidden, vae_hidden, N, 0.99, 0.005, 0.5, 2, 2, 1.5, 10, 1000, device=dev)
        CPQTrainer(m, None, None, actor_lr=1e-4, critic_lr=1e-3, alpha_lr=1e-4, vae_lr=1e-3, reward_scale=0.1,
                   cost_scale=1.0, device=dev, stats_mode="none")
    else:
        m = BCQL(od, ad, 1.0, hidden, hidden, vae_hidden, N, 0.99, 0.005, 0.05, 0.75, 0.5, [0.1, 0.003, 0.001], 2, 2, 10,
                 1000, device=dev)
        BCQLTrainer(m, None, None, 1e-3, 1e-3, 1e-3, stats_mode="none")
    eng = m.engine(B)
    eng.attach_replay(ReplayStore(synthetic_transitions(100_000, od, ad, seed=1), torch.device(dev), reward_scale=0.1,
                                  cost_scale=1.0, seed=3))
    spg = int(eng.plan.steps_per_graph)
    eng.steps_replay(2 * spg)
    torch.cuda.synchronize()
    n = max(steps // spg, 1) * spg
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    eng.steps_replay(n)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    return dict(what="train_step", algo=algo, od=od, ad=ad, B=B, N=N, hidden=hidden, vae_hidden=vae_hidden,
                steps_per_graph=spg, ms_per_step=round(ms, 3), steps_per_s=round(1000 / ms, 1))


def _net(dims, acts, dev, seed=0):
    from osrl_amd.engine.core import FlatGroup, LayerRef, NetDesc
    rs = np.random.RandomState(seed)
    g = FlatGroup("probe", dev)
    for l in range(len(dims) - 1):
        g.add(f"w{l}", (dims[l + 1], dims[l]))
        g.mark_weight(f"w{l}")
        g.add(f"b{l}", (dims[l + 1],))
    g.finalize()
    refs = []
    for l in range(len(dims) - 1):
        k = 1 / math.sqrt(dims[l])
        W, b = g.view(f"w{l}"), g.view(f"b{l}")
        W.copy_(torch.tensor(rs.uniform(-k, k, W.shape), dtype=torch.float32))
        b.copy_(torch.tensor(rs.uniform(-k, k, b.shape), dtype=torch.float32))
        refs.append(LayerRef(W, b, g, f"w{l}", f"b{l}"))
    g.repack()
    return g, NetDesc([refs], acts)


def _time(fn, reps=50):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def layer_fractions(M, K, N):
    """The forward layer launch (relu epilogue) and the backward-dZ layer launch (act' epilogue) on [M, K] x [K, N]."""
    from osrl_amd.engine.core import MlpRun
    dev = torch.device("cuda:0")
    flop = 2.0 * M * K * N
    out = []
    _, d1 = _net([K, N], ["relu"], dev)
    x = torch.randn(M, K, device=dev)
    r1 = MlpRun(d1, M, False, dev)
    us = _time(lambda: r1.forward(x))
    out.append(dict(what="wide_layer", launch="forward", M=M, K=K, N=N, us=round(us, 1),
                    frac_fp32_mfma=round(flop / (us * 1e-6) / 1e12 / FP32_MFMA_TFLOPS, 4)))
    # backward-dZ layer launch: dZ_0 = (dZ_1 W_1) * relu'(h_0) of the net [8, N, K] (contraction over K, N outputs), timed
    # as the whole backward (the element-wise dZ_1 launch over [M, K] + the layer launch) minus the dZ_1 launch alone
    # (the same call with dz[0] NULL: the wide path then stops at dZ_1)
    from osrl_amd import _lib as L
    from osrl_amd.engine.core import cur_stream
    import ctypes as C
    _, d2 = _net([8, N, K], ["relu", "id"], dev)
    x2 = torch.randn(M, 8, device=dev)
    r2 = MlpRun(d2, M, True, dev)
    r2.forward(x2)
    r2.setup_backward(torch.randn(1, M, K, device=dev))
    g_top = L.GradsT.from_buffer_copy(r2.grads_c)
    g_top.dz[0][0] = None
    lib = L.load()
    us_all = _time(lambda: r2.backward_dz())
    us_top = _time(lambda: L.check(lib.osrl_mlp_backward_dz(C.byref(r2.bwd_net.c), M, C.byref(r2.saved_c), C.byref(g_top),
                                                            cur_stream()), "osrl_mlp_backward_dz"))
    us = us_all - us_top
    out.append(dict(what="wide_layer", launch="backward_dz", M=M, K=K, N=N, us=round(us, 1), us_with_dy=round(us_all, 1),
                    frac_fp32_mfma=round(flop / (us * 1e-6) / 1e12 / FP32_MFMA_TFLOPS, 4)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    for M, K, N in ((20480, 1024, 1024), (2048, 1024, 1024), (20480, 512, 512), (2048, 750, 750)):
        for r in layer_fractions(M, K, N):
            print(json.dumps(r), flush=True)
    if not args.skip_train:
        for a in (("cpq", 76, 2, 2048, 10, [512, 512], 750), ("cpq", 76, 2, 2048, 10, [1024, 1024], 1024),
                  ("bcql", 33, 8, 4096, 10, [512, 512], 750)):
            print(json.dumps(train_rate(*a, args.steps)), flush=True)


if __name__ == "__main__":
    main()
