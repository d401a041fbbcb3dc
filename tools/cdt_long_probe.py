"""Long-sequence / wide-embedding CDT measurements (not part of bench.py): train-step rate at user sizes and the tiled
attention kernels against the register-tile ones.  python tools/cdt_long_probe.py [--steps N]
Prints one JSON line per measurement.  Attention FLOPs: 4 * S^2 * d / 2 per (sample, head) and pass (causal half)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP32_MFMA_TFLOPS = 157.3  # MI355X dense fp32 matrix peak


def train_rate(B, seq_len, E, H, layers, p, steps):
    from osrl_amd.algorithms import CDT, CDTTrainer
    from osrl_amd.common.logger import DummyLogger
    od, ad, dev = 11, 3, "cuda:0"
    torch.manual_seed(0)
    m = CDT(od, ad, 1.0, seq_len=seq_len, episode_len=1000, embedding_dim=E, num_layers=layers, num_heads=H,
            attention_dropout=p, residual_dropout=p, embedding_dropout=p, use_rew=True, use_cost=True, device=dev)
    tr = CDTTrainer(m, None, DummyLogger(), device=dev, stats_mode="lazy", use_graph=True)
    rs = np.random.RandomState(0)
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    b = (f(rs.randn(B, seq_len, od).astype(np.float32)), f(rs.uniform(-1, 1, (B, seq_len, ad)).astype(np.float32)),
         f(rs.uniform(0, 10, (B, seq_len)).astype(np.float32)), f(rs.uniform(0, 20, (B, seq_len)).astype(np.float32)),
         f(np.tile(np.arange(seq_len), (B, 1)).astype(np.int64)), f(np.ones((B, seq_len), np.float32)),
         f(np.full(B, 5.0, np.float32)), f((rs.rand(B, seq_len) < 0.1).astype(np.float32)))
    for _ in range(3):
        tr.train_one_step(*b)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        tr.train_one_step(*b)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    S, M = 4 * seq_len, B * 4 * seq_len
    # executed FLOPs: 12 E^2 per token and layer (QKV 3, out 1, MLP 8) x 3 (fwd + dX + dW); attention fwd 2 + bwd 5
    # matrix products of S^2 d / 2 (causal) per (sample, head), 2 FLOP per multiply-add
    gemm = 3 * 2 * 12 * E * E * M * layers
    attn = 7 * 2 * (S * S / 2) * (E // H) * B * H * layers
    return dict(what="train_step", B=B, S=S, E=E, H=H, layers=layers, dropout=p, ms_per_step=round(ms, 3),
                steps_per_s=round(1000 / ms, 2), frac_fp32_mfma=round((gemm + attn) / (ms * 1e-3) / 1e12 / FP32_MFMA_TFLOPS, 4))


def attn_times(B, S, E, H, rep, p, tiled, reps=20):
    from osrl_amd import _lib as L
    from osrl_amd.engine.core import StepState, cur_stream
    lib = L.load()
    dev = torch.device("cuda:0")
    st = StepState(dev, ["x"])
    st.tick()
    qkv, do = torch.randn(B, S, 3 * E, device=dev), torch.randn(B, S, E, device=dev)
    mk = torch.ones(B, S // rep, device=dev)
    o, dq = torch.empty(B, S, E, device=dev), torch.empty(B, S, 3 * E, device=dev)
    n = max(1, int(lib.osrl_attention_tiled_ws_bytes(B, S, E, H)) // 4)
    lse, ws = torch.empty(n, device=dev), torch.empty(n, device=dev)
    dr = L.DropoutT(p, 9, 13, st.ptr)
    drp = C.byref(dr) if p > 0 else None
    a = (qkv.data_ptr(), mk.data_ptr())

    def fwd():
        if tiled:
            L.check(lib.osrl_attention_fwd_ws(*a, B, S, E, H, rep, 0, drp, o.data_ptr(), lse.data_ptr(), cur_stream()), "f")
        else:
            L.check(lib.osrl_attention_fwd(*a, B, S, E, H, rep, 0, drp, o.data_ptr(), cur_stream()), "f")

    def bwd():
        if tiled:
            L.check(lib.osrl_attention_bwd_ws(*a, do.data_ptr(), B, S, E, H, rep, 0, drp, o.data_ptr(), lse.data_ptr(),
                                              ws.data_ptr(), dq.data_ptr(), cur_stream()), "b")
        else:
            L.check(lib.osrl_attention_bwd(*a, do.data_ptr(), B, S, E, H, rep, 0, drp, dq.data_ptr(), cur_stream()), "b")

    out = {}
    for nm, fn in (("fwd", fwd), ("bwd", bwd)):
        fwd()
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        flop = (2 if nm == "fwd" else 5) * 2 * (S * S / 2) * (E // H) * B * H
        out[nm + "_us"] = round(us, 1)
        out[nm + "_frac_fp32_mfma"] = round(flop / (us * 1e-6) / 1e12 / FP32_MFMA_TFLOPS, 4)
    return dict(what="attention", kernels="tiled" if tiled else "register-tile", B=B, S=S, E=E, H=H, dropout=p, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    rows = []
    if not args.skip_train:
        rows.append(train_rate(256, 64, 512, 8, 3, 0.1, args.steps))
        rows.append(train_rate(64, 256, 512, 8, 3, 0.1, args.steps))
    rows.append(attn_times(256, 256, 512, 8, 4, 0.1, True))
    rows.append(attn_times(64, 1024, 512, 8, 4, 0.1, True))
    rows.append(attn_times(1024, 80, 256, 8, 4, 0.1, False))
    rows.append(attn_times(1024, 80, 256, 8, 4, 0.1, True))
    for r in rows:
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
