#!/usr/bin/env python3
"""Time of the differentiable CDT forward + backward (CDT(..., differentiable=True), ops.cdt_apply) against the fused
CDTTrainer step, at C5's shape (B 1024, seq_len 20, E 256, 8 heads, 3 layers, dropout 0.1, train mode).

Rows: the fused step replayed from its hipGraph (bench.py's path) and run eagerly; the differentiable forward alone;
forward + the reference's training loss in torch (cdt.py:355-395) + loss.backward(); the same + torch.optim.AdamW.step()
on model.parameters().  Writes profiles/cdt_autograd_probe.json (--out)."""
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
from osrl_amd.algorithms import CDT, CDTTrainer  # noqa: E402
from osrl_amd.common.logger import DummyLogger  # noqa: E402

DEV = "cuda:0"
C5 = CDTCase("c5", od=11, ad=3, B=1024, T=20, E=256, heads=8, layers=3, episode_len=1000, dropout=0.1, seed=6)


def make(use_graph):
    torch.manual_seed(0)
    c = C5
    m = CDT(c.od, c.ad, 1.0, seq_len=c.T, episode_len=c.episode_len, embedding_dim=c.E, num_layers=c.layers,
            num_heads=c.heads, attention_dropout=c.dropout, residual_dropout=c.dropout, embedding_dropout=c.dropout,
            use_rew=True, use_cost=True, cost_transform=True, stochastic=True, target_entropy=-c.ad, device=DEV,
            differentiable=True)
    tr = CDTTrainer(m, None, DummyLogger(), loss_cost_weight=0.02, device=DEV, stats_mode="none", use_graph=use_graph)
    return m, tr


def loss_of(m, b, temp):
    ap, lp, sp = m(b["states"], b["actions"], b["returns"], b["costs_return"], b["time_steps"],
                   ~b["mask"].to(torch.bool), b["episode_cost"])
    mask = b["mask"]
    sel = mask > 0
    act = -(ap.log_prob(b["actions"])[sel].mean() + temp * ap.entropy()[sel].mean())
    cl = (torch.nn.functional.nll_loss(lp.reshape(-1, 2), b["costs"].flatten().long(), reduction="none")
          * mask.flatten()).mean()
    sl = ((sp[:, :-1] - b["states"][:, 1:]) ** 2 * mask[:, :-1].unsqueeze(-1)).mean()
    return act + 0.02 * cl + 0.0 * sl


def timed(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return dict(ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), iters=iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdt_autograd_probe.json"))
    a = ap.parse_args()
    b = {k: torch.as_tensor(v, device=DEV) for k, v in make_cdt_batch(C5).items()}
    args = (b["states"], b["actions"], b["returns"], b["costs_return"], b["time_steps"], b["mask"], b["episode_cost"],
            b["costs"])
    rows = {}
    for use_graph in (True, False):
        m, tr = make(use_graph)
        rows["fused_step_graph" if use_graph else "fused_step_eager"] = timed(lambda: tr.train_one_step(*args),
                                                                               a.iters, a.warmup)
        del m, tr
        torch.cuda.empty_cache()
    m, tr = make(False)
    m.train()
    temp = float(m.temperature())

    def fwd():
        with torch.enable_grad():
            loss_of(m, b, temp)

    def fwd_bwd():
        m.zero_grad(set_to_none=True)
        loss_of(m, b, temp).backward()

    opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)

    def fwd_bwd_opt():
        opt.zero_grad(set_to_none=True)
        loss_of(m, b, temp).backward()
        opt.step()

    rows["diff_forward_and_loss"] = timed(fwd, a.iters, a.warmup)
    rows["diff_forward_backward"] = timed(fwd_bwd, a.iters, a.warmup)
    rows["diff_forward_backward_adamw"] = timed(fwd_bwd_opt, a.iters, a.warmup)
    ref = rows["fused_step_graph"]["ms_median"]
    out = dict(shape=dict(B=C5.B, T=C5.T, E=C5.E, heads=C5.heads, layers=C5.layers, dropout=C5.dropout),
               device=torch.cuda.get_device_name(0), rows=rows,
               ratio_forward_backward_vs_fused_graph=rows["diff_forward_backward"]["ms_median"] / ref,
               ratio_forward_backward_vs_fused_eager=rows["diff_forward_backward"]["ms_median"]
               / rows["fused_step_eager"]["ms_median"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
