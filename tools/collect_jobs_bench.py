"""``collect_jobs`` (noisy rollouts on host environments, recorded), measured in one session with interleaved repeats:

(a) the untouched paths of this tree against a built checkout of the parent commit (``--parent DIR``; skipped without
    it), as child processes alternating A B B A: ``rollout_many`` of a CPQ policy at C2's shape -- (obs, act) = (76, 2),
    hidden [256, 256] -- on 64 ``SyntheticSafeEnv``s of 200 steps, and CDT ``rollout_many`` at C5's model shape (obs 11,
    act 3, seq_len 20, embedding 256, 8 heads, 3 layers) on 16 of 100 steps.  The act kernels gained a branch that these
    calls do not take.  ``ratio`` = parent median / this tree's median (1.0: equal, below 1: this tree is slower);
    ``parent_spread`` = (max - min) / median of the parent's own repeats; ``ok``: this tree's median is not above the
    parent's by more than that spread.
(b) the recorder's own cost: ``collect_jobs(noise_std=0.3)`` against ``rollout_jobs``, same tree, same environments and
    jobs (one job per environment), A B B A in one process.  The difference is host bookkeeping plus one upload:
    reported as a ratio, not gated.

Every number is ms per call; every repeat is kept.  Writes profiles/collect_jobs_bench.json (``--out``).  Needs an
MI355X: there is no CPU path."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MLP = dict(od=76, ad=2, hidden=[256, 256], envs=64, episode_len=200)
CDT = dict(od=11, ad=3, T=20, E=256, heads=8, layers=3, envs=16, episode_len=100)


def summary(v):
    s = sorted(v)
    return dict(min=round(s[0], 3), median=round(s[len(s) // 2], 3), max=round(s[-1], 3), n=len(s), all=[round(x, 3) for x in v])


def make_mlp():
    import torch
    from osrl_amd.algorithms import CPQ, CPQTrainer
    from osrl_amd.common.logger import DummyLogger
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    s = MLP
    torch.manual_seed(0)
    m = CPQ(s["od"], s["ad"], 1.0, s["hidden"], s["hidden"], 400, 10, episode_len=s["episode_len"], device="cuda:0")
    tr = CPQTrainer(m, None, DummyLogger(), 1e-4, 1e-3, 1e-4, 1e-3, device="cuda:0", stats_mode="none")
    envs = [SyntheticSafeEnv(s["od"], s["ad"], s["episode_len"], seed=1, init_noise=0.5) for _ in range(s["envs"])]
    return tr, envs


def make_cdt():
    import torch
    from osrl_amd.algorithms import CDT as Model
    from osrl_amd.algorithms import CDTTrainer
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    s = CDT
    torch.manual_seed(0)
    m = Model(s["od"], s["ad"], 1.0, seq_len=s["T"], episode_len=s["episode_len"], embedding_dim=s["E"],
              num_layers=s["layers"], num_heads=s["heads"], use_rew=True, use_cost=True, cost_transform=True,
              stochastic=True, target_entropy=-s["ad"], device="cuda:0")
    m.eval()
    tr = CDTTrainer(m, None, None, learning_rate=1e-4, lr_warmup_steps=500, stats_mode="none")
    envs = [SyntheticSafeEnv(s["od"], s["ad"], s["episode_len"], seed=3, init_noise=0.5) for _ in range(s["envs"])]
    return tr, envs


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def worker(tree, what, reps):
    """Runs in a child process with ``tree`` first on the path: ms per call, every repeat."""
    sys.path.insert(0, tree)
    out = {}
    if what == "rollout":
        tr, envs = make_mlp()
        tr.rollout_many(envs)
        out["mlp"] = [timed(lambda: tr.rollout_many(envs)) for _ in range(reps)]
        ct, cenvs = make_cdt()
        n = len(cenvs)
        ct.rollout_many(ct.model, cenvs, [300.0] * n, [10.0] * n)
        out["cdt"] = [timed(lambda: ct.rollout_many(ct.model, cenvs, [300.0] * n, [10.0] * n)) for _ in range(reps)]
    else:
        tr, envs = make_mlp()
        ct, cenvs = make_cdt()
        n = len(cenvs)
        arms = dict(
            mlp=(lambda: tr.rollout_jobs(envs, len(envs)), lambda i: tr.collect_jobs(envs, len(envs), 0.3, seed=i)),
            cdt=(lambda: ct.rollout_jobs(ct.model, cenvs, [300.0] * n, [10.0] * n),
                 lambda i: ct.collect_jobs(ct.model, cenvs, [300.0] * n, [10.0] * n, noise_std=0.3, seed=i)))
        for name, (ro, co) in arms.items():
            ro()
            co(0)
            a, b = [], []
            for i in range(reps):  # A B B A
                order = (a, b, b, a) if i % 2 == 0 else (b, a, a, b)
                for dst in order:
                    dst.append(timed(ro if dst is a else (lambda: co(i))))
            out[name] = dict(rollout_jobs_ms=a, collect_jobs_ms=b)
    print("RESULT " + json.dumps(out))


def child(tree, what, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--tree", tree, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tree)
    if r.returncode != 0:
        raise RuntimeError(f"worker {what} failed in {tree}: {r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def against_parent(parent, reps, rounds):
    here, there = {"mlp": [], "cdt": []}, {"mlp": [], "cdt": []}
    for _ in range(rounds):  # A B B A
        for tree, dst in ((ROOT, here), (parent, there), (parent, there), (ROOT, here)):
            for k, v in child(tree, "rollout", reps).items():
                dst[k] += v
    out = {}
    for k in here:
        h, t = summary(here[k]), summary(there[k])
        spread = (t["max"] - t["min"]) / t["median"]
        out[k] = dict(this_tree_ms=h, parent_ms=t, ratio=round(t["median"] / h["median"], 4),
                      parent_spread=round(spread, 4), ok=h["median"] <= t["median"] * (1 + spread))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collect_jobs_bench.json"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part a)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="A B B A rounds of part (a): 4 child processes per tree each")
    ap.add_argument("--worker", default=None, choices=["rollout", "collect"])
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.tree), args.worker, args.reps)
    out = dict(shapes=dict(mlp=MLP, cdt=CDT), rollout_many_vs_parent=None)
    if args.parent:
        out["rollout_many_vs_parent"] = against_parent(os.path.abspath(args.parent), args.reps, args.rounds)
    co = child(ROOT, "collect", args.reps)
    out["collect_jobs_vs_rollout_jobs"] = {}
    for k, v in co.items():
        a, b = summary(v["rollout_jobs_ms"]), summary(v["collect_jobs_ms"])
        out["collect_jobs_vs_rollout_jobs"][k] = dict(rollout_jobs_ms=a, collect_jobs_ms=b,
                                                      ratio=round(b["median"] / a["median"], 4))
    import torch  # (after the children: this process never opens the device before them)
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
