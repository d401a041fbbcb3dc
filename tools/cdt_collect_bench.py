"""CDT in the collect -> store -> train -> evaluate loop, measured in one session with interleaved repeats, at C5's model
shape (obs 11, act 3, seq_len 20, embedding 256, 8 heads, 3 layers) on a VecSyntheticSafeEnv of 200-step episodes:

(a) ``evaluate`` of this tree against ``evaluate`` of a built checkout of the parent commit (``--parent DIR``; skipped
    without it), 256 and 1024 episodes, as child processes alternating A B B A: the per-episode-target reset must cost
    nothing.  ``ratio`` = parent median / this tree's median (1.0: equal, below 1: this tree is slower);
    ``parent_spread`` = (max - min) / median of the parent's own repeats; ``ok``: this tree's median is not above the
    parent's by more than that spread.
(b) ``collect_targets(sample=True)`` against ``evaluate`` of this tree, same episodes (one launch after the forward plus
    the table writes, against four launches);
(c) a 25-target grid x 10 rollouts as ONE rollout of 250 episodes against 25 rollouts of 10 episodes.

Every repeat is kept.  Writes profiles/cdt_collect_bench.json (``--out``)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(od=11, ad=3, T=20, E=256, heads=8, layers=3)
EPISODE_LEN = 200
GRID = [(float(r), float(c)) for r in (100, 200, 300, 400, 500) for c in (5, 10, 20, 40, 80)]


def summary(v):
    s = sorted(v)
    return dict(min=round(s[0], 3), median=round(s[len(s) // 2], 3), max=round(s[-1], 3), n=len(s), all=[round(x, 3) for x in v])


def make_trainer(episodes):
    import torch
    from osrl_amd.algorithms import CDT, CDTTrainer
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv, VecSyntheticSafeEnv
    s = SHAPE
    torch.manual_seed(0)
    m = CDT(s["od"], s["ad"], 1.0, seq_len=s["T"], episode_len=EPISODE_LEN, embedding_dim=s["E"], num_layers=s["layers"],
            num_heads=s["heads"], use_rew=True, use_cost=True, cost_transform=True, stochastic=True, target_entropy=-s["ad"],
            device="cuda:0")
    tr = CDTTrainer(m, None, None, learning_rate=1e-4, lr_warmup_steps=500, stats_mode="none")
    tr.env = VecSyntheticSafeEnv(SyntheticSafeEnv(s["od"], s["ad"], EPISODE_LEN, seed=3, init_noise=0.5), episodes, "cuda:0",
                                 base_seed=100)
    return tr


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def worker(tree, what, reps):
    """Runs in a child process with ``tree`` first on the path: ms per call, every repeat."""
    sys.path.insert(0, tree)
    out = {}
    if what == "evaluate":
        for n in (256, 1024):
            tr = make_trainer(n)
            tr.evaluate(n, 300.0, 10.0)  # captures
            out[str(n)] = [timed(lambda: tr.evaluate(n, 300.0, 10.0)) for _ in range(reps)]
    elif what == "collect":
        for n in (256, 1024):
            tr = make_trainer(n)
            tr.evaluate(n, 300.0, 10.0)
            tr.collect_targets(300.0, 10.0, sample=True, seed=0)
            ev, co = [], []
            for i in range(reps):  # A B B A
                order = (ev, co, co, ev) if i % 2 == 0 else (co, ev, ev, co)
                for dst in order:
                    dst.append(timed((lambda: tr.evaluate(n, 300.0, 10.0)) if dst is ev else
                                     (lambda: tr.collect_targets(300.0, 10.0, sample=True, seed=i))))
            out[str(n)] = dict(evaluate_ms=ev, collect_targets_ms=co)
    else:
        k = 10
        one, many = make_trainer(k * len(GRID)), make_trainer(k)
        one.evaluate_targets(k, GRID)
        many.evaluate_targets(k, GRID)
        a, b = [], []
        for i in range(reps):
            order = (a, b, b, a) if i % 2 == 0 else (b, a, a, b)
            for dst in order:
                dst.append(timed(lambda: (one if dst is a else many).evaluate_targets(k, GRID)))
        out = dict(targets=len(GRID), rollouts_per_target=k, one_rollout_ms=a, one_rollout_per_target_ms=b)
    print("RESULT " + json.dumps(out))


def child(tree, what, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--tree", tree, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tree)
    if r.returncode != 0:
        raise RuntimeError(f"worker {what} failed in {tree}: {r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def against_parent(parent, reps, rounds):
    here, there = {"256": [], "1024": []}, {"256": [], "1024": []}
    for _ in range(rounds):  # A B B A
        for tree, dst in ((ROOT, here), (parent, there), (parent, there), (ROOT, here)):
            for n, v in child(tree, "evaluate", reps).items():
                dst[n] += v
    out = {}
    for n in here:
        h, t = summary(here[n]), summary(there[n])
        spread = (t["max"] - t["min"]) / t["median"]
        out[n] = dict(episodes=int(n), this_tree_ms=h, parent_ms=t, ratio=round(t["median"] / h["median"], 4),
                      parent_spread=round(spread, 4), ok=h["median"] <= t["median"] * (1 + spread))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdt_collect_bench.json"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part a)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="A B B A rounds of part (a): 4 child processes per tree each")
    ap.add_argument("--worker", default=None, choices=["evaluate", "collect", "grid"])
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.tree), args.worker, args.reps)
    out = dict(shape=dict(SHAPE, episode_len=EPISODE_LEN), evaluate_vs_parent=None)
    if args.parent:
        out["evaluate_vs_parent"] = against_parent(os.path.abspath(args.parent), args.reps, args.rounds)
    co = child(ROOT, "collect", args.reps)
    out["collect_vs_evaluate"] = {n: dict(evaluate_ms=summary(v["evaluate_ms"]), collect_targets_ms=summary(v["collect_targets_ms"]))
                                  for n, v in co.items()}
    g = child(ROOT, "grid", max(2, args.reps // 2))
    out["grid"] = dict(targets=g["targets"], rollouts_per_target=g["rollouts_per_target"],
                       one_rollout_ms=summary(g["one_rollout_ms"]), one_rollout_per_target_ms=summary(g["one_rollout_per_target_ms"]))
    import torch  # (after the children: this process never opens the device before them)
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
