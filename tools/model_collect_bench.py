"""Recorded model rollouts (``collect_model``, engine/collect.py ``ModelCollector``) measured in one session with
interleaved repeats (A B B A), medians.  The shape is C2's: a CPQ policy at (obs, act) = (76, 2), hidden [256, 256], on a
``ModelVecEnv`` of 5 members with hidden [200, 200, 200] and 1024 episodes.

(a) the untouched ``evaluate`` on the model environment (200 steps) of this tree against a built checkout of the parent
    commit (``--parent DIR``; skipped without it), as child processes alternating A B B A -- the evaluating kernel's body
    is now one instance of a template.  ``ratio`` = parent median / this tree's median; ``parent_spread`` = the parent's
    own max / min across its repeats; ``ok``: the ratio lies inside [1 / parent_spread, parent_spread].
(b) ``collect_model(horizon=5, start=store, noise_std=0.3)`` against ``evaluate`` on the same model with
    ``episode_len=5``: what the noise, the seven tables, the discounted sums and the branch-start launch cost.  Reported.
(c) one round of the model-based loop -- ``collect_model(into=store)`` of 1024 x 5 rows plus ten CPQ ``steps_replay`` at
    batch 2048 -- against the same ten steps without the collection.  Reported.

Every number is ms per call; every repeat is kept.  Writes profiles/model_collect_bench.json (``--out``).  Needs an
MI355X: there is no CPU path."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(od=76, ad=2, hidden=[256, 256], members=5, model_hidden=[200, 200, 200], episodes=1024, episode_len=200,
             horizon=5, batch=2048, rows=20000)


def summary(v):
    s = sorted(v)
    return dict(min=round(s[0], 3), median=round(s[len(s) // 2], 3), max=round(s[-1], 3), n=len(s), all=[round(x, 3) for x in v])


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def make(episode_len):
    """(trainer, model environment, dataset): only what the parent commit has as well."""
    import numpy as np
    import torch
    from osrl_amd.algorithms import CPQ, CPQTrainer, Dynamics
    from osrl_amd.common.logger import DummyLogger
    from osrl_amd.common.model_env import ModelVecEnv
    from osrl_amd.common.replay import synthetic_transitions
    s = SHAPE
    d = synthetic_transitions(s["rows"], s["od"], s["ad"], seed=1)
    d["next_observations"] = (d["observations"] + 0.1 * d["next_observations"]).astype(np.float32)
    torch.manual_seed(0)
    dyn = Dynamics(s["od"], s["ad"], s["model_hidden"], num_models=s["members"], device="cuda:0")
    dyn.fit_normalizer(d)
    cpq = CPQ(s["od"], s["ad"], 1.0, s["hidden"], s["hidden"], 400, 10, episode_len=s["episode_len"], device="cuda:0")
    menv = ModelVecEnv(dyn, d["observations"][:s["episodes"]], s["episodes"], episode_len, reward_penalty=0.5)
    tr = CPQTrainer(cpq, menv, DummyLogger(), 1e-4, 1e-3, 1e-4, 1e-3, device="cuda:0", stats_mode="none")
    return tr, menv, d


def abba(a, b, reps):
    ta, tb = [], []
    for i in range(reps):
        for dst in ((ta, tb, tb, ta) if i % 2 == 0 else (tb, ta, ta, tb)):
            dst.append(timed(a if dst is ta else b))
    return ta, tb


def worker(tree, what, reps):
    """Runs in a child process with ``tree`` first on the path."""
    sys.path.insert(0, tree)
    s = SHAPE
    out = {}
    if what == "evaluate":
        tr, menv, _ = make(s["episode_len"])
        tr.evaluate(s["episodes"])
        out["evaluate_ms"] = [timed(lambda: tr.evaluate(s["episodes"])) for _ in range(reps)]
    else:
        from osrl_amd.common.replay import ReplayStore
        tr, menv, d = make(s["horizon"])
        n, rows = s["rows"], s["episodes"] * s["horizon"]
        store = ReplayStore(d, "cuda:0", seed=2, capacity=n + 8 * rows, pinned_rows=n)
        kw = dict(horizon=s["horizon"], start=store, noise_std=0.3)
        tr.evaluate(s["episodes"])
        tr.collect_model(menv, **kw)
        seeds = iter(range(1, 1 << 30))
        a, b = abba(lambda: tr.evaluate(s["episodes"]), lambda: tr.collect_model(menv, seed=next(seeds), **kw), reps)
        out["branch"] = dict(evaluate_len5_ms=a, collect_model_ms=b)
        eng = tr.model.engine(s["batch"])
        eng.attach_replay(store)
        eng.steps_replay(10)
        tr.collect_model(menv, into=store, **kw)

        def round_():
            tr.collect_model(menv, into=store, seed=next(seeds), **kw)
            eng.steps_replay(10)
        a, b = abba(lambda: eng.steps_replay(10), round_, reps)
        out["loop"] = dict(ten_steps_ms=a, round_ms=b, live_rows=int(store.n_rows))
    print("RESULT " + json.dumps(out))


def child(tree, what, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--tree", tree, "--reps", str(reps)]
    env = dict(os.environ)
    lib = os.path.join(tree, "osrl_amd", "lib", "libosrl_amd.so")
    if os.path.exists(lib):  # each tree measures the library it was built with, whatever the files' times say
        env["OSRL_LIB"] = lib
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tree, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"worker {what} failed in {tree}: {r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def against_parent(parent, reps, rounds):
    here, there = [], []
    for _ in range(rounds):  # A B B A
        for tree, dst in ((ROOT, here), (parent, there), (parent, there), (ROOT, here)):
            dst += child(tree, "evaluate", reps)["evaluate_ms"]
    h, t = summary(here), summary(there)
    spread, ratio = t["max"] / t["min"], t["median"] / h["median"]
    return dict(this_tree_ms=h, parent_ms=t, ratio=round(ratio, 4), parent_spread=round(spread, 4),
                ok=bool(1.0 / spread <= ratio <= spread))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_collect_bench.json"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part a)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="A B B A rounds of part (a): 2 child processes per tree each")
    ap.add_argument("--worker", default=None, choices=["evaluate", "collect"])
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.tree), args.worker, args.reps)
    out = dict(shape=SHAPE, evaluate_vs_parent=None)
    if args.parent:
        out["evaluate_vs_parent"] = against_parent(os.path.abspath(args.parent), args.reps, args.rounds)
    co = child(ROOT, "collect", args.reps)
    a, b = summary(co["branch"]["evaluate_len5_ms"]), summary(co["branch"]["collect_model_ms"])
    out["collect_model_vs_evaluate"] = dict(evaluate_len5_ms=a, collect_model_ms=b, ratio=round(b["median"] / a["median"], 4))
    a, b = summary(co["loop"]["ten_steps_ms"]), summary(co["loop"]["round_ms"])
    out["loop_round_vs_ten_steps"] = dict(ten_steps_ms=a, round_ms=b, ratio=round(b["median"] / a["median"], 4),
                                          live_rows=co["loop"]["live_rows"])
    import torch  # (after the children: this process never opens the device before them)
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
