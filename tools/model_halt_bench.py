"""What halting on uncertainty costs (csrc/model_env.hip flag kPess, csrc/compact.hip), measured in one session on one
device at (76, 2), 5 x [200, 200, 200], 1024 episodes (tools/model_env_bench.py's shape and setup).  Every run is a child
process under its own ``timeout``; the runs alternate A B B A; medians.  Writes profiles/model_halt_bench.json (``--out``).

(a) gated, against a built checkout of the parent commit (``--parent DIR``; skipped without it): the untouched paths --
    the deterministic model's ``evaluate`` and ``collect_model(horizon=5)`` and the Gaussian model's ``evaluate``.
    ``ratio`` = parent median / this tree's median (below 1: this tree is slower); ``parent_spread`` = max / min of the
    parent's own repeats; ``ok``: the ratio is not below 1 / parent_spread.
(b) gated, the same rule: ``bench.py --gpus 1 --steps 20 --warmup 5`` (its timed region) of both trees, grad-steps/s.
(c) reported, not gated: ``evaluate`` through the ``_halt`` step with the threshold at +inf against the plain step.
(d) reported, not gated: a halting ``collect_model(horizon=5)`` -- compaction and its host sync included -- against the
    plain run followed by a torch boolean-mask selection of the same rows from the eight tables.  The threshold is the
    median of the per-row u of a plain run, so that about half the rows are past a halt.

The first failing child ends the run: nothing more is started on the device after it."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_env_bench as MB  # noqa: E402  (the shape, the setup, summary / gate / timed)

CHILD_TIMEOUT = 420  # seconds, per child process


def worker(tree, what, reps):
    """Runs in a child process with ``tree`` first on the path: ms per call, every repeat."""
    sys.path.insert(0, tree)
    import torch
    dev = torch.device("cuda", 0)
    E, H = MB.GAUSS_SHAPE["episodes"], MB.GAUSS_SHAPE["horizon"]
    one = lambda f: MB.timed(f)[0]  # noqa: E731
    out = {}
    if what == "untouched":  # only what the parent commit has too
        tr, menv, _, _, _ = MB._setup(dev, 50)
        tr.evaluate(E)
        tr.collect_model(menv, horizon=H, noise_std=0.3, seed=0)
        out["evaluate_ms"] = [one(lambda: tr.evaluate(E)) for _ in range(reps)]
        out["collect_model_ms"] = [one(lambda: tr.collect_model(menv, horizon=H, noise_std=0.3, seed=1)) for _ in range(reps)]
        trg = MB._setup(dev, 50, probabilistic=True)[0]
        trg.evaluate(E)
        out["gauss_evaluate_ms"] = [one(lambda: trg.evaluate(E)) for _ in range(reps)]
    else:
        from osrl_amd.algorithms import CPQTrainer
        from osrl_amd.common.model_env import ModelVecEnv
        from osrl_amd.engine.collect import KEYS
        plain = MB._setup(dev, 50)
        # the same policy, model and initial states behind the _halt entry points
        mh = ModelVecEnv(plain[2], plain[1].state0, E, MB.EL, halt_threshold=float("inf"))
        halt = (CPQTrainer(plain[0].model, env=mh, stats_mode="none"), mh)
        sides = dict(plain_step=plain, halt_step_threshold_inf=halt)
        ms = {k: [] for k in sides}
        for a in sides.values():
            a[0].evaluate(E)
        for _ in range(reps):
            for k in list(sides) + list(sides)[::-1]:
                ms[k].append(one(lambda: sides[k][0].evaluate(E)))
        out["evaluate_ms"] = ms
        assert torch.equal(plain[1].acc, halt[1].acc)  # (the same bits: tests/test_gpu_model_halt.py)
        # (d) the threshold from a plain run's per-row u; then halting + compaction against plain + boolean mask
        tr, menv = plain[0], plain[1]
        tr.collect_model(menv, horizon=H, noise_std=0.3, seed=1)
        thr = float(tr.model_collector(menv).row_disagreement.median().item())
        trh = halt[0]
        mh.halt_threshold = thr
        res = trh.collect_model(mh, horizon=H, noise_std=0.3, seed=1)
        rows = int(res.lengths.sum())

        def masked():
            r = tr.collect_model(menv, horizon=H, noise_std=0.3, seed=1)
            col = tr.model_collector(menv)
            u = col.row_disagreement.view(E, H)
            live = ((u > thr).cumsum(1) - (u > thr).int() == 0).reshape(-1)  # rows up to and including the first u > thr
            d = {k: r.dataset[k][live] for k in KEYS}
            return d, col.row_disagreement[live]

        d, _ = masked()
        assert d["rewards"].shape[0] == rows, (d["rewards"].shape, rows)
        sides = dict(plain_then_mask=masked, halting_with_compaction=lambda: trh.collect_model(mh, horizon=H, noise_std=0.3, seed=1))
        ms = {k: [] for k in sides}
        for _ in range(reps):
            for k in list(sides) + list(sides)[::-1]:
                ms[k].append(one(sides[k]))
        out["collect_model_ms"] = ms
        out["collect_rows"] = dict(kept=rows, of=E * H, threshold=thr)
    print("RESULT " + json.dumps(out))


def child(tree, what, reps):
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--worker", what,
           "--tree", tree, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tree)
    if r.returncode != 0:
        raise RuntimeError(f"worker {what} ended with {r.returncode} in {tree}: {r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def bench_child(tree):
    r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable] + MB.BENCH_CMD, capture_output=True,
                       text=True, cwd=tree)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py ended with {r.returncode} in {tree}: {r.stderr[-2000:]}")
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{") and '"value"' in ln]
    return float(rows[-1]["value"])


def write(out, path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_halt_bench.json"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (parts a and b)")
    ap.add_argument("--rounds", type=int, default=2, help="A B B A rounds of parts (a) and (b)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--worker", default=None, choices=["untouched", "halt"])
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.tree), args.worker, args.reps)
    out = dict(shape=MB.GAUSS_SHAPE, reported_not_gated=None, untouched_vs_parent=None, bench_vs_parent=None)
    g = child(ROOT, "halt", args.reps)
    rep = dict(collect_rows=g["collect_rows"])
    for key, base in (("evaluate_ms", "plain_step"), ("collect_model_ms", "plain_then_mask")):
        sides = {k: MB.summary(v) for k, v in g[key].items()}
        rep[key] = dict(sides, ratio_to_first={k: round(v["median"] / sides[base]["median"], 4) for k, v in sides.items()
                                               if k != base})
    out["reported_not_gated"] = rep
    write(out, args.out)  # (kept even if a later child fails)
    print("reported part done", file=sys.stderr, flush=True)
    if args.parent:
        parent = os.path.abspath(args.parent)
        here, there, bh, bt = {}, {}, [], []
        for _ in range(args.rounds):  # A B B A
            for tree, dst, bd in ((ROOT, here, bh), (parent, there, bt), (parent, there, bt), (ROOT, here, bh)):
                for k, v in child(tree, "untouched", args.reps).items():
                    dst.setdefault(k, []).extend(v)
                bd.append(bench_child(tree))
                print(f"{'this tree' if tree == ROOT else 'parent'}: bench {bd[-1]}", file=sys.stderr, flush=True)
        out["untouched_vs_parent"] = {k: MB.gate(here[k], there[k]) for k in here}
        out["bench_vs_parent"] = dict(command="python " + " ".join(MB.BENCH_CMD), unit="grad-steps/s",
                                      **MB.gate(bh, bt, higher_is_better=True))
    import torch  # (after the children: this process never opens the device before them)
    out["device"] = torch.cuda.get_device_name(0)
    write(out, args.out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
