"""What bootstrap weights, the holdout loss and elite members cost (csrc/dyn_loss.hip, engine/dynamics.py
``BootDynamicsEngine``, ``DynamicsTrainer.validate``, the elites in ``ModelVecEnv``), measured in one session on one device at
(76, 2), 5 x [200, 200, 200], fit batch 256, 1024 episodes (tools/model_env_bench.py's shape and setup).  Every run is a
child process under its own ``timeout``; the runs alternate A B B A; medians.  Writes profiles/dyn_ensemble_bench.json
(``--out``).

(a) gated, against a built checkout of the parent commit (``--parent DIR``; skipped without it): the untouched paths -- the
    default fit step (``step_replay`` at batch 256) of the deterministic and of the Gaussian model, and ``evaluate`` on a
    ``ModelVecEnv`` of a model without elites.  ``ratio`` = parent median / this tree's median (below 1: this tree is
    slower); ``parent_spread`` = max / min of the parent's own repeats; ``ok``: the ratio is not below 1 / parent_spread.
(b) gated, the same rule: ``bench.py --gpus 1 --steps 20 --warmup 5`` (its timed region) of both trees, grad-steps/s.
(c) reported, not gated: the bootstrap fit step against the default one (two more launches and a dY round trip),
    ``validate`` on the 51 200 collected rows, and ``evaluate`` with 5 elites of 7 members against all 7 and against a
    5-member model.

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
FIT_STEPS = 200      # step_replay calls per timed sample


def _step_ms(eng):
    return MB.timed(lambda: [eng.step_replay() for _ in range(FIT_STEPS)])[0] / FIT_STEPS


def worker(tree, what, reps):
    """Runs in a child process with ``tree`` first on the path: ms per call (per train step), every repeat."""
    sys.path.insert(0, tree)
    import torch
    dev = torch.device("cuda", 0)
    s = MB.GAUSS_SHAPE
    E = s["episodes"]
    one = lambda f: MB.timed(f)[0]  # noqa: E731
    out = {}
    if what == "untouched":  # only what the parent commit has too
        tr, _, dyn, _, _ = MB._setup(dev, 50)
        tr.evaluate(E)
        out["evaluate_ms"] = [one(lambda: tr.evaluate(E)) for _ in range(reps)]
        out["fit_step_ms"] = [_step_ms(dyn._engine) for _ in range(reps)]
        dyn_g = MB._setup(dev, 50, probabilistic=True)[2]
        out["gauss_fit_step_ms"] = [_step_ms(dyn_g._engine) for _ in range(reps)]
    else:
        from osrl_amd.algorithms import CPQTrainer, Dynamics, DynamicsTrainer
        from osrl_amd.common.model_env import ModelVecEnv
        from osrl_amd.common.replay import ReplayStore
        tr, menv, dyn, _, data = MB._setup(dev, 50)
        for name, kw in (("fit_step_ms", {}), ("gauss_fit_step_ms", dict(probabilistic=True))):
            sides = dict(default=dyn if not kw else MB.fit_model(s["od"], s["ad"], data, 50, dev, **kw)[0],
                         bootstrap=MB.fit_model(s["od"], s["ad"], data, 50, dev, bootstrap=True, boot_seed=1, **kw)[0])
            assert type(sides["bootstrap"]._engine).__name__ == "BootDynamicsEngine"
            ms = {k: [] for k in sides}
            for _ in range(reps):
                for k in list(sides) + list(sides)[::-1]:
                    ms[k].append(_step_ms(sides[k]._engine))
            out[name] = ms
        # the holdout loss on every collected row
        vt = DynamicsTrainer(dyn, lr=1e-3, stats_mode="none")
        store = ReplayStore(data, dev, seed=0)
        rows = int(store.n_rows)
        vt.validate(store)
        out["validate_ms"] = [one(lambda: vt.validate(store)) for _ in range(reps)]
        out["validate_rows"] = rows
        # 5 elites of 7 against all 7 members and against a 5-member model (the untouched evaluate)
        sides = {"5_members": tr}
        for name, kw in (("7_members", dict(num_models=7)), ("5_elites_of_7", dict(num_models=7, num_elites=5))):
            torch.manual_seed(0)
            d7 = Dynamics(s["od"], s["ad"], list(s["model_hidden"]), device=str(dev), **kw)
            d7.fit_normalizer(store)
            if d7.num_elites:
                d7.set_elites([0, 2, 3, 5, 6])
            sides[name] = CPQTrainer(tr.model, env=ModelVecEnv(d7, menv.state0, E, MB.EL), stats_mode="none")
        ms = {k: [] for k in sides}
        for t in sides.values():
            t.evaluate(E)
        for _ in range(reps):
            for k in list(sides) + list(sides)[::-1]:
                ms[k].append(one(lambda: sides[k].evaluate(E)))
        out["evaluate_ms"] = ms
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dyn_ensemble_bench.json"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (parts a and b)")
    ap.add_argument("--rounds", type=int, default=2, help="A B B A rounds of parts (a) and (b)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--worker", default=None, choices=["untouched", "ensemble"])
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.tree), args.worker, args.reps)
    out = dict(shape=dict(MB.GAUSS_SHAPE, fit_steps_per_sample=FIT_STEPS), reported_not_gated=None,
               untouched_vs_parent=None, bench_vs_parent=None)
    g = child(ROOT, "ensemble", args.reps)
    rep = dict(validate=dict(rows=g["validate_rows"], ms=MB.summary(g["validate_ms"])))
    for key, base in (("fit_step_ms", "default"), ("gauss_fit_step_ms", "default"), ("evaluate_ms", "5_members")):
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
