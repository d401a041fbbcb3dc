#!/usr/bin/env python3
"""Step-time A/B of the OOD-tail changes (select rounds, short row-set tiles, plan.vae_dw_side), four sides alternating
inside one lease:

    parent          OSRL_LIB = the parent commit's library, plan.vae_dw_side off
    lib             this tree's library, plan.vae_dw_side off
    plan            the parent's library, plan.vae_dw_side on
    both            this tree's library, plan.vae_dw_side on

    python tools/ood_tail_ab.py --parent-lib PATH [--config c2] [--steps 300] [--rounds 5] [--out profiles/x.json]

Every run is ``bench.py --gpus 1 --warmup 5`` in a process of its own; ``--dump`` adds one 20-step run a side with
``--dump-outputs`` and compares the arrays byte for byte against the parent side's.  Appends to --out (a JSON list)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(side, parent_lib, config, steps, dump=None, timeout=240):
    env = dict(os.environ, OSRL_LAB="1", OSRL_VAE_DW_SIDE="1" if side in ("plan", "both") else "0")
    if side in ("parent", "plan"):
        env["OSRL_LIB"] = parent_lib
    else:
        env.pop("OSRL_LIB", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "5", "--config", config,
           "--no-cpu-baseline", "--no-roofline", "--no-extras"] + (["--dump-outputs", dump] if dump else [])
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit(f"bench.py failed on side {side} (exit {p.returncode}): stopping")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)["value"]


def digest(d):
    out = {}
    for f in sorted(os.listdir(d)):
        out[f] = hashlib.sha256(open(os.path.join(d, f), "rb").read()).hexdigest()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--config", default="c2")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sides", default="parent,lib,plan,both")
    ap.add_argument("--dump", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ood_tail_bench_ab.json"))
    a = ap.parse_args()
    sides = a.sides.split(",")
    rec = {"config": a.config, "steps": a.steps, "warmup": 5, "sides": {s: [] for s in sides}}
    for r in range(a.rounds):
        for s in sides:
            rec["sides"][s].append(run(s, a.parent_lib, a.config, a.steps))
            print(a.config, a.steps, r, s, rec["sides"][s][-1], flush=True)
    rec["summary"] = {s: {"min": min(v), "median": statistics.median(v), "max": max(v)} for s, v in rec["sides"].items() if v}
    if a.dump:
        with tempfile.TemporaryDirectory() as tmp:
            digs = {}
            for s in sides:
                d = os.path.join(tmp, s)
                run(s, a.parent_lib, a.config, 20, dump=d)
                digs[s] = digest(d)
            ref = digs[sides[0]]
            rec["outputs_compare"] = {s: {"arrays": len(digs[s]), "byte_equal_to_" + sides[0]: digs[s] == ref,
                                          "differing": sorted(k for k in ref if digs[s].get(k) != ref[k])} for s in sides}
            print("outputs_compare", json.dumps(rec["outputs_compare"]), flush=True)
    prev = json.load(open(a.out)) if os.path.exists(a.out) else []
    prev.append(rec)
    json.dump(prev, open(a.out, "w"), indent=1)
    print(json.dumps(rec["summary"]))


if __name__ == "__main__":
    main()
