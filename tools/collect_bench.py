"""What recording costs: env-steps/s of ``Collector.run`` (the rollout that writes the dataset) against
``BatchedRollout.run`` (``evaluate``'s rollout, which keeps three sums per episode) for a CPQ policy at C2's shape --
(obs, act) = (76, 2), hidden [256, 256] -- at 256 and 1024 episodes of 200 steps, in one process, interleaved
(A B B A per round):

* ``evaluate``        ``BatchedRollout.run()``;
* ``collect``         ``Collector.run(0.3)``: noise drawn in the kernel, seven tables written, copied out at the end;
* ``collect_sigma0``  ``Collector.run(0.0)``: the same without the Philox draw.

Every number is env-steps/s = episodes * episode_len / wall time of one ``run`` (its one host sync included), after
``--warmup`` runs (captures, code objects, allocator).  Writes profiles/collect_bench.json (``--out``).  Needs an MI355X:
there is no CPU path."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

OD, AD, HID, EL = 76, 2, [256, 256], 200


def summary(v):
    v = sorted(v)
    return dict(min=round(v[0]), median=round(v[len(v) // 2]), max=round(v[-1]), n=len(v))


def rate(run, env_steps, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    return reps * env_steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--reps", type=int, default=5, help="runs per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collect_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("collect_bench needs an MI355X (no CPU path): not measured")
    from osrl_amd.algorithms import CPQ
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv, VecSyntheticSafeEnv
    from osrl_amd.engine.collect import Collector
    from osrl_amd.engine.rollout import BatchedRollout
    dev = "cuda:0"
    torch.manual_seed(0)
    m = CPQ(OD, AD, 1.0, HID, HID, 400, 10, episode_len=EL, device=dev)
    out = dict(shape=dict(obs=OD, act=AD, hidden=HID, episode_len=EL, policy="cpq"), device=torch.cuda.get_device_name(0),
               reps=args.reps, warmup=args.warmup, rounds=args.rounds, order="evaluate collect collect_sigma0, then reversed, per round",
               env_steps_per_s={})
    for E in args.episodes:
        venv = VecSyntheticSafeEnv(SyntheticSafeEnv(OD, AD, EL, seed=1, init_noise=0.5), E, dev)
        ro, co = BatchedRollout(m, venv, "cpq"), Collector(m, venv, "cpq")
        arms = dict(evaluate=ro.run, collect=lambda: co.run(0.3), collect_sigma0=lambda: co.run(0.0))
        for f in arms.values():
            for _ in range(args.warmup):
                f()
        res = {k: [] for k in arms}
        order = list(arms) + list(arms)[::-1]
        for _ in range(args.rounds):
            for name in order:
                res[name].append(rate(arms[name], E * EL, args.reps))
        s = {k: summary(v) for k, v in res.items()}
        s["collect_over_evaluate"] = round(s["collect"]["median"] / s["evaluate"]["median"], 3)
        s["guards_intact"] = co.guards_intact()
        out["env_steps_per_s"][str(E)] = s
        print(E, json.dumps(s))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
