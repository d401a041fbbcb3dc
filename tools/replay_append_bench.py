"""Stores that grow (ReplayStore(capacity=) / append, collect(into=)) measured in one session, interleaved repeats:

(a) the fixed-store path against the parent commit: ``bench.py --config c1`` and ``--config c2`` in this tree and in a
    built checkout of the parent (``--parent DIR``; skipped without it), alternating.  The sampler's NULL path must cost
    nothing: this tree's median must not lie below the lowest of the parent's own repeats (``ok``).
(b) a growing store against a fixed store: C2's shape through the pipelined graphs, the same rows in a fixed store and
    in a capacity store of twice the size, steps/s (the extra cost is one load ahead of the index);
(c) one round of the online loop at C2's shape: ``collect(into=store)`` + 100 steps against collect + ``merge_datasets`` +
    a new store + ``attach_replay`` + 100 steps -- the difference is the recapture (and re-upload) the feature removes.

Writes profiles/replay_append_ab.json (``--out``)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

DEV = torch.device("cuda", 0)


def summary(v):
    v = sorted(v)
    return dict(min=round(v[0], 3), median=round(v[len(v) // 2], 3), max=round(v[-1], 3), n=len(v), all=[round(x, 3) for x in v])


def bench_value(tree, config, steps, warmup):
    """One ``bench.py`` run in ``tree`` as a child process: the value of its last JSON result line."""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--config", config,
           "--no-cpu-baseline", "--no-roofline", "--no-extras"]
    out = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(f"bench.py failed in {tree}: {out.stderr[-2000:]}")
    vals = []
    for ln in out.stdout.splitlines():
        try:
            r = json.loads(ln)
        except ValueError:
            continue
        if isinstance(r, dict) and "value" in r:
            vals.append(float(r["value"]))
    return vals[-1]


def against_parent(parent, config, steps, warmup, rounds):
    here, there = [], []
    for _ in range(rounds):  # A B B A
        here.append(bench_value(ROOT, config, steps, warmup))
        there.append(bench_value(parent, config, steps, warmup))
        there.append(bench_value(parent, config, steps, warmup))
        here.append(bench_value(ROOT, config, steps, warmup))
    h, t = summary(here), summary(there)
    return dict(config=config, steps=steps, this_change_steps_per_s=h, parent_steps_per_s=t, ok=h["median"] >= t["min"])


def timed_steps(wl, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wl.run(steps)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def grown_against_fixed(steps, rounds, n_store=1 << 18):
    import bench
    from osrl_amd.common.replay import ReplayStore, synthetic_transitions
    cfg = bench.CONFIGS["c2"]
    fixed = bench.Workload("c2", DEV, 0, 1, None, n_store=n_store)
    grown = bench.Workload("c2", DEV, 0, 1, None, n_store=n_store)
    grown.store = ReplayStore(synthetic_transitions(n_store, cfg["od"], cfg["ad"], seed=1), DEV, reward_scale=0.1,
                              cost_scale=1.0, seed=1, capacity=2 * n_store)
    grown.eng.attach_replay(grown.store)
    for wl in (fixed, grown):
        wl.build_pipe(0)
        wl.run(200)
    f, g = [], []
    for _ in range(rounds):
        f.append(timed_steps(fixed, steps))
        g.append(timed_steps(grown, steps))
        g.append(timed_steps(grown, steps))
        f.append(timed_steps(fixed, steps))
    return dict(config="c2", rows=n_store, capacity=2 * n_store, steps=steps, fixed_steps_per_s=summary(f),
                capacity_steps_per_s=summary(g))


def loop_round(rounds, episodes=64, episode_len=100, steps=100, n0=1 << 16):
    """Per arm: a CPQ trainer at C2's shape on a VecSyntheticSafeEnv; one round = collect E * L rows + ``steps`` steps."""
    import bench
    from osrl_amd.algorithms import CPQ, CPQTrainer
    from osrl_amd.common.replay import ReplayStore, synthetic_transitions
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv, VecSyntheticSafeEnv
    from osrl_amd.engine.collect import merge_datasets
    cfg = bench.CONFIGS["c2"]
    od, ad, B = cfg["od"], cfg["ad"], cfg["B"]
    keys = ("observations", "next_observations", "actions", "rewards", "costs", "terminals", "timeouts")

    def arm():
        torch.manual_seed(0)
        m = CPQ(od, ad, 1.0, bench.HID, bench.HID, bench.VAE_H, bench.NS, 0.99, 0.005, 0.5, 2, 2, 1.5, 10, episode_len,
                device=str(DEV))
        tr = CPQTrainer(m, None, None, actor_lr=1e-4, critic_lr=1e-3, alpha_lr=1e-4, vae_lr=1e-3, reward_scale=0.1,
                        cost_scale=1.0, device=str(DEV), stats_mode="none")
        tr.env = VecSyntheticSafeEnv(SyntheticSafeEnv(od, ad, episode_len, seed=3, init_noise=0.5), episodes, DEV, base_seed=100)
        data = {k: torch.as_tensor(v, device=DEV) for k, v in synthetic_transitions(n0, od, ad, seed=1).items()}
        return m, tr, m.engine(B), {k: data[k] for k in keys}

    ma, ta, ea, da = arm()
    store = ReplayStore(da, DEV, reward_scale=0.1, cost_scale=1.0, seed=1, capacity=n0 + (4 * rounds + 4) * episodes * episode_len)
    ea.attach_replay(store)
    mb, tb, eb, db = arm()
    eb.attach_replay(ReplayStore(db, DEV, reward_scale=0.1, cost_scale=1.0, seed=1))
    state = dict(data=db)
    for e, t in ((ea, ta), (eb, tb)):  # capture everything once, the collector's graph included
        e.steps_replay(steps)
        t.collect(0.3, seed=0)
    torch.cuda.synchronize()

    def into(i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ta.collect(0.3, seed=i, into=store)
        ea.steps_replay(steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def rebuild(i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = tb.collect(0.3, seed=i)
        state["data"] = merge_datasets([state["data"], c.dataset])
        eb.attach_replay(ReplayStore(state["data"], DEV, reward_scale=0.1, cost_scale=1.0, seed=1))
        eb.steps_replay(steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    a, b, i = [], [], 1
    for _ in range(rounds):
        a.append(into(i))
        b.append(rebuild(i + 1))
        b.append(rebuild(i + 2))
        a.append(into(i + 3))
        i += 4
    sa, sb = summary(a), summary(b)
    return dict(config="c2", rows_at_start=n0, rows_per_round=episodes * episode_len, steps_per_round=steps,
                into_ms_per_round=sa, rebuild_ms_per_round=sb, removed_ms_per_round=round(sb["median"] - sa["median"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_append_ab.json"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part a)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--bench-steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    out = dict(device=None, fixed_store_vs_parent=None)
    if args.parent:  # (child processes, before this one opens the device)
        out["fixed_store_vs_parent"] = [against_parent(os.path.abspath(args.parent), c, args.bench_steps * (4 if c == "c1" else 1),
                                                       20, args.rounds) for c in ("c1", "c2")]
    out["device"] = torch.cuda.get_device_name(0)
    out["capacity_vs_fixed_store"] = grown_against_fixed(args.steps, args.rounds)
    out["loop_round"] = loop_round(args.rounds)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
