"""SequenceStore(evict="oldest") measured in one session, interleaved repeats (A B B A), medians:

(a) the NON-evicting ``SequenceStore.append`` of one chunk, whose code the eviction touches, in this tree and in a built
    checkout of the parent commit (``--parent DIR``; skipped without it): one child process per repeat, each building a
    capacity store at C5's data shape (1024 episodes x 200 rows, obs 11, act 3, ``cost_sample``) and timing ``append`` of
    chunks of that size.  This tree's median is to lie inside the spread of the parent's own repeats (``ok``);
(b) one round of the online CDT loop on a FULL evicting store at that shape -- ``append`` of 1024 x 200 rows (which evicts
    the 1024 oldest episodes) + ``--steps`` ``step_store`` calls on the graph the engine has -- against what a store
    without eviction forces: ``SequenceStore.from_dataset`` over survivors + chunk, ``attach_store`` and the recapture,
    then the same steps.  Reported, not gated.

Writes profiles/seq_ring_bench.json (``--out``)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPISODES, EPISODE_LEN, OD, AD, T = 1024, 200, 11, 3, 20


def summary(v):
    v = sorted(v)
    return dict(min=round(v[0], 3), median=round(v[len(v) // 2], 3), max=round(v[-1], 3), n=len(v), all=[round(x, 3) for x in v])


def chunk(seed, device):
    """One chunk of complete episodes as device tensors under the DSRL keys."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = EPISODES * EPISODE_LEN
    d = dict(observations=torch.randn(n, OD, generator=g), next_observations=torch.randn(n, OD, generator=g),
             actions=torch.rand(n, AD, generator=g) * 2 - 1, rewards=torch.rand(n, generator=g),
             costs=(torch.rand(n, generator=g) < 0.1).float(), terminals=torch.zeros(n), timeouts=torch.zeros(n))
    d["timeouts"][EPISODE_LEN - 1::EPISODE_LEN] = 1
    return {k: v.to(device) for k, v in d.items()}


def child_append(tree, chunks):
    """Runs in a child process: ``osrl_amd`` of ``tree``; ms per non-evicting append of one chunk (median of ``chunks``)."""
    sys.path.insert(0, tree)
    import torch
    from osrl_amd.common.replay import SequenceStore
    dev = torch.device("cuda", 0)
    n = EPISODES * EPISODE_LEN
    store = SequenceStore.from_dataset(chunk(0, dev), T, dev, reward_scale=0.1, cost_sample=True, seed=1,
                                       capacity_rows=(chunks + 2) * n, capacity_traj=(chunks + 2) * EPISODES)
    new = [chunk(i, dev) for i in range(1, chunks + 2)]
    store.append(new[0])  # (warm: the first call loads the kernels)
    torch.cuda.synchronize()
    ms = []
    for d in new[1:]:
        t0 = time.perf_counter()
        store.append(d)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    assert store.n_traj == (chunks + 2) * EPISODES
    print(json.dumps(dict(append_ms=sorted(ms)[len(ms) // 2])))


def append_ms(tree, chunks):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--chunks", str(chunks)],
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(f"the append child failed in {tree}: {out.stderr[-2000:]}")
    return float(json.loads(out.stdout.strip().splitlines()[-1])["append_ms"])


def against_parent(parent, chunks, rounds):
    here, there = [], []
    for _ in range(rounds):  # A B B A
        here.append(append_ms(ROOT, chunks))
        there.append(append_ms(parent, chunks))
        there.append(append_ms(parent, chunks))
        here.append(append_ms(ROOT, chunks))
    h, t = summary(here), summary(there)
    return dict(rows_per_chunk=EPISODES * EPISODE_LEN, trajectories_per_chunk=EPISODES, this_change_ms=h, parent_ms=t,
                ratio=round(h["median"] / t["median"], 4), parent_spread=round(t["max"] / t["min"], 4),
                ok=t["min"] <= h["median"] <= t["max"] or h["median"] <= t["min"])


def loop_round(rounds, steps):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from osrl_amd.common.replay import SequenceStore
    dev = torch.device("cuda", 0)
    n = EPISODES * EPISODE_LEN
    kw = dict(reward_scale=0.1, cost_sample=True, seed=1)
    a, b = bench.Workload("c5", dev, 0, 1, None), bench.Workload("c5", dev, 0, 1, None)
    ring = SequenceStore.from_dataset(chunk(0, dev), T, dev, capacity_rows=n, capacity_traj=EPISODES, evict="oldest", **kw)
    a.eng.attach_store(ring)
    b.eng.attach_store(SequenceStore.from_dataset(chunk(0, dev), T, dev, **kw))
    new = [chunk(i, dev) for i in range(1, 5)]
    for wl in (a, b):
        for _ in range(steps):
            wl.eng.step_store()
    torch.cuda.synchronize()

    def evicting(d):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ring.append(d)  # full: the 1024 oldest episodes go
        for _ in range(steps):
            a.eng.step_store()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def rebuild(d):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.eng.attach_store(SequenceStore.from_dataset(d, T, dev, **kw))  # (no survivors at this size: the chunk alone)
        for _ in range(steps):
            b.eng.step_store()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ta, tb = [], []
    for i in range(rounds):
        ta.append(evicting(new[0]))
        tb.append(rebuild(new[1]))
        tb.append(rebuild(new[2]))
        ta.append(evicting(new[3]))
    assert ring.n_traj == EPISODES and ring.n_evicted == 2 * rounds * EPISODES
    sa, sb = summary(ta), summary(tb)
    return dict(config="c5", rows_in_store=n, rows_per_round=n, steps_per_round=steps, evicting_ms_per_round=sa,
                rebuild_ms_per_round=sb, removed_ms_per_round=round(sb["median"] - sa["median"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_ring_bench.json"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part a)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--chunks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    if args.child:
        child_append(args.child, args.chunks)
        return
    out = dict(device=None, append_vs_parent=None)
    if args.parent:  # (child processes, before this one opens the device)
        out["append_vs_parent"] = against_parent(os.path.abspath(args.parent), args.chunks, args.rounds)
    out["loop_round"] = loop_round(args.rounds, args.steps)
    import torch
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
