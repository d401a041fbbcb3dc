"""Weighted transition sampling (ReplayStore.set_sample_prob) against the uniform draw, one session, interleaved ABBA:

* the step prologue (tick + noise + 6-table gather, osrl_step_begin_w) at B = 2048 over 2^18 and 2^22 rows: a captured
  chain of K prologue launches replayed, time per launch (launch-to-launch inside a graph: kernel time plus the graph's
  per-node gap, the same gap for both arms);
* BC's one-launch step at B = 256 (direct launches) and the C2 step through the pipelined graphs (bench.Workload), steps/s;
* the table build (osrl_weights_cum_u64) at both sizes.

``--trace``: only the prologue launches, for a ``rocprofv3 --kernel-trace --stats`` run of its own (kernel durations).
Writes profiles/replay_weighted.json (``--out``)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from osrl_amd.common.replay import ReplayStore, synthetic_transitions  # noqa: E402
from osrl_amd.engine.core import StepState, graph_capture  # noqa: E402

DEV = torch.device("cuda", 0)


def weights(n, seed=0):
    """DSRL-like: ~10 % of the rows carry cost and are drawn ten times as often."""
    rs = np.random.RandomState(seed)
    return np.where(rs.uniform(size=n) < 0.1, 10.0, 1.0)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps  # seconds per call


def abba(run_a, run_b, rounds=3):
    """A B B A per round; returns the two lists of measurements."""
    a, b = [], []
    for _ in range(rounds):
        a.append(run_a())
        b.append(run_b())
        b.append(run_b())
        a.append(run_a())
    return a, b


def summary(v, scale=1.0):
    v = sorted(x * scale for x in v)
    return dict(min=round(v[0], 3), median=round(v[len(v) // 2], 3), max=round(v[-1], 3), n=len(v))


def prologue(n_rows, B=2048, od=76, ad=2, K=100, trace=False):
    mk = lambda w: ReplayStore(synthetic_transitions(n_rows, od, ad), DEV, sample_prob=w)  # noqa: E731
    stores = dict(uniform=mk(None), weighted=mk(weights(n_rows)))
    dst = [torch.zeros(B, w, device=DEV) for w in (od, od, ad, 1, 1, 1)]
    noise = torch.zeros(B * 30, device=DEV)
    st = StepState(DEV, ["a", "b", "c", "d", "e"])
    graphs = {}
    for name, s in stores.items():
        ga = s.gather_args(dst)
        for _ in range(3):
            st.begin(noise, 1, 0, ga)
        torch.cuda.synchronize()
        if trace:
            for _ in range(K):
                st.begin(noise, 1, 0, ga)
            torch.cuda.synchronize()
            continue
        g = torch.cuda.CUDAGraph()
        with graph_capture(g):
            for _ in range(K):
                st.begin(noise, 1, 0, ga)
        g.replay()
        graphs[name] = g
    if trace:
        return None
    u, w = abba(lambda: timed(graphs["uniform"].replay, 20) / K, lambda: timed(graphs["weighted"].replay, 20) / K)
    t0 = time.perf_counter()
    build = timed(lambda: stores["weighted"].set_sample_prob(weights(n_rows, 1)), 3)
    return dict(n_rows=n_rows, B=B, launches_per_graph=K, uniform_us=summary(u, 1e6), weighted_us=summary(w, 1e6),
                set_sample_prob_ms=round(build * 1e3, 3), set_sample_prob_wall_ms=round((time.perf_counter() - t0) / 3 * 1e3, 3))


def workload(name, steps, pipe):
    import bench
    wl = bench.Workload(name, DEV, 0, 1, None, n_store=1 << 18)
    if pipe:
        wl.build_pipe(0)
    w = weights(wl.store.n_rows)

    def arm(weighted):
        wl.store.set_sample_prob(w if weighted else None)
        wl.run(steps // 4 + 40)  # (a switch of mode captures again: outside the timed region)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wl.run(steps)
        torch.cuda.synchronize()
        return steps / (time.perf_counter() - t0)

    u, ww = abba(lambda: arm(False), lambda: arm(True), rounds=2)
    return dict(config=name, steps=steps, uniform_steps_per_s=summary(u), weighted_steps_per_s=summary(ww))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_weighted.json"))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--steps", type=int, default=2000)
    args = ap.parse_args()
    if args.trace:
        for n in (1 << 18, 1 << 22):
            prologue(n, trace=True)
        return
    out = dict(device=torch.cuda.get_device_name(0),
               prologue=[prologue(1 << 18), prologue(1 << 22)],
               bc_one_launch_B256=workload("c1", args.steps * 4, False),
               c2_steps_replay=workload("c2", args.steps, True))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
