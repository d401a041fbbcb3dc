"""Digests of the training state after the same train steps, along every path a step engine offers.

For each case (tests/cases.py) a fresh model is stepped along

  graph       6 steps through ``step_replay`` (the captured hipGraph; CDT: ``step(..., use_graph=True)``)
  eager       6 eager steps with injected noise (BC / CDT: ``use_graph=False``)
  pipelined   CPQ, BCQ-Lag: 8 steps through ``steps_replay(8, steps_per_graph=4)``
  sequential  CPQ: the captured step with ``parallel_branches=False``
  graph_plan  BC: the captured six-launch plan (``direct=False``; "graph" takes the directly launched one-launch step)

and, for the dynamics fit (the shape and data of tests/dyn_ensemble_cases.py TRAIN, raw log-variances on both sides of both
bounds), 6 ``step_replay`` calls on a store along graph and eager; a SHA-256 is written per group buffer (p / m / v / tgt), per scalar-state tensor and of ``read_stats_many`` over all
steps.  Everything is seeded (the cases' numpy streams, store seeds 7 / 3, engine seed 0), so two trees that issue the
same launches give the same file: run it on both and diff.  The two CDT cases are the exception: the CDT step's
timestep-embedding scatter accumulates with fp32 atomics, so their digests differ between two runs of ONE tree -- run the
older tree twice to see which cases those are, and judge them by the tolerance tests (tests/test_gpu_cdt.py).  The tool
only uses what the engines offered before the shared engine base too, so it runs on a checkout from before that change.

    python tools/engine_ab.py --out a.json [--case cpq_wide --case bcql_wide]
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ["bc_small", "cpq_small", "bcql_pid", "bearl_lap", "coptidice_kl", "cdt_small", "cdt_det",
         "cpq_wide", "bcql_wide", "bearl_wide", "coptidice_wide", "dyn_mse", "dyn_gauss", "dyn_boot_elites"]
DYN_CASES = {"dyn_mse": dict(), "dyn_gauss": dict(probabilistic=True),
             "dyn_boot_elites": dict(probabilistic=True, bootstrap=True, num_elites=2)}
DEV = "cuda:0"
STEPS, PIPE_STEPS, PIPE_SPG = 6, 8, 4


def _sha(t) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def digests(m, eng, n_steps: int) -> dict:
    import numpy as np
    import torch
    torch.cuda.synchronize()
    out = {}
    for name, g in m.groups.items():
        for b in ("p", "m", "v", "tgt"):
            if getattr(g, b) is not None:
                out[f"{name}.{b}"] = _sha(getattr(g, b))
    for k in ("log_alpha", "pid_state", "log_temperature", "scalar_leaves"):
        if isinstance(getattr(m, k, None), torch.Tensor):
            out[k] = _sha(getattr(m, k))
    if getattr(eng, "temp_mv", None) is not None:
        out["temp_mv"] = _sha(eng.temp_mv)
    assert n_steps <= eng.st.ring_len, "the statistics ring must still hold every step that is digested"
    stats = eng.st.read_stats_many(range(1, n_steps + 1))
    rows = np.asarray([stats[s] for s in range(1, n_steps + 1)], np.float32)
    out["stats"] = hashlib.sha256(rows.tobytes()).hexdigest()
    out["steps"] = eng.st.device_step()
    # [blocks, hits, misses] of every argument arena (core.ArgArena) this path captured with: all zero under OSRL_ARG_ARENA=0
    arenas = {"step": getattr(eng, "_arena", None), "direct": getattr(eng, "_arena_direct", None),
              "pipelined": getattr(getattr(eng, "_pipe", None), "_arena", None)}
    out["arena"] = {k: [a.blocks, a.hits, a.misses] for k, a in arenas.items() if a is not None}
    return out


def run_mlp(c) -> dict:
    import torch
    from gpu_util import build_gpu, gpu_batch, gpu_step
    from osrl_amd.common.replay import ReplayStore, synthetic_transitions

    def on_store(prepare=None, pipelined=False):
        m, tr, lg = build_gpu(c, stats_mode="none", use_graph=True)
        eng = m.engine(c.B)
        eng.attach_replay(ReplayStore(synthetic_transitions(4096, c.od, c.ad, seed=7, max_action=c.max_action),
                                      torch.device(DEV), reward_scale=0.1, cost_scale=1.0, seed=3,
                                      state_init=c.algo == "coptidice"))
        if prepare is not None:
            prepare(eng)
        if pipelined:
            eng.steps_replay(PIPE_STEPS, steps_per_graph=PIPE_SPG)
            return digests(m, eng, PIPE_STEPS)
        for _ in range(STEPS):
            eng.step_replay(True)
        return digests(m, eng, STEPS)

    out = {"graph": on_store()}
    m, tr, lg = build_gpu(c, stats_mode="none", use_graph=False)
    b = gpu_batch(c, DEV)
    for s in range(STEPS):
        gpu_step(tr, c, b, s)
    out["eager"] = digests(m, m._engine, STEPS)
    if c.algo in ("cpq", "bcql"):
        out["pipelined"] = on_store(pipelined=True)
    if c.algo == "cpq":
        out["sequential"] = on_store(lambda e: setattr(e, "parallel_branches", False))
    if c.algo == "bc":
        out["graph_plan"] = on_store(lambda e: setattr(e, "direct", False))
    return out


def run_cdt(c) -> dict:
    import torch
    from cases import make_cdt_batch
    from test_gpu_cdt import build_cdt_gpu
    out = {}
    for path, use_graph in (("graph", True), ("eager", False)):
        m, tr, lg = build_cdt_gpu(c, stats_mode="none", use_graph=use_graph)
        b = {k: torch.from_numpy(v).to(DEV) for k, v in make_cdt_batch(c).items()}
        for _ in range(STEPS):
            tr.train_one_step(b["states"], b["actions"], b["returns"], b["costs_return"], b["time_steps"], b["mask"],
                              b["episode_cost"], b["costs"])
        out[path] = digests(m, m._engine, STEPS)
    return out


def run_dyn(kw) -> dict:
    import numpy as np
    import torch
    import dyn_ensemble_cases as DC
    import gauss_dynamics_cases as GC
    from osrl_amd.algorithms import Dynamics, DynamicsTrainer
    from osrl_amd.common.replay import ReplayStore
    T = DC.TRAIN
    if kw.get("bootstrap"):
        kw = dict(kw, boot_seed=DC.BOOT_SEED)
    data = DC.transitions(T["B"] * T["steps"] + 213, T["od"], T["ad"])
    out = {}
    for path, use_graph in (("graph", True), ("eager", False)):
        torch.manual_seed(9)
        m = Dynamics(T["od"], T["ad"], list(T["hidden"]), num_models=T["M"], device=DEV, **kw)
        store = ReplayStore(data, torch.device(DEV), seed=5)
        m.fit_normalizer(store)
        if kw.get("probabilistic"):
            sd = GC.with_logvar_rows({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, T["od"], T["M"])
            m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
        DynamicsTrainer(m, lr=T["lr"], stats_mode="none")
        eng = m.engine(T["B"])
        eng.attach_replay(store)
        for _ in range(STEPS):
            eng.step_replay(use_graph=use_graph)
        out[path] = digests(m, eng, STEPS)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", action="append", choices=CASES, help="repeatable; default: all of them")
    ap.add_argument("--out", default="engine_ab.json")
    a = ap.parse_args()
    from cases import BEARL_CASES, CASES as MLP, CDT_CASES, COPTIDICE_CASES
    res = {"what": "SHA-256 of every group buffer, scalar-state tensor and of the statistics of all steps, per case and path "
                   "(tools/engine_ab.py)",
           "seeds": {"cases": "tests/cases.py", "synthetic_transitions": 7, "replay_store": 3, "engine": 0},
           "steps": {"graph": STEPS, "eager": STEPS, "pipelined": [PIPE_STEPS, PIPE_SPG]}, "cases": {}}
    for name in a.case or CASES:
        if name in DYN_CASES:
            res["cases"][name] = run_dyn(DYN_CASES[name])
        elif name in CDT_CASES:
            res["cases"][name] = run_cdt(CDT_CASES[name])
        else:
            res["cases"][name] = run_mlp({**MLP, **BEARL_CASES, **COPTIDICE_CASES}[name])
        print(name, {p: (d["stats"][:12], d["arena"]) for p, d in res["cases"][name].items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
