"""Planning at act time (``Trainer.planner`` / engine/mpc.py ``ModelPlanner``) measured: what one ``act`` costs, and what
the feature cost the paths it did not touch.  The shape is C2's: a CPQ policy at (obs, act) = (76, 2), hidden [256, 256],
on a ``ModelVecEnv`` of 5 members with hidden [200, 200, 200].

(a) reported, not gated: microseconds per ``planner.act`` (upload, fan-out, H recorded model steps on N * K episodes,
    select, one host sync) at N in {1, 16} slots, K in {64, 256} candidates, H in {3, 5} steps, beside the microseconds
    per policy call of ``rollout_many`` of the bare policy (``VecFastPolicy``, one launch per call) on the same N host
    ``SyntheticSafeEnv``s.  Both sides run in child processes alternating A B B A (planner, policy, policy, planner);
    medians over every repeat of a side.  The ``rollout_many`` figure includes the host environments' own steps
    (``env_step_us`` is measured beside it and reported).
(b) with ``--parent DIR`` (a built checkout of the parent commit): the untouched ``collect_model(horizon=5)`` (ms per
    call at 1024 episodes) and ``bench.py --gpus 1 --steps 20 --warmup 5`` (its timed region) of this tree against the
    parent's, child processes A B B A.  ``ratio`` = parent median / this tree's median (bench.py: this tree's / the
    parent's, so that above 1 is faster in both); ``parent_spread`` = the parent's own max / min over its repeats;
    ``ok``: the ratio lies inside [1 / parent_spread, parent_spread].

(c) with ``--terminal``, reported, not gated: microseconds per ``act`` without and with ``terminal=`` (an ``FQE`` of the
    policy, [256, 256] critics, num_q = 2: one more launch, csrc/plan_value.hip) at the same N, K, H grid, and the same
    ``Q(s, pi(s))`` taken by the existing launch chain (``PolicyForward`` + ``MlpRun`` on E = N K rows, then a stream
    sync) for scale; the three sides interleave A B C C B A in ONE child process.  With ``--parent`` as well, the
    untouched ``act`` (no terminal) of this tree against the parent's, child processes A B B A, gated like (b).

(d) with ``--quantiles M``, ALONE (parts a to c are not run; the output is profiles/plan_quantile_bench.json): reported, not
    gated, microseconds per ``act`` with a quantile terminal (``FQE(num_quantiles=M)``, ``risk_alpha = 0.25``: one launch,
    csrc/plan_value_quantile.hip), with the scalar terminal, and the same per-row CVaR by the existing launch chain
    (``PolicyForward`` + ``MlpRun`` with M outputs, ``torch.sort`` and the tail mean on E = N K rows, then a stream sync),
    A B C C B A in one child process.  With ``--parent``: the untouched scalar-terminal ``act`` and ``bench.py`` of this
    tree against the parent's, child processes A B B A, gated like (b).

(e) with ``--refine R``, ALONE (the output is profiles/plan_refine_bench.json): reported, not gated, microseconds per ``act``
    with ``refine_rounds`` = 0, 1, .., R (csrc/plan_refine.hip: each round is one more fan-out, H-step run and refit, so
    roughly (rounds + 1) times the R = 0 call), the sides interleaved 0 1 .. R R .. 1 0 in one child process.  With
    ``--parent``: the untouched ``act`` (``refine_rounds=0``) and ``bench.py`` of this tree against the parent's, child
    processes A B B A, gated like (b).

(f) with ``--split``, ALONE (merged into profiles/model_env_split_bench.json, which tools/model_env_bench.py --split writes
    too): reported, not gated, microseconds per ``act`` on ``ModelVecEnv(split_members=True)`` (csrc/model_env_split.hip:
    one workgroup per tile and member) against the plain environment, the same policy and model, A B B A in one child
    process.  With ``--parent``: the untouched plain ``act`` and ``bench.py`` of this tree against the parent's, child
    processes A B B A, gated like (b).

Every repeat is kept.  Writes profiles/plan_bench.json (``--out``).  Needs an MI355X: there is no CPU path."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(od=76, ad=2, hidden=[256, 256], members=5, model_hidden=[200, 200, 200], slots=[1, 16], candidates=[64, 256],
             horizons=[3, 5], episode_len=50, collect_episodes=1024, collect_horizon=5)
BENCH_CMD = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-roofline", "--no-extras"]


def summary(v):
    s = sorted(v)
    return dict(min=round(s[0], 3), median=round(s[len(s) // 2], 3), max=round(s[-1], 3), n=len(s), all=[round(x, 3) for x in v])


def make(episodes, episode_len):
    """(trainer, model environment): only what the parent commit has as well."""
    import numpy as np
    import torch
    from osrl_amd.algorithms import CPQ, CPQTrainer, Dynamics
    from osrl_amd.common.logger import DummyLogger
    from osrl_amd.common.model_env import ModelVecEnv
    from osrl_amd.common.replay import synthetic_transitions
    s = SHAPE
    d = synthetic_transitions(4096, s["od"], s["ad"], seed=1)
    d["next_observations"] = (d["observations"] + 0.1 * d["next_observations"]).astype(np.float32)
    torch.manual_seed(0)
    dyn = Dynamics(s["od"], s["ad"], s["model_hidden"], num_models=s["members"], device="cuda:0")
    dyn.fit_normalizer(d)
    cpq = CPQ(s["od"], s["ad"], 1.0, s["hidden"], s["hidden"], 400, 10, episode_len=s["episode_len"], device="cuda:0")
    menv = ModelVecEnv(dyn, d["observations"][:episodes], episodes, episode_len, reward_penalty=0.5)
    tr = CPQTrainer(cpq, menv, DummyLogger(), 1e-4, 1e-3, 1e-4, 1e-3, device="cuda:0", stats_mode="none")
    return tr, menv


def host_envs(n):
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    s = SHAPE
    return [SyntheticSafeEnv(s["od"], s["ad"], s["episode_len"], seed=3 + e, init_noise=0.5) for e in range(n)]


def worker(tree, what, reps):
    """Runs in a child process with ``tree`` first on the path."""
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    s, out = SHAPE, {}
    if what == "untouched":
        tr, menv = make(s["collect_episodes"], s["collect_horizon"])
        kw = dict(horizon=s["collect_horizon"], noise_std=0.3)
        tr.collect_model(menv, seed=0, **kw)
        ms = []
        for i in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.collect_model(menv, seed=1 + i, **kw)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        out["collect_model_ms"] = ms
    elif what in ("plan", "plan_terminal"):
        from osrl_amd.algorithms.fqe import FQE
        for n in s["slots"]:
            states = np.stack([e.reset(seed=i)[0] for i, e in enumerate(host_envs(n))]).astype(np.float32)
            for k in s["candidates"]:
                for h in s["horizons"]:
                    tr, menv = make(n * k, h)
                    kw = {}
                    if what == "plan_terminal":  # (the scalar terminal: what the parent commit has as well)
                        kw = dict(gamma=0.99, terminal=FQE(tr.model, s["hidden"], 0.99, num_q=2, device="cuda:0"))
                    p = tr.planner(menv, n, h, noise_std=0.3, **kw)
                    for _ in range(3):
                        p.act(states, 5.0)
                    us = []
                    for _ in range(reps * 10):
                        t0 = time.perf_counter()
                        p.act(states, 5.0)
                        us.append((time.perf_counter() - t0) * 1e6)
                    out[f"N{n}_K{k}_H{h}"] = us
                    del p, tr, menv
    elif what == "terminal":
        from osrl_amd.algorithms.fqe import FQE
        from osrl_amd.engine.core import MlpRun
        from osrl_amd.engine.fqe import PolicyForward, _critic_descs
        dev = torch.device("cuda:0")
        for n in s["slots"]:
            states = np.stack([e.reset(seed=i)[0] for i, e in enumerate(host_envs(n))]).astype(np.float32)
            for k in s["candidates"]:
                for h in s["horizons"]:
                    tr, menv = make(n * k, h)
                    fqe = FQE(tr.model, s["hidden"], 0.99, num_q=2, device="cuda:0")
                    kw = dict(noise_std=0.3, gamma=0.99)
                    p0, p1 = tr.planner(menv, n, h, **kw), tr.planner(menv, n, h, terminal=fqe, **kw)
                    pi, rq = PolicyForward(tr.model, "cpq", n * k, dev), MlpRun(_critic_descs(fqe)[0], n * k, False, dev)

                    def chain():
                        rq.forward(p0.obs, pi.forward(p0.obs))
                        torch.cuda.synchronize()
                    sides = dict(act=lambda: p0.act(states, 5.0), act_terminal=lambda: p1.act(states, 5.0), chain=chain)
                    us = {name: [] for name in sides}
                    for i in range(3 + reps * 10):
                        for name in ("act", "act_terminal", "chain", "chain", "act_terminal", "act"):
                            t0 = time.perf_counter()
                            sides[name]()
                            if i >= 3:
                                us[name].append((time.perf_counter() - t0) * 1e6)
                    out[f"N{n}_K{k}_H{h}"] = us
                    del p0, p1, pi, rq, fqe, tr, menv
    elif what.startswith("refine"):
        rounds = list(range(int(what[6:]) + 1))
        for n in s["slots"]:
            states = np.stack([e.reset(seed=i)[0] for i, e in enumerate(host_envs(n))]).astype(np.float32)
            for k in s["candidates"]:
                for h in s["horizons"]:
                    tr, menv = make(n * k, h)
                    ps = [tr.planner(menv, n, h, noise_std=0.3, refine_rounds=r) for r in rounds]
                    us = {f"R{r}": [] for r in rounds}
                    for i in range(3 + reps * 10):
                        for r in rounds + rounds[::-1]:  # A B C D D C B A
                            t0 = time.perf_counter()
                            ps[r].act(states, 5.0)
                            if i >= 3:
                                us[f"R{r}"].append((time.perf_counter() - t0) * 1e6)
                    out[f"N{n}_K{k}_H{h}"] = us
                    del ps, tr, menv
    elif what == "split":
        for n in s["slots"]:
            states = np.stack([e.reset(seed=i)[0] for i, e in enumerate(host_envs(n))]).astype(np.float32)
            for k in s["candidates"]:
                for h in s["horizons"]:
                    ps = {}
                    for name in ("plain", "split"):  # (make() seeds alike: the same policy and model on both sides)
                        tr, menv = make(n * k, h)
                        menv.split_members = name == "split"
                        ps[name] = (tr.planner(menv, n, h, noise_std=0.3), tr, menv)
                    us = {name: [] for name in ps}
                    for i in range(3 + reps * 10):
                        for name in ("plain", "split", "split", "plain"):
                            t0 = time.perf_counter()
                            ps[name][0].act(states, 5.0)
                            if i >= 3:
                                us[name].append((time.perf_counter() - t0) * 1e6)
                    out[f"N{n}_K{k}_H{h}"] = us
                    del ps
    elif what.startswith("quantile"):
        from osrl_amd.algorithms.fqe import FQE, tail_count
        from osrl_amd.engine.core import MlpRun
        from osrl_amd.engine.fqe import PolicyForward, _critic_descs
        dev, M, alpha = torch.device("cuda:0"), int(what[8:]), 0.25
        for n in s["slots"]:
            states = np.stack([e.reset(seed=i)[0] for i, e in enumerate(host_envs(n))]).astype(np.float32)
            for k in s["candidates"]:
                for h in s["horizons"]:
                    tr, menv = make(n * k, h)
                    fs = FQE(tr.model, s["hidden"], 0.99, num_q=2, device="cuda:0")
                    fq = FQE(tr.model, s["hidden"], 0.99, num_q=2, num_quantiles=M, device="cuda:0")
                    kw = dict(noise_std=0.3, gamma=0.99)
                    ps = tr.planner(menv, n, h, terminal=fs, **kw)
                    pq = tr.planner(menv, n, h, terminal=fq, risk_alpha=alpha, **kw)
                    pi, rq = PolicyForward(tr.model, "cpq", n * k, dev), MlpRun(_critic_descs(fq)[0], n * k, False, dev)
                    kt = tail_count(alpha, M)

                    def chain():
                        th = torch.sort(rq.forward(ps.obs, pi.forward(ps.obs)).view(4, n * k, M), -1).values
                        cvar = (th[:2, :, :kt].mean(-1).mean(0), th[2:, :, M - kt:].mean(-1).mean(0))  # noqa: F841
                        torch.cuda.synchronize()
                    sides = dict(act_scalar=lambda: ps.act(states, 5.0), act_quantile=lambda: pq.act(states, 5.0), chain=chain)
                    us = {name: [] for name in sides}
                    for i in range(3 + reps * 10):
                        for name in ("act_scalar", "act_quantile", "chain", "chain", "act_quantile", "act_scalar"):
                            t0 = time.perf_counter()
                            sides[name]()
                            if i >= 3:
                                us[name].append((time.perf_counter() - t0) * 1e6)
                    out[f"N{n}_K{k}_H{h}"] = us
                    del ps, pq, pi, rq, fs, fq, tr, menv
    else:  # "policy": rollout_many of the bare policy on the same N host environments
        tr, _ = make(16, 5)
        for n in s["slots"]:
            envs = host_envs(n)
            tr.rollout_many(envs)
            us = []
            for _ in range(reps):
                t0 = time.perf_counter()
                tr.rollout_many(envs)
                us.append((time.perf_counter() - t0) * 1e6 / s["episode_len"])
            a = np.zeros(s["ad"], np.float32)
            for e in envs:
                e.reset()
            t0 = time.perf_counter()
            for _ in range(s["episode_len"]):
                for e in envs:
                    e.step(a)
            out[f"N{n}"] = dict(per_call_us=us, env_step_us=(time.perf_counter() - t0) * 1e6 / s["episode_len"])
    print("RESULT " + json.dumps(out))


def child(tree, what, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--tree", tree, "--reps", str(reps)]
    env = dict(os.environ)
    lib = os.path.join(tree, "osrl_amd", "lib", "libosrl_amd.so")
    if os.path.exists(lib):  # each tree measures the library it was built with, whatever the files' times say
        env["OSRL_LIB"] = lib
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tree, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"worker {what} failed in {tree}: {r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def bench_child(tree):
    """'value' of one ``bench.py`` process of ``tree`` (its own library, its own bench.py)."""
    env = dict(os.environ)
    lib = os.path.join(tree, "osrl_amd", "lib", "libosrl_amd.so")
    if os.path.exists(lib):
        env["OSRL_LIB"] = lib
    r = subprocess.run([sys.executable] + BENCH_CMD, capture_output=True, text=True, timeout=900, cwd=tree, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py failed in {tree}: {r.stderr[-2000:]}")
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{") and '"value"' in ln]
    return float(rows[-1]["value"])


def gate(here, there, higher_is_better=False):
    h, t = summary(here), summary(there)
    ratio = h["median"] / t["median"] if higher_is_better else t["median"] / h["median"]
    spread = t["max"] / t["min"]
    return dict(this_tree=h, parent=t, ratio=round(ratio, 4), parent_spread=round(spread, 4),
                ok=bool(1.0 / spread <= ratio <= spread))


def against_parent(parent, reps, rounds):
    ch, ct, bh, bt = [], [], [], []
    for _ in range(rounds):  # A B B A
        for tree, c, b in ((ROOT, ch, bh), (parent, ct, bt), (parent, ct, bt), (ROOT, ch, bh)):
            c += child(tree, "untouched", reps)["collect_model_ms"]
            b.append(bench_child(tree))
            print(f"{'this tree' if tree == ROOT else 'parent'}: bench {b[-1]}", file=sys.stderr, flush=True)
    return dict(collect_model_horizon5_ms=gate(ch, ct),
                bench=dict(command="python " + " ".join(BENCH_CMD), unit="grad-steps/s", **gate(bh, bt, higher_is_better=True)))


def terminal_rows(reps, rounds):
    got = {}
    for _ in range(rounds):
        for k, v in child(ROOT, "terminal", reps).items():
            for name, us in v.items():
                got.setdefault(k, {}).setdefault(name, []).extend(us)
    rows = {}
    for k, v in got.items():
        a, b, c = summary(v["act"]), summary(v["act_terminal"]), summary(v["chain"])
        rows[k] = dict(act_us=a, act_terminal_us=b, launch_chain_us=c, added_us=round(b["median"] - a["median"], 3))
    return rows


def quantile_rows(M, reps, rounds):
    got = {}
    for _ in range(rounds):
        for k, v in child(ROOT, f"quantile{M}", reps).items():
            for name, us in v.items():
                got.setdefault(k, {}).setdefault(name, []).extend(us)
    rows = {}
    for k, v in got.items():
        a, b, c = summary(v["act_scalar"]), summary(v["act_quantile"]), summary(v["chain"])
        rows[k] = dict(act_scalar_terminal_us=a, act_quantile_terminal_us=b, launch_chain_us=c,
                       quantile_minus_scalar_us=round(b["median"] - a["median"], 3))
    return rows


def refine_rows(R, reps, rounds):
    got = {}
    for _ in range(rounds):
        for k, v in child(ROOT, f"refine{R}", reps).items():
            for name, us in v.items():
                got.setdefault(k, {}).setdefault(name, []).extend(us)
    rows = {}
    for k, v in got.items():
        base = summary(v["R0"])
        rows[k] = {f"act_{name}_us": summary(us) for name, us in v.items()}
        rows[k]["ratio_to_R0"] = {name: round(summary(us)["median"] / base["median"], 3) for name, us in v.items()}
    return rows


def split_rows(reps, rounds):
    got = {}
    for _ in range(rounds):
        for k, v in child(ROOT, "split", reps).items():
            for name, us in v.items():
                got.setdefault(k, {}).setdefault(name, []).extend(us)
    rows = {}
    for k, v in got.items():
        a, b = summary(v["plain"]), summary(v["split"])
        rows[k] = dict(act_plain_us=a, act_split_us=b, plain_over_split=round(a["median"] / b["median"], 3))
    return rows


def merge_into(path, update):
    """``update``'s keys into the JSON at ``path`` (tools/model_env_bench.py --split writes the same file)."""
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)
    out.update(update)
    return write(out, path)


def bench_against_parent(parent, rounds):
    here, there = [], []
    for _ in range(rounds):  # A B B A
        for tree, acc in ((ROOT, here), (parent, there), (parent, there), (ROOT, here)):
            acc.append(bench_child(tree))
            print(f"{'this tree' if tree == ROOT else 'parent'}: bench {acc[-1]}", file=sys.stderr, flush=True)
    return dict(command="python " + " ".join(BENCH_CMD), unit="grad-steps/s", **gate(here, there, higher_is_better=True))


def act_against_parent(parent, reps, rounds, what="plan"):
    here, there = {}, {}
    for _ in range(rounds):  # A B B A
        for tree, acc in ((ROOT, here), (parent, there), (parent, there), (ROOT, here)):
            for k, v in child(tree, what, reps).items():
                acc.setdefault(k, []).extend(v)
            print(f"{'this tree' if tree == ROOT else 'parent'}: {what} done", file=sys.stderr, flush=True)
    return {k: gate(here[k], there[k]) for k in here}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="profiles/plan_bench.json, with --quantiles profiles/plan_quantile_bench.json")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part b)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1, help="A B B A rounds")
    ap.add_argument("--terminal", action="store_true", help="part c: act with and without terminal=, and the launch chain")
    ap.add_argument("--quantiles", type=int, default=None, metavar="M", help="part d alone: act with a quantile terminal")
    ap.add_argument("--refine", type=int, default=None, metavar="R", help="part e alone: act with 1 .. R refinement rounds")
    ap.add_argument("--split", action="store_true", help="part f alone: act on a split_members environment against the plain one")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.tree), args.worker, args.reps)
    if args.quantiles:
        out = dict(shape=SHAPE, quantiles=args.quantiles, risk_alpha=0.25,
                   quantile_terminal=quantile_rows(args.quantiles, args.reps, args.rounds), scalar_terminal_act_vs_parent=None,
                   bench_vs_parent=None)
        if args.parent:
            parent = os.path.abspath(args.parent)
            out["scalar_terminal_act_vs_parent"] = act_against_parent(parent, args.reps, args.rounds, "plan_terminal")
            out["bench_vs_parent"] = bench_against_parent(parent, args.rounds)
        return write(out, args.out or os.path.join(ROOT, "profiles", "plan_quantile_bench.json"))
    if args.refine:
        out = dict(shape=SHAPE, refine_rounds=args.refine, refine=refine_rows(args.refine, args.reps, args.rounds),
                   act_vs_parent=None, bench_vs_parent=None)
        if args.parent:
            parent = os.path.abspath(args.parent)
            out["act_vs_parent"] = act_against_parent(parent, args.reps, args.rounds)
            out["bench_vs_parent"] = bench_against_parent(parent, args.rounds)
        return write(out, args.out or os.path.join(ROOT, "profiles", "plan_refine_bench.json"))
    if args.split:
        out = dict(plan_shape=SHAPE, act_split_vs_plain=split_rows(args.reps, args.rounds))
        if args.parent:
            parent = os.path.abspath(args.parent)
            out["plain_act_vs_parent"] = act_against_parent(parent, args.reps, args.rounds)
            out["bench_vs_parent"] = bench_against_parent(parent, args.rounds)
        return merge_into(args.out or os.path.join(ROOT, "profiles", "model_env_split_bench.json"), out)
    plan, pol, env_us = {}, {}, {}
    for _ in range(args.rounds):  # A B B A: planner, policy, policy, planner
        for what in ("plan", "policy", "policy", "plan"):
            got = child(ROOT, what, args.reps)
            for k, v in got.items():
                if what == "plan":
                    plan.setdefault(k, []).extend(v)
                else:
                    pol.setdefault(k, []).extend(v["per_call_us"])
                    env_us.setdefault(k, []).append(v["env_step_us"])
    rows = {}
    for k, v in plan.items():
        n = k.split("_")[0]
        a, b = summary(v), summary(pol[n])
        rows[k] = dict(act_us=a, rollout_many_per_call_us=b, env_step_us=round(sorted(env_us[n])[len(env_us[n]) // 2], 3),
                       ratio=round(a["median"] / b["median"], 3))
    out = dict(shape=SHAPE, act_vs_rollout_many=rows, vs_parent=None, terminal=None, act_vs_parent=None)
    if args.parent:
        out["vs_parent"] = against_parent(os.path.abspath(args.parent), args.reps, args.rounds)
    if args.terminal:
        out["terminal"] = terminal_rows(args.reps, args.rounds)
        if args.parent:
            out["act_vs_parent"] = act_against_parent(os.path.abspath(args.parent), args.reps, args.rounds)
    write(out, args.out or os.path.join(ROOT, "profiles", "plan_bench.json"))


def write(out, path):
    import torch  # (after the children: this process never opens the device before them)
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
