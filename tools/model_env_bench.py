"""``evaluate`` on a learned-dynamics environment (common/model_env.py) measured in one session, interleaved repeats
(A B B A), medians:

(a) a CPQ policy at C2's shape (obs 76, act 2) on a ``ModelVecEnv`` (5 members, hidden [200, 200, 200]) at 256 and 1024
    episodes of 200 steps, in env-steps/s; beside it the same policy on ``VecSyntheticSafeEnv``, for scale only (its step
    is a 76 x 78 matrix-vector product per episode, the model's five three-layer MLPs);
(b) CDT at C5's model shape (obs 11, act 3, seq_len 20, embed 256, 8 heads, 3 layers) at 256 episodes;
(c) the return / cost gap between the two environments, same policy, same initial states, for a model fitted (``--fit-steps``
    steps, batch 256) on data ``collect``ed from the synthetic one -- with the model's own trust signal, ``disagreement()``.

Nothing is gated.  Writes profiles/model_env_bench.json (``--out``)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EL = 200
CALLS = 5  # evaluate() calls per timed sample


def summary(v):
    v = sorted(v)
    return dict(min=round(v[0], 3), median=round(v[len(v) // 2], 3), max=round(v[-1], 3), n=len(v), all=[round(x, 3) for x in v])


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def abba(a, b, rounds):
    """ms per call of ``a`` and of ``b``: A B B A per round, every sample ``CALLS`` calls behind one synchronise."""
    ta, tb = [], []
    many = lambda f: timed(lambda: [f() for _ in range(CALLS)])[0] / CALLS  # noqa: E731
    for _ in range(rounds):
        ta.append(many(a))
        tb.append(many(b))
        tb.append(many(b))
        ta.append(many(a))
    return summary(ta), summary(tb)


def fit_model(od, ad, data, steps, dev, seed=0):
    import torch
    from osrl_amd.algorithms import Dynamics, DynamicsTrainer
    from osrl_amd.common.replay import ReplayStore
    store = ReplayStore(data, dev, seed=seed, state_init=True)
    torch.manual_seed(seed)
    dyn = Dynamics(od, ad, [200, 200, 200], num_models=5, device=str(dev))
    dyn.fit_normalizer(store)
    DynamicsTrainer(dyn, lr=1e-3, stats_mode="none")
    eng = dyn.engine(256)
    eng.attach_replay(store)
    ms, _ = timed(lambda: [eng.step_replay() for _ in range(steps)])
    loss = eng.st.read_stats()["loss/dynamics_loss"]
    return dyn, dict(rows=int(store.n_rows), steps=steps, batch=256, fit_ms=round(ms, 1),
                     steps_per_s=round(steps / ms * 1e3, 1), last_loss_sum_over_members=round(loss, 5))


def cpq_part(dev, rounds, fit_steps):
    import numpy as np
    import torch
    from osrl_amd.algorithms import CPQ, CPQTrainer
    from osrl_amd.common.model_env import ModelVecEnv
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv, VecSyntheticSafeEnv
    od, ad = 76, 2
    torch.manual_seed(0)
    cpq = CPQ(od, ad, 1.0, [256, 256], [256, 256], 400, 10, episode_len=EL, device=str(dev))
    host = SyntheticSafeEnv(od, ad, EL, seed=3, init_noise=0.5)
    out = {}
    real256 = VecSyntheticSafeEnv(host, 256, dev)
    data = CPQTrainer(cpq, env=real256, stats_mode="none").collect(noise_std=0.3, seed=1).dataset
    dyn, out["fit"] = fit_model(od, ad, data, fit_steps, dev)
    for E in (256, 1024):
        real = VecSyntheticSafeEnv(host, E, dev)
        model = ModelVecEnv(dyn, real.state0, E, EL)  # the same initial states, episode by episode
        tr_m, tr_r = CPQTrainer(cpq, env=model, stats_mode="none"), CPQTrainer(cpq, env=real, stats_mode="none")
        res_m, res_r = tr_m.evaluate(E), tr_r.evaluate(E)  # (warm: capture)
        sm, sr = abba(lambda: tr_m.evaluate(E), lambda: tr_r.evaluate(E), rounds)
        mx, mean = model.disagreement()
        out[f"episodes_{E}"] = dict(
            model_env_ms=sm, synthetic_env_ms=sr, model_env_steps_per_s=round(E * EL / sm["median"] * 1e3),
            synthetic_env_steps_per_s=round(E * EL / sr["median"] * 1e3),
            model_env=dict(zip(("return", "cost", "length"), map(float, res_m))),
            synthetic_env=dict(zip(("return", "cost", "length"), map(float, res_r))),
            return_gap=round(float(res_m[0] - res_r[0]), 4), cost_gap=round(float(res_m[1] - res_r[1]), 4),
            disagreement_max=round(float(np.max(mx)), 4), disagreement_mean=round(float(np.mean(mean)), 4))
    return out


def cdt_part(dev, rounds, fit_steps):
    import torch
    from osrl_amd.algorithms import BC, CDT, BCTrainer, CDTTrainer
    from osrl_amd.common.model_env import ModelVecEnv
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv, VecSyntheticSafeEnv
    od, ad, E = 11, 3, 256
    torch.manual_seed(0)
    cdt = CDT(od, ad, 1.0, seq_len=20, episode_len=EL, embedding_dim=256, num_layers=3, num_heads=8, use_rew=True,
              use_cost=True, cost_transform=True, stochastic=True, target_entropy=-ad, device=str(dev))
    bc = BC(od, ad, 1.0, [256, 256], EL, device=str(dev))
    host = SyntheticSafeEnv(od, ad, EL, seed=3, init_noise=0.5)
    real = VecSyntheticSafeEnv(host, E, dev)
    data = BCTrainer(bc, env=real, stats_mode="none").collect(noise_std=0.5, seed=1).dataset
    dyn, fit = fit_model(od, ad, data, fit_steps, dev)
    model = ModelVecEnv(dyn, real.state0, E, EL)
    tr_m, tr_r = CDTTrainer(cdt, env=model, stats_mode="none"), CDTTrainer(cdt, env=real, stats_mode="none")
    res_m, res_r = tr_m.evaluate(E, 100.0, 10.0), tr_r.evaluate(E, 100.0, 10.0)
    sm, sr = abba(lambda: tr_m.evaluate(E, 100.0, 10.0), lambda: tr_r.evaluate(E, 100.0, 10.0), rounds)
    return dict(fit=fit, episodes=E, model_env_ms=sm, synthetic_env_ms=sr,
                model_env_steps_per_s=round(E * EL / sm["median"] * 1e3),
                synthetic_env_steps_per_s=round(E * EL / sr["median"] * 1e3),
                model_env=dict(zip(("return", "cost", "length"), map(float, res_m))),
                synthetic_env=dict(zip(("return", "cost", "length"), map(float, res_r))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_env_bench.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fit-steps", type=int, default=2000)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    dev = torch.device("cuda", 0)
    out = dict(device=torch.cuda.get_device_name(0), episode_len=EL, members=5, hidden=[200, 200, 200],
               repeats_per_side=2 * args.rounds, calls_per_repeat=CALLS)
    out["cpq_c2_shape"] = cpq_part(dev, args.rounds, args.fit_steps)
    out["cdt_c5_shape"] = cdt_part(dev, args.rounds, args.fit_steps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
