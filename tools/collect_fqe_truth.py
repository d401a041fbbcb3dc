"""How far fitted Q evaluation lands from the Monte-Carlo truth on collected data, in fp64 on the CPU: the measurement
behind the absolute gate of tests/test_gpu_collect.py::test_fqe_against_the_truth.

The setup is tests/collect_cases.py: two BC policies (A and its mirror), each collected for 256 episodes with per-episode
exploration noise by the numpy restatement (tests/collect_oracle.py), the two collections merged; per policy,
``OracleFQE`` (tests/fqe_oracle.py) runs the test's number of steps on uniform minibatches, three minibatch seeds; the
truth is the policy's noise-free mean discounted return from the same initial states.  Writes every run's error to
profiles/collect_fqe_truth.json; the test's bound is twice the worst.

    python tools/collect_fqe_truth.py [--truth-only] [--seeds 0 1 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import collect_cases as CC  # noqa: E402
from collect_oracle import collect  # noqa: E402
from fqe_oracle import OracleFQE, policy_action  # noqa: E402


def critic_state_dict(seed):
    torch.manual_seed(seed)
    sizes = [CC.OD + CC.AD] + CC.FQE_HIDDEN + [1]
    sd = {}
    for ens in ("critic", "cost_critic"):
        for e in range(CC.FQE_NUM_Q):
            for i in range(len(sizes) - 1):
                lin = torch.nn.Linear(sizes[i], sizes[i + 1])
                for tgt in ("", "_old"):
                    sd[f"{ens}{tgt}.q_nets.{e}.{2 * i}.weight"] = lin.weight.data.clone()
                    sd[f"{ens}{tgt}.q_nets.{e}.{2 * i}.bias"] = lin.bias.data.clone()
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--truth-only", action="store_true")
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--out", default=os.path.join(ROOT, CC.TRUTH_JSON))
    a = ap.parse_args()
    torch.set_num_threads(1)
    sds = CC.policies()
    acts = {k: policy_action("bc", {n: v.numpy().astype(np.float64) for n, v in sd.items()}, 1.0) for k, sd in sds.items()}
    truth, data = {}, []
    for name, act in acts.items():
        det = collect(CC.make_env, lambda o, act=act: act(o), CC.BASE_SEED, CC.EPISODES, CC.EL, gamma=CC.GAMMA)
        truth[name] = dict(value=float(det.disc_returns.mean()), cost_value=float(det.disc_cost_returns.mean()))
        noisy = collect(CC.make_env, lambda o, act=act: act(o), CC.BASE_SEED, CC.EPISODES, CC.EL, sigma=CC.sigmas(),
                        eps=CC.injected_noise(name), gamma=CC.GAMMA)
        data.append(noisy.dataset)
        print(name, truth[name], "clipped actions:", float((np.abs(noisy.dataset["actions"]) == 1.0).mean()), flush=True)
    print("true reward gap", truth["A"]["value"] - truth["mirror"]["value"], flush=True)
    if a.truth_only:
        return
    d = {k: np.concatenate([x[k] for x in data]) for k in data[0]}
    done = np.maximum(d["terminals"], d["timeouts"])
    init = np.concatenate([[1.0], done[:-1]]) == 1
    s0 = d["observations"][init]
    assert s0.shape[0] == 2 * CC.EPISODES
    n = len(done)
    runs = []
    for name, act in acts.items():
        for seed in a.seeds:
            t0 = time.time()
            o = OracleFQE(critic_state_dict(1000 + seed), act, CC.GAMMA, CC.FQE_TAU, CC.FQE_LR)
            rs = np.random.RandomState(seed)
            for _ in range(CC.FQE_STEPS):
                i = rs.randint(0, n, CC.FQE_BATCH)
                o.step(d["observations"][i], d["next_observations"][i], d["actions"][i], d["rewards"][i], d["costs"][i],
                       done[i])
            est = o.estimate(s0)
            run = dict(policy=name, minibatch_seed=seed, value=est[0], cost_value=est[2],
                       value_error=abs(est[0] - truth[name]["value"]),
                       cost_value_error=abs(est[2] - truth[name]["cost_value"]))
            runs.append(run)
            print(run, f"{time.time() - t0:.0f}s", flush=True)
    out = dict(setup={k: getattr(CC, k) for k in ("OD", "AD", "EL", "GAMMA", "INIT_NOISE", "ENV_SEED", "BASE_SEED", "EPISODES",
                                                   "POLICY_HIDDEN", "POLICY_SEED", "LAST_LAYER_SCALE", "SIGMAS", "FQE_HIDDEN",
                                                   "FQE_NUM_Q", "FQE_STEPS", "FQE_BATCH", "FQE_LR", "FQE_TAU")},
               truth=truth, runs=runs,
               worst_value_error=max(r["value_error"] for r in runs),
               worst_cost_value_error=max(r["cost_value_error"] for r in runs),
               note="fp64 OracleFQE on the numpy restatement's data; the GPU test's bound is twice the worst error")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
