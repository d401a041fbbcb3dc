"""Fitted Q evaluation (osrl_amd.algorithms.FQE) at C2's shape -- (obs, act) = (76, 2), batch 2048, hidden [256, 256],
num_q = 2, a CPQ policy -- against two yardsticks taken in the same process, interleaved (A B C C B A per round):

* ``fqe``      the FQE step as shipped: one-step hipGraph, minibatch drawn inside the step from the attached store;
* ``cpq``      the CPQ train step on the same store (one-step graph: the same launch discipline, a heavier step);
* ``autograd`` the same FQE update written the way a user would without the engine: ``ops.mlp_apply`` under autograd,
               ``torch.optim.Adam`` on device, Polyak through ``torch._foreach_lerp_``, the batch indexed on the host
               (numpy) and copied to the device every step.

Every number is steps/s over ``--steps`` steps between two device synchronisations, after ``--warmup`` steps.
Writes profiles/fqe_bench.json (``--out``).  Needs an MI355X: there is no CPU path."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

OD, AD, B, HID, NUM_Q = 76, 2, 2048, [256, 256], 2
GAMMA, TAU, LR = 0.99, 0.005, 1e-3


def summary(v):
    v = sorted(v)
    return dict(min=round(v[0], 1), median=round(v[len(v) // 2], 1), max=round(v[-1], 1), n=len(v))


def rate(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


class AutogradFQE:
    """The FQE update through autograd and torch.optim.Adam on a second FQE model's parameters."""

    def __init__(self, policy, data, dev):
        from osrl_amd.algorithms import FQE
        from osrl_amd.common.net import net_desc_seq
        torch.manual_seed(1)
        m = self.model = FQE(policy, HID, GAMMA, TAU, NUM_Q, device=str(dev))
        self.policy, self.dev = policy, dev
        seq = lambda mod: net_desc_seq(list(mod.q_nets), 1.0)  # noqa: E731
        self.on = [seq(m.critic), seq(m.cost_critic)]
        self.tg = [seq(m.critic_old), seq(m.cost_critic_old)]
        self.params = [p for mod in (m.critic, m.cost_critic) for p in mod.parameters()]
        self.targets = [p for mod in (m.critic_old, m.cost_critic_old) for p in mod.parameters()]
        self.opt = torch.optim.Adam(self.params, lr=LR)
        done = np.logical_or(data["terminals"] == 1, data["timeouts"] == 1).astype(np.float32)
        self.host = [data["observations"], data["next_observations"], data["actions"], data["rewards"] * np.float32(0.1),
                     data["costs"], done]
        self.rs = np.random.RandomState(0)

    def step(self):
        from osrl_amd import ops
        idx = self.rs.randint(0, self.host[0].shape[0], B)
        obs, nobs, act, rew, cost, done = (torch.from_numpy(t[idx]).to(self.dev) for t in self.host)
        with torch.no_grad():
            a_next = ops.cpq_act(self.policy, nobs, True)[0]
            backups = [x[None] + GAMMA * (1 - done)[None] * ops.mlp_apply(d, nobs, a_next)[..., 0]
                       for d, x in zip(self.tg, (rew, cost))]
        loss = sum(((ops.mlp_apply(d, obs, act)[..., 0] - bk) ** 2).mean(1).sum() for d, bk in zip(self.on, backups))
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        with torch.no_grad():
            torch._foreach_lerp_([t.data for t in self.targets], [p.data for p in self.params], TAU)
        self.model.repack()  # the kernels read the packed copies of the parameters and of the targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1 << 18, help="transitions in the store")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fqe_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fqe_bench needs an MI355X (no CPU path): not measured")
    from osrl_amd.algorithms import CPQ, CPQTrainer, FQE, FQETrainer
    from osrl_amd.common.replay import ReplayStore, synthetic_transitions
    dev = torch.device("cuda", 0)
    data = synthetic_transitions(args.rows, OD, AD, seed=1)
    store = ReplayStore(data, dev, reward_scale=0.1, cost_scale=1.0, seed=1)  # what both engines draw from
    store_init = ReplayStore(data, dev, reward_scale=0.1, cost_scale=1.0, seed=1, state_init=True)  # what estimate() reads

    def cpq_model(seed):
        torch.manual_seed(seed)
        m = CPQ(OD, AD, 1.0, HID, HID, 400, 10, GAMMA, TAU, 0.5, 2, 2, 1.5, 10, 1000, device=str(dev))
        return m, CPQTrainer(m, None, None, actor_lr=1e-4, critic_lr=1e-3, alpha_lr=1e-4, vae_lr=1e-3, reward_scale=0.1,
                             stats_mode="none")

    policy, _ = cpq_model(0)          # the frozen policy both FQE arms evaluate
    trained, _ = cpq_model(0)         # the model the CPQ arm trains
    cpq_eng = trained.engine(B)
    cpq_eng.attach_replay(store)
    torch.manual_seed(1)
    fqe = FQE(policy, HID, GAMMA, TAU, NUM_Q, device=str(dev))
    tr = FQETrainer(fqe, critic_lr=LR, reward_scale=0.1, stats_mode="none")
    fqe_eng = fqe.engine(B)
    fqe_eng.attach_replay(store)
    auto = AutogradFQE(policy, data, dev)
    arms = dict(fqe=lambda: fqe_eng.step_replay(True), cpq=lambda: cpq_eng.step_replay(True), autograd=auto.step)
    for name, f in arms.items():  # captures, code objects, allocator: outside every timed window
        for _ in range(args.warmup):
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in arms}
    order = list(arms) + list(arms)[::-1]
    for _ in range(args.rounds):
        for name in order:
            n = args.steps if name != "autograd" else max(args.steps // 5, 20)
            res[name].append(rate(arms[name], n))
    est = tr.estimate(store_init)
    out = dict(shape=dict(obs=OD, act=AD, batch=B, hidden=HID, num_q=NUM_Q, policy="cpq", store_rows=args.rows),
               device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, rounds=args.rounds,
               order="fqe cpq autograd autograd cpq fqe per round",
               steps_per_s={k: summary(v) for k, v in res.items()}, raw={k: [round(x, 1) for x in v] for k, v in res.items()},
               fqe_over_autograd=round(summary(res["fqe"])["median"] / summary(res["autograd"])["median"], 2),
               fqe_over_cpq=round(summary(res["fqe"])["median"] / summary(res["cpq"])["median"], 2),
               estimate_after_run=est._asdict())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["steps_per_s"]), "fqe/autograd", out["fqe_over_autograd"], "fqe/cpq", out["fqe_over_cpq"])


if __name__ == "__main__":
    main()
