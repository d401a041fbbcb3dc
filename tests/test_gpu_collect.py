"""On-device dataset collection (csrc/collect.hip, engine/collect.py) on the GPU.

Shapes, the smallest at which the kernel can go wrong: (od, ad, E) = (6, 2, 5) and (70, 5, 33) -- 70 states need two
waves and the cross-wave reduction, 5 action columns a second Philox counter, neither E fills a 16-row policy tile;
episode length 23 = one 20-step graph replay and a second that overshoots by 17 steps; hidden [32, 32].

Bounds (u = 2^-24, one fp32 rounding):
  * next state, per component: the device sums od + ad products with fmaf in four partial sums, numpy's fp32 matmul
    rounds every product and sum: each is within (od + ad + 2) u sum|terms| of the exact value, so they differ by at most
    b_i = (od + ad + 2) 2^-23 (sum_j |A_ij s_j| + sum_k |B_ik a_k|).
  * reward 1 - 0.1 sum d_i^2, d = s' - goal: the state difference moves it by 0.1 sum (2 |d_i| b_i + b_i^2), the
    od + 2 roundings of each side by (od + 2) 2^-23 (1 + 0.1 sum d_i^2).
  * s'.w: sum |w_i| b_i + (od + 2) 2^-23 sum |s'_i w_i|; costs are compared only on rows farther than that from 0.75.
  * discounted sums: gamma^t carries t - 1 roundings, the running fmaf sum one per later step: (L - 1) u sum|gamma^t x|,
    asserted as L 2^-24 sum|gamma^t x|.
  * actions against the fp64 oracle policy: the project's 1e-4 policy bound.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import collect_cases as CC
from fqe_oracle import policy_action

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HID, EL = [32, 32], 23
SMALL, BIG = (6, 2, 5), (70, 5, 33)
ENV_SEED, BASE_SEED = 3, 100  # (tests/test_collect_cpu.py checks this env's margin at the cost threshold on the CPU)
U23 = 2.0 ** -23


def make_env(od, ad):
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    return SyntheticSafeEnv(od, ad, 50, seed=ENV_SEED, init_noise=0.5)


def make_venv(od, ad, E, base_seed=BASE_SEED):
    from osrl_amd.common.synthetic_env import VecSyntheticSafeEnv
    return VecSyntheticSafeEnv(make_env(od, ad), E, DEV, base_seed=base_seed)


def make_model(kind, od, ad, seed=3):
    from osrl_amd.algorithms import BC, BCQL, CPQ, COptiDICE
    torch.manual_seed(seed)
    if kind == "bc":
        m = BC(od, ad, 1.0, HID, EL, device=DEV)
        m.load_state_dict(CC.bc_state_dict(od, ad, HID, seed))  # (the weights the CPU margin check uses)
        return m
    if kind == "cpq":
        return CPQ(od, ad, 1.0, HID, HID, 32, 2, episode_len=EL, device=DEV)
    if kind == "dice":
        return COptiDICE(od, ad, 1.0, "softchi", 0.15, np.ones((1, od), np.float32), np.ones((1, ad), np.float32), HID, HID,
                         episode_len=EL, device=DEV)
    return BCQL(od, ad, 1.0, HID, HID, 32, 2, episode_len=EL, device=DEV)


def oracle_policy(kind, model):
    p = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in model.state_dict().items()}
    f = policy_action(kind, p, 1.0)
    return lambda obs: f(np.asarray(obs, np.float64), None)


def npd(dataset):
    return {k: v.cpu().numpy() for k, v in dataset.items()}


def same_tables(a, b, rows=None):
    for k in a:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert torch.equal(x, y), k


def same_sums(a, b):
    for name, x, y in zip(a._fields[1:], a[1:], b[1:]):
        np.testing.assert_array_equal(x, y, err_msg=name)


@functools.lru_cache(maxsize=None)
def bc_setup(shape):
    """One BC model, environment and collector per shape, shared (read-only) by the tests below."""
    from osrl_amd.engine.collect import Collector
    od, ad, E = shape
    m = make_model("bc", od, ad)
    venv = make_venv(od, ad, E)
    return m, venv, Collector(m, venv, "bc", cost_scale=2.0, seed=7)


@functools.lru_cache(maxsize=None)
def bc_noisy(shape):
    """sigma = 0.3, gamma = 0.9, Philox noise, graph replay."""
    m, venv, col = bc_setup(shape)
    return col.run(0.3, gamma=0.9, seed=7)


# ------------------------------------------------------------------------------------------------------------------ #
# 1. sigma = 0 is evaluate
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("kind", ["bc", "cpq", "dice", "bcql"])
@pytest.mark.parametrize("shape", [SMALL, BIG])
def test_sigma_zero_is_evaluate(kind, shape):
    from osrl_amd.engine.collect import Collector
    from osrl_amd.engine.rollout import BatchedRollout
    od, ad, E = shape
    m, venv = make_model(kind, od, ad), make_venv(od, ad, E)
    z = None
    if kind == "bcql":
        z = torch.tensor(np.random.RandomState(5).randn(E, m.latent_dim).astype(np.float32), device=DEV)
    ref = BatchedRollout(m, venv, kind, 2.0, z=z).run()
    g = Collector(m, venv, kind, 2.0, z=z, use_graph=True).run(0.0)
    e = Collector(m, venv, kind, 2.0, z=z, use_graph=False).run(0.0)
    for name, want, got in zip(("returns", "cost_returns", "lengths"), ref, g[1:4]):
        np.testing.assert_array_equal(got, want, err_msg=name)
    assert (g.lengths == EL).all() and np.unique(g.returns).size == E
    same_tables(g.dataset, e.dataset)
    same_sums(g, e)
    np.testing.assert_array_equal(g.disc_returns, g.returns)  # gamma = None is 1.0
    np.testing.assert_array_equal(g.disc_cost_returns, g.cost_returns)


def test_trainer_collect_uses_evaluates_policy_and_caches_the_collector():
    """``BCTrainer.collect`` in multi-task mode: the appended cost limit reaches the policy and not the dataset."""
    from osrl_amd.algorithms import BC, BCTrainer
    from osrl_amd.common.logger import DummyLogger
    od, ad, E = SMALL
    torch.manual_seed(0)
    m = BC(od + 1, ad, 1.0, HID, EL, device=DEV)
    tr = BCTrainer(m, None, DummyLogger(), actor_lr=1e-3, bc_mode="multi-task", cost_limit=20, device=DEV)
    tr.env = make_venv(od, ad, E)
    tr.evaluate(E)
    ref = tr._rollout[1].run()
    c = tr.collect(0.0)
    col = tr._collector[1]
    np.testing.assert_array_equal(c.returns, ref[0])
    np.testing.assert_array_equal(c.cost_returns, ref[1])
    assert c.dataset["observations"].shape == (E * EL, od) and c.dataset["actions"].shape == (E * EL, ad)
    c2 = tr.collect(0.2, gamma=0.9, seed=3)
    assert tr._collector[1] is col and not np.array_equal(c2.returns, c.returns)
    assert c2.dataset["actions"].data_ptr() != c.dataset["actions"].data_ptr()  # fresh tensors every run


# ------------------------------------------------------------------------------------------------------------------ #
# 2. the table is a trajectory
# ------------------------------------------------------------------------------------------------------------------ #
def step_bounds(env, obs, act, nobs_ref):
    """(b [n, od], reward bound [n], s'.w bound [n]) of the module docstring, in fp64 from the operands."""
    od, ad = env.state_dim, env.action_dim
    A, B = np.abs(env.A.astype(np.float64)), np.abs(env.Bm.astype(np.float64))
    b = (od + ad + 2) * U23 * (np.abs(obs.astype(np.float64)) @ A.T + np.abs(act.astype(np.float64)) @ B.T)
    s2 = nobs_ref.astype(np.float64)
    d = np.abs(s2 - env.goal.astype(np.float64))
    rb = 0.1 * (2 * d * b + b * b).sum(1) + (od + 2) * U23 * (1 + 0.1 * (d * d).sum(1))
    w = np.abs(env.w.astype(np.float64))
    wb = (w * b).sum(1) + (od + 2) * U23 * (np.abs(s2) * w).sum(1)
    return b, rb, wb


@pytest.mark.parametrize("shape", [SMALL, BIG])
def test_table_is_a_trajectory(shape):
    od, ad, E = shape
    m, venv, col = bc_setup(shape)
    c = bc_noisy(shape)
    for k, v in c.dataset.items():
        w = {"observations": (od,), "next_observations": (od,), "actions": (ad,)}.get(k, ())
        assert v.shape == (E * EL,) + w and v.dtype == torch.float32 and v.is_cuda, k
    d = npd(c.dataset)
    t = np.arange(E * EL) % EL
    np.testing.assert_array_equal(d["observations"][t == 0], venv.state0.cpu().numpy())
    np.testing.assert_array_equal(d["next_observations"][t < EL - 1], d["observations"][t > 0])
    assert (d["terminals"] == 0).all()
    np.testing.assert_array_equal(d["timeouts"], (t == EL - 1).astype(np.float32))
    assert (np.abs(d["actions"]) <= 1.0).all() and set(np.unique(d["costs"])) <= {0.0, 1.0}
    env = make_env(od, ad)
    ref_o, ref_r, ref_c, ref_sw = [], [], [], []
    for row in range(E * EL):
        env.s, env.t = d["observations"][row].copy(), 0
        o2, r, _, _, info = env.step(d["actions"][row])
        ref_o.append(o2), ref_r.append(r), ref_c.append(info["cost"])
        ref_sw.append(float(o2.astype(np.float64) @ env.w.astype(np.float64)))
    ref_o, ref_r, ref_c, ref_sw = np.array(ref_o), np.array(ref_r), np.array(ref_c, np.float32), np.array(ref_sw)
    b, rb, wb = step_bounds(env, d["observations"], d["actions"], ref_o)
    eo = np.abs(d["next_observations"].astype(np.float64) - ref_o)
    er = np.abs(d["rewards"].astype(np.float64) - ref_r)
    print(f"{shape}: next_obs worst err / bound {np.max(eo / b):.3f}, reward {np.max(er / rb):.3f}")
    assert (eo <= b).all() and (er <= rb).all()
    clear = np.abs(ref_sw - env.COST_THRESHOLD) > wb
    print(f"{shape}: rows within the bound of the cost threshold: {(~clear).sum()} of {E * EL}; cost rate {d['costs'].mean():.3f}")
    assert (~clear).mean() <= 0.01
    np.testing.assert_array_equal(d["costs"][clear], ref_c[clear])
    assert 0.0 < d["costs"].mean() < 1.0, "the environment must produce both cost values"


# ------------------------------------------------------------------------------------------------------------------ #
# 3. injected noise
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("kind,shape", [("bc", BIG), ("cpq", SMALL)])
def test_injected_noise(kind, shape):
    from osrl_amd.engine.collect import Collector
    od, ad, E = shape
    if kind == "bc":
        m, venv, _ = bc_setup(shape)
    else:
        m, venv = make_model(kind, od, ad), make_venv(od, ad, E)
    col = Collector(m, venv, kind)
    sigma = np.where(np.arange(E) % 2 == 1, 0.3, 0.0).astype(np.float32)
    eps = (np.random.RandomState(2).randn(EL, E, ad) * 3.0).astype(np.float32)
    eps[:, sigma == 0] = np.nan
    det = col.run(0.0)
    c = col.run(sigma, noise=torch.tensor(eps, device=DEV))
    d = npd(c.dataset)
    assert all(np.isfinite(v).all() for v in d.values()) and np.isfinite(c.returns).all()
    pi = oracle_policy(kind, m)(d["observations"]).reshape(E, EL, ad)
    want = pi.copy()
    noisy = sigma != 0
    want[noisy] += sigma[noisy, None, None] * eps.transpose(1, 0, 2)[noisy].astype(np.float64)
    want = np.clip(want, -1.0, 1.0)
    err = np.abs(d["actions"].reshape(E, EL, ad) - want).max()
    print(f"{kind} {shape}: actions vs clip(pi + sigma eps): {err:.2e}; clipped {np.mean(np.abs(want) == 1.0):.3f}")
    assert err <= 1e-4
    assert (np.abs(want[noisy]) == 1.0).any(), "the clip must be exercised"
    for e in np.flatnonzero(~noisy):  # sigma = 0: the deterministic episode, bit for bit, NaN never read
        same_tables(c.dataset, det.dataset, slice(e * EL, (e + 1) * EL))
    for a, b_ in zip(c[1:], det[1:]):
        np.testing.assert_array_equal(a[~noisy], b_[~noisy])
    assert (c.returns[noisy] != det.returns[noisy]).all()
    with pytest.raises(ValueError):
        col.run(0.1, noise=torch.zeros(EL, E, ad + 1, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ #
# 4. Philox noise
# ------------------------------------------------------------------------------------------------------------------ #
def test_philox_noise():
    from osrl_amd.engine.collect import Collector
    od, ad, E = BIG
    m, venv, _ = bc_setup(BIG)
    col = Collector(m, venv, "bc")
    sg = 0.05
    a = col.run(sg, seed=11)
    g0 = col.graph
    b = col.run(sg, seed=11)
    same_tables(a.dataset, b.dataset)
    same_sums(a, b)
    other = col.run(sg, seed=12)
    assert col.graph is g0 and g0 is not None, "a new seed must not need a recapture"
    assert not torch.equal(other.dataset["actions"], a.dataset["actions"])
    again = col.run(sg, seed=11)
    same_tables(a.dataset, again.dataset)
    # keyed by the episode id: the first five episodes do not care how many run beside them
    od5 = Collector(m, make_venv(od, ad, 5), "bc").run(sg, seed=11)
    same_tables(od5.dataset, a.dataset, slice(0, 5 * EL))
    np.testing.assert_array_equal(od5.returns, a.returns[:5])
    # ... and a shifted base seed shifts the keys with it
    sh = Collector(m, make_venv(od, ad, 5, BASE_SEED + 2), "bc").run(sg, seed=11)
    for k in a.dataset:
        assert torch.equal(sh.dataset[k][:3 * EL], a.dataset[k][2 * EL:5 * EL]), k
    d = npd(a.dataset)
    pi = oracle_policy("bc", m)(d["observations"])
    assert np.abs(d["actions"]).max() < 1.0 and np.abs(pi).max() + 6 * sg < 1.0, "the policy must stay inside the clip"
    zn = (d["actions"].astype(np.float64) - pi) / sg  # [E * L, ad] recovered noise rows (within 1e-4 / sigma = 2e-3)
    n = zn.size
    mean, var = zn.mean(), zn.var()
    print(f"philox noise: n = {n}, mean {mean:+.4f} (bound {5 / np.sqrt(n):.4f}), var {var:.4f} "
          f"(bound 1 +- {5 * np.sqrt(2 / n):.4f}), max |z| {np.abs(zn).max():.2f}")
    assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1.0) <= 5 * np.sqrt(2.0 / n)
    dist = np.abs(zn[:, None, :] - zn[None, :, :]).max(-1)
    dist[np.arange(len(zn)), np.arange(len(zn))] = np.inf
    assert dist.min() > 0.02, "two (episode, step) pairs share a noise row"
    # the second Philox block (column 4) is not a copy of a column of the first
    cc = np.corrcoef(zn.T)
    assert np.abs(cc - np.eye(ad)).max() <= 5 / np.sqrt(len(zn))


# ------------------------------------------------------------------------------------------------------------------ #
# 5. discounted sums
# ------------------------------------------------------------------------------------------------------------------ #
def disc_from_rows(d, E, gamma32, key, scale=1.0):
    g = float(np.float32(gamma32)) ** np.arange(EL)
    terms = g[None, :] * d[key].astype(np.float64).reshape(E, EL) * scale
    return terms.sum(1), EL * 2.0 ** -24 * np.abs(terms).sum(1)


@pytest.mark.parametrize("shape", [SMALL, BIG])
def test_discounted_sums(shape):
    od, ad, E = shape
    m, venv, col = bc_setup(shape)
    c = bc_noisy(shape)  # gamma = 0.9, cost_scale = 2
    d = npd(c.dataset)
    for got, key, scale in ((c.disc_returns, "rewards", 1.0), (c.disc_cost_returns, "costs", 2.0)):
        want, bound = disc_from_rows(d, E, 0.9, key, scale)
        print(f"{shape} {key}: worst err / bound {np.max(np.abs(got - want) / np.maximum(bound, 1e-300)):.3f}")
        assert (np.abs(got - want) <= bound).all(), key
    und, ubound = disc_from_rows(d, E, 1.0, "rewards")
    assert (np.abs(c.returns - und) <= ubound).all() and (c.lengths == EL).all()
    np.testing.assert_array_equal(c.cost_returns, 2.0 * d["costs"].reshape(E, EL).sum(1))
    g0 = col.graph
    one = col.run(0.3, gamma=1.0, seed=7)
    np.testing.assert_array_equal(one.disc_returns, one.returns)
    np.testing.assert_array_equal(one.disc_cost_returns, one.cost_returns)
    half = col.run(0.3, gamma=0.5, seed=7)
    assert col.graph is g0 and g0 is not None
    same_tables(half.dataset, c.dataset)  # gamma changes the sums, not the trajectory
    want, bound = disc_from_rows(d, E, 0.5, "rewards")
    assert (np.abs(half.disc_returns - want) <= bound).all()
    assert np.abs(half.disc_returns - c.disc_returns).min() > 1e-3


# ------------------------------------------------------------------------------------------------------------------ #
# 6. nothing is written past the table
# ------------------------------------------------------------------------------------------------------------------ #
def test_guard_rows_survive_the_overshooting_replay():
    from osrl_amd.engine.collect import Collector
    od, ad, E = BIG
    m, venv, _ = bc_setup(BIG)
    col = Collector(m, venv, "bc", seed=4)
    a = col.run(0.3)
    assert col.graph is not None and col.guards_intact()
    b = col.run(0.3)
    assert col.guards_intact()
    same_tables(a.dataset, b.dataset)
    same_sums(a, b)
    for k, t in a.dataset.items():  # the copies handed out do not alias the collector's tables
        assert t.data_ptr() != col.tables[k].data_ptr() and t.is_contiguous()
    col.bufs["rewards"][0] = 0.0  # (the check does see a touched guard row)
    assert not col.guards_intact()


# ------------------------------------------------------------------------------------------------------------------ #
# 7. the stores take it as it is
# ------------------------------------------------------------------------------------------------------------------ #
def test_stores_take_the_dataset_as_it_is():
    from osrl_amd.common.ingest import process_bc_dataset
    from osrl_amd.common.replay import ReplayStore, SequenceStore
    from osrl_amd.engine.collect import merge_datasets
    od, ad, E = 6, 2, 33
    m = make_model("bc", od, ad)
    from osrl_amd.engine.collect import Collector
    col = Collector(m, make_venv(od, ad, E), "bc")
    c = col.run(0.3, seed=1)
    d = c.dataset
    seq = SequenceStore.from_dataset(d, 8, DEV)
    assert seq.n_traj == E and (seq.traj_len == EL).all()
    np.testing.assert_array_equal(seq.traj_start.cpu().numpy(), np.arange(E) * EL)
    rtg0 = seq.ret[seq.traj_start].cpu().numpy().astype(np.float64)
    bound = EL * 2.0 ** -24 * np.abs(d["rewards"].cpu().numpy().astype(np.float64)).reshape(E, EL).sum(1)
    assert (np.abs(rtg0 - c.returns) <= bound).all()
    rs = ReplayStore(d, DEV, state_init=True)
    init = rs.tables[6].reshape(-1).cpu().numpy()
    assert rs.n_rows == E * EL and init.sum() == E and (init[::EL] == 1).all()
    limit = float(np.median(c.cost_returns)) + 0.5  # (between two attainable cost sums: no tie at the threshold)
    safe = process_bc_dataset(d, limit, 1.0, "safe", DEV)
    idx = safe["index"].cpu().numpy()
    kept = np.flatnonzero(c.cost_returns <= limit)
    assert 0 < len(kept) and len(idx) == len(kept) * EL
    np.testing.assert_array_equal(idx.reshape(-1, EL), kept[:, None] * EL + np.arange(EL)[None, :])
    c2 = col.run(0.3, seed=2)
    both = merge_datasets([d, c2.dataset])
    assert all(v.shape[0] == 2 * E * EL for v in both.values())
    assert torch.equal(both["actions"][:E * EL], d["actions"]) and torch.equal(both["actions"][E * EL:], c2.dataset["actions"])
    seq2 = SequenceStore.from_dataset(both, 8, DEV)
    assert seq2.n_traj == 2 * E and (seq2.traj_len == EL).all()
    assert int(ReplayStore(both, DEV, state_init=True).tables[6].sum().item()) == 2 * E


# ------------------------------------------------------------------------------------------------------------------ #
# 8. FQE against the truth
# ------------------------------------------------------------------------------------------------------------------ #
def test_fqe_against_the_truth():
    """Two BC policies (A and its mirror) on the setup of tests/collect_cases.py: each is collected for 256 episodes with
    sigma_e cycling over {0, 0.1, 0.3, 0.5}, the collections are merged, and per policy an FQE (num_q 2, [64, 64]) runs
    4000 replay steps at B = 256 on the merged store.  Its estimate at the store's initial states is held against the
    policy's noise-free mean discounted return from the same initial states.

    (a) precondition: the two true reward values differ by >= 1.0;  (b) FQE ranks them as the truth does, with at least
    half the true gap;  (c) |estimate - truth| <= twice the worst error of the fp64 OracleFQE on the numpy restatement's
    data over three minibatch seeds per policy (tools/collect_fqe_truth.py -> profiles/collect_fqe_truth.json).
    What it shows: the collected tables, their done flags and initial-state marks, the discounted sums and FQE fit
    together and land where an independent fp64 run lands.  What it does not: that FQE is unbiased -- the stores set
    done = timeouts, so the critic mixes full and truncated horizons; gamma^L = 1e-4 keeps that below the bound here."""
    from osrl_amd.algorithms import BC, FQE, FQETrainer
    from osrl_amd.common.replay import ReplayStore
    from osrl_amd.common.synthetic_env import VecSyntheticSafeEnv
    from osrl_amd.engine.collect import Collector, merge_datasets
    ref = json.load(open(os.path.join(ROOT, CC.TRUTH_JSON)))
    venv = VecSyntheticSafeEnv(CC.make_env(), CC.EPISODES, DEV, base_seed=CC.BASE_SEED)
    sigma = CC.sigmas()
    models, truth, data = {}, {}, []
    for name, sd in CC.policies().items():
        m = models[name] = BC(CC.OD, CC.AD, 1.0, CC.POLICY_HIDDEN, CC.EL, device=DEV)
        m.load_state_dict(sd)
        col = Collector(m, venv, "bc")
        det = col.run(0.0, gamma=CC.GAMMA)
        truth[name] = (det.disc_returns.mean(), det.disc_cost_returns.mean())
        data.append(col.run(sigma, gamma=CC.GAMMA, noise=torch.tensor(CC.injected_noise(name), device=DEV)).dataset)
    for name in truth:  # the device's truth is the numpy restatement's
        assert abs(truth[name][0] - ref["truth"][name]["value"]) <= 1e-3
        assert abs(truth[name][1] - ref["truth"][name]["cost_value"]) <= 0.02
    gap = truth["A"][0] - truth["mirror"][0]
    assert abs(gap) >= 1.0, f"precondition (a): true reward values {truth}"
    store = ReplayStore(merge_datasets(data), DEV, state_init=True, seed=1)
    est = {}
    for name, m in models.items():
        torch.manual_seed(11)
        fqe = FQE(m, CC.FQE_HIDDEN, gamma=CC.GAMMA, tau=CC.FQE_TAU, num_q=CC.FQE_NUM_Q, device=DEV)
        tr = FQETrainer(fqe, critic_lr=CC.FQE_LR, stats_mode="none")
        eng = fqe.engine(CC.FQE_BATCH)
        eng.attach_replay(store)
        for _ in range(CC.FQE_STEPS):
            eng.step_replay()
        est[name] = tr.estimate(store)
        assert est[name].n_init == 2 * CC.EPISODES
    rb, cb = 2 * ref["worst_value_error"], 2 * ref["worst_cost_value_error"]
    for name in truth:
        print(f"{name}: truth reward {truth[name][0]:.4f} cost {truth[name][1]:.4f}; FQE {est[name].value:.4f} "
              f"{est[name].cost_value:.4f}; error {abs(est[name].value - truth[name][0]):.4f} (bound {rb:.4f}) "
              f"{abs(est[name].cost_value - truth[name][1]):.4f} (bound {cb:.4f})")
    fgap = est["A"].value - est["mirror"].value
    assert np.sign(fgap) == np.sign(gap) and abs(fgap) >= 0.5 * abs(gap), (fgap, gap)  # (b)
    for name in truth:  # (c)
        assert abs(est[name].value - truth[name][0]) <= rb, (name, est[name], truth[name], rb)
        assert abs(est[name].cost_value - truth[name][1]) <= cb, (name, est[name], truth[name], cb)
