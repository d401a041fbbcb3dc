"""The lockstep act path of the MLP policies (csrc/act_vec.hip ``osrl_policy_*_n``, engine/act.py VecFastPolicy) and its
trainer wiring (``rollout_many``, ``evaluate`` over a list of host environments) for BC, CPQ, BCQ-Lag, BEAR-Lag and
COptiDICE.

Exact checks (no tolerance): no arithmetic in the kernel crosses rows and a dot product's k-order is fixed by the layer
shape, so a slot of an N-wide policy returns, bit for bit, what the 1-wide policy returns for that slot's inputs, at
N = 5, N = 64 and under a random active mask; closed loop, ``rollout_many`` over five environments equals
``rollout_many`` on each of them alone.  Toleranced checks use the gates the project already has: 1e-5 / 1e-4 of
``test_fast_policy_matches_oracle_and_batched_path`` against ``FastPolicy.act``, the numpy oracle and the batched actor;
the closed-loop gate of ``test_batched_evaluate_matches_oracle_rollouts`` against the trainers' own ``rollout()``.

Every model is used after two train steps, so its weights are not the initial ones."""
import numpy as np
import pytest
import torch

from cases import BEARL_CASES, CASES, COPTIDICE_CASES, Case
from gpu_util import build_gpu, gpu_batch, gpu_step
from oracle_util import build_oracle, oracle_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# a small and a wide case per algorithm from tests/cases.py, plus nets with layers past 512 (the 1024-wide instantiation
# of the kernel): a three-layer 1024 BC actor, a CPQ actor with unequal wide layers, a BCQ-Lag pair whose decoder AND
# perturbation net are wide
WIDE = {c.name: c for c in [
    Case("bc_vec_1024", "bc", od=17, ad=6, B=32, hidden=[1024, 1024, 1024], steps=1, seed=81),
    Case("cpq_vec_640", "cpq", od=33, ad=4, B=32, hidden=[640, 576], vae_hidden=64, N=3, steps=1, seed=82,
         max_action=2.0),
    Case("bcql_vec_750", "bcql", od=33, ad=8, B=32, hidden=[750, 750], vae_hidden=600, N=3, steps=1, seed=83),
    # BC in multi-task mode: the actor's input is the observation plus the cost limit (8 + 1)
    Case("bc_vec_mt", "bc", od=9, ad=2, B=32, hidden=[32, 32], steps=1, seed=84),
]}
ALL = {**CASES, **BEARL_CASES, **COPTIDICE_CASES, **WIDE}
NAMES = ["bc_small", "bc_c1", "bc_vec_1024", "cpq_small", "cpq_wide", "cpq_vec_640", "bcql_small", "bcql_wide",
         "bcql_vec_750", "bearl_small", "bearl_wide", "coptidice_small", "coptidice_wide"]
SMALL = ["bc_small", "cpq_small", "bcql_small", "bearl_small", "coptidice_small"]
KIND = {"bc": "mlp", "cpq": "gauss", "bearl": "gauss", "coptidice": "gauss", "bcql": "bcq"}


def _trained(name, steps=2):
    """(case, model, trainer, fp32 oracle, batch) after ``steps`` train steps of both."""
    c = ALL[name]
    m, tr, lg = build_gpu(c)
    o = build_oracle(c)
    b = gpu_batch(c)
    for st in range(steps):
        gpu_step(tr, c, b, st)
        oracle_step(o, c, st)
    return c, m, tr, o, b


def _noise_dim(c):
    return {"mlp": 0, "gauss": c.ad, "bcq": 2 * c.ad}[KIND[c.algo]]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _run(pol, obs, noise, deterministic, active=None, ids=None):
    """Teacher-forced: reset on obs[0], step on obs[1:]; returns actions [T, N, ad] and log-probs [T, N] (or None)."""
    acts, lps = [], []
    for t in range(obs.shape[0]):
        kw = dict(noise=None if noise is None else noise[t], deterministic=deterministic,
                  active=None if active is None else active[t])
        a, lp = pol.reset(obs[t], episode_ids=ids, **kw) if t == 0 else pol.step(obs[t], **kw)
        acts.append(a)
        lps.append(lp)
    return np.stack(acts), (None if lps[0] is None else np.stack(lps))


def _modes(c):
    """(deterministic, explicit noise?) combinations to run: GAUSS both ways, BCQ with explicit z, MLP plain."""
    kind = KIND[c.algo]
    if kind == "gauss":
        return [(True, False), (False, True)]
    return [(True, True)] if kind == "bcq" else [(True, False)]


@pytest.mark.parametrize("name", NAMES)
def test_slot_results_do_not_depend_on_width_slot_or_neighbours(name):
    c, m, tr, o, b = _trained(name)
    T, N = 22, 5
    rs = np.random.RandomState(11)
    nd = _noise_dim(c)
    obs = rs.randn(T, N, c.od).astype(np.float32)
    nz = rs.randn(T, N, max(nd, 1)).astype(np.float32)[:, :, :nd] if nd else None
    p1, p5, p64 = m.fast_policy(num_envs=1), m.fast_policy(num_envs=5), m.fast_policy(num_envs=64)
    assert p5 is m.fast_policy(num_envs=5) and p1 is not p5 and p5.num_envs == 5
    for det, use_noise in _modes(c):
        noise = nz if use_noise else None
        a5, l5 = _run(p5, obs, noise, det)
        assert a5.shape == (T, N, c.ad) and a5.dtype == np.float32 and np.isfinite(a5).all()
        assert (l5 is None) == (KIND[c.algo] != "gauss")
        assert np.unique(_bits(a5[:, :, 0])).size > T * N // 2, "the streams must differ"
        # ---- N = 1 through the same entry points, on each slot's inputs
        for e in range(N):
            a1, l1 = _run(p1, obs[:, e:e + 1], None if noise is None else noise[:, e:e + 1], det)
            np.testing.assert_array_equal(_bits(a1[:, 0]), _bits(a5[:, e]), err_msg=f"{name} slot {e} det={det}")
            if l5 is not None:
                np.testing.assert_array_equal(_bits(l1[:, 0]), _bits(l5[:, e]))
        # ---- N = 64: the five streams scattered over all four row tiles, other streams beside them
        slots = [0, 15, 16, 37, 63]
        obs64 = rs.randn(T, 64, c.od).astype(np.float32) * 3.0
        obs64[:, slots] = obs
        nz64 = None
        if noise is not None:
            nz64 = rs.randn(T, 64, nd).astype(np.float32)
            nz64[:, slots] = noise
        a64, l64 = _run(p64, obs64, nz64, det)
        np.testing.assert_array_equal(_bits(a64[:, slots]), _bits(a5))
        if l5 is not None:
            np.testing.assert_array_equal(_bits(l64[:, slots]), _bits(l5))
        # ---- a random active mask: active slots as before; idle slots' rows of obs / noise are not read (NaN) and
        # their action and log-prob words keep their previous values
        mask = rs.rand(T, N) < 0.6
        mask[0, 0], mask[0, 1] = True, False  # (an idle slot at reset too)
        prev_a, prev_l = a5[-1].copy(), None if l5 is None else l5[-1].copy()  # what the block holds now
        obs_m = np.where(mask[:, :, None], obs, np.nan).astype(np.float32)
        nz_m = None if noise is None else np.where(mask[:, :, None], noise, np.nan).astype(np.float32)
        for t in range(T):
            kw = dict(noise=None if nz_m is None else nz_m[t], deterministic=det, active=mask[t])
            a, lp = p5.reset(obs_m[t], **kw) if t == 0 else p5.step(obs_m[t], **kw)
            want_a = np.where(mask[t][:, None], a5[t], prev_a)
            np.testing.assert_array_equal(_bits(a), _bits(want_a), err_msg=f"{name} masked step {t}")
            if l5 is not None:
                want_l = np.where(mask[t], l5[t], prev_l)
                np.testing.assert_array_equal(_bits(lp), _bits(want_l))
                prev_l = want_l
            prev_a = want_a


@pytest.mark.parametrize("name", ["cpq_small", "bcql_small", "bcql_vec_750", "coptidice_wide"])
def test_device_drawn_noise_follows_the_episode_not_the_slot(name):
    """Noise drawn in the kernel is keyed by (seed, episode id, step): episode q gives the same actions in a 1-wide
    policy and in slot 3 of a 5-wide one, two ids differ, two runs agree."""
    c, m, tr, o, b = _trained(name)
    T, q = 20, 41
    rs = np.random.RandomState(12)
    stream = rs.randn(T, c.od).astype(np.float32)
    p1, p5 = m.fast_policy(num_envs=1), m.fast_policy(num_envs=5)
    det = KIND[c.algo] == "bcq"  # BCQ-Lag draws z whatever the flag says; GAUSS draws eps when stochastic
    _run(p1, stream[:3, None], None, det, ids=np.array([7]))  # earlier calls on the handle must not matter
    a1, l1 = _run(p1, stream[:, None], None, det, ids=np.array([q]))
    obs5 = np.repeat(stream[:, None], 5, axis=1)  # the same observations in every slot: only the ids differ
    ids = np.array([3, q + 1, 9, q, q])
    a5, l5 = _run(p5, obs5, None, det, ids=ids)
    np.testing.assert_array_equal(_bits(a5[:, 3]), _bits(a1[:, 0]))
    np.testing.assert_array_equal(_bits(a5[:, 4]), _bits(a1[:, 0]))  # the same id in another slot
    if l1 is not None:
        np.testing.assert_array_equal(_bits(l5[:, 3]), _bits(l1[:, 0]))
    assert (a5[:, 2] != a5[:, 3]).any() and (a5[:, 1] != a5[:, 3]).any(), "two episode ids must draw different noise"
    assert (a5[1:, 3] != a5[:-1, 3]).any()
    again, _ = _run(p5, obs5, None, det, ids=ids)
    np.testing.assert_array_equal(_bits(again), _bits(a5))
    # the step within the episode is part of the key: an idle call does not advance it
    act = np.ones((T, 5), bool)
    act[5, 3] = False
    shifted = obs5.copy()
    shifted[6:, 3] = obs5[5:-1, 3]  # slot 3 sees stream[5] one call later
    a_m, _ = _run(p5, shifted, None, det, active=act, ids=ids)
    np.testing.assert_array_equal(_bits(a_m[6:, 3]), _bits(a5[5:-1, 3]))


@pytest.mark.parametrize("name", NAMES)
def test_matches_fast_policy_oracle_and_batched_actor(name):
    """Gates of test_fast_policy_matches_oracle_and_batched_path: actions within 1e-5 of FastPolicy.act and of the
    numpy oracle, GAUSS log-probs within 1e-4 of the batched model.actor path."""
    c, m, tr, o, b = _trained(name)
    N = 5
    rs = np.random.RandomState(13)
    obs = rs.randn(N, c.od).astype(np.float32)
    pol, fp = m.fast_policy(num_envs=N), m.fast_policy()
    assert type(fp).__name__ == "FastPolicy"  # num_envs=None: today's object
    kind = KIND[c.algo]
    if kind == "mlp":
        got, lp = pol.reset(obs)
        assert lp is None
        want = o.act(obs)
        old = np.concatenate([fp.act(obs[:4])[0], fp.act(obs[4:])[0]])
    elif kind == "bcq":
        z = rs.randn(N, 2 * c.ad).astype(np.float32)  # includes |z| > 0.5: the clamp is exercised
        assert (np.abs(z) > 0.5).any()
        got, lp = pol.reset(obs, noise=z)
        want = np.stack([o.act(obs[i][None], z[i][None])[0] for i in range(N)])
        old = np.concatenate([fp.act(obs[:4], True, noise=z[:4])[0], fp.act(obs[4:], True, noise=z[4:])[0]])
    else:
        got, lp = pol.reset(obs)
        want = np.stack([o.act(obs[i][None])[0] for i in range(N)])
        old = np.concatenate([fp.act(obs[:4], True)[0], fp.act(obs[4:], True)[0]])
        t = lambda a: torch.tensor(a, device=DEV)  # noqa: E731
        scale = 1.0 if c.algo == "coptidice" else c.max_action
        lp_det = m.actor(t(obs), True, True)[1].cpu().numpy()
        print(f"{name}: det logp err {np.abs(lp - lp_det).max():.3e}")
        assert np.abs(lp - lp_det).max() <= 1e-4
        eps = rs.randn(N, c.ad).astype(np.float32)
        ab, lpb = m.actor(t(obs), False, True, eps=t(eps))
        an, lpn = pol.step(obs, noise=eps, deterministic=False)
        an_old, lpn_old = fp.act(obs[:4], False, noise=eps[:4])
        print(f"{name}: stochastic act err {np.abs(an - ab.cpu().numpy() * scale).max():.3e} "
              f"logp err {np.abs(lpn - lpb.cpu().numpy()).max():.3e}")
        assert np.abs(an - ab.cpu().numpy() * scale).max() <= 1e-5
        assert np.abs(lpn - lpb.cpu().numpy()).max() <= 1e-4
        assert np.abs(an[:4] - an_old).max() <= 1e-5 and np.abs(lpn[:4] - lpn_old).max() <= 1e-4
    print(f"{name}: act err vs oracle {np.abs(got - want).max():.3e} vs FastPolicy {np.abs(got - old).max():.3e}")
    assert got.shape == (N, c.ad) and np.abs(got - want).max() <= 1e-5 and np.abs(got - old).max() <= 1e-5


@pytest.mark.parametrize("name", ["bc_small", "cpq_wide", "bcql_vec_750", "bearl_small", "coptidice_small"])
def test_same_policy_object_follows_the_parameters(name):
    c, m, tr, o, b = _trained(name)
    N = 5
    rs = np.random.RandomState(14)
    obs = rs.randn(N, c.od).astype(np.float32)
    z = rs.randn(N, 2 * c.ad).astype(np.float32)

    def want(orc):
        if c.algo == "bc":
            return orc.act(obs)
        if c.algo == "bcql":
            return np.stack([orc.act(obs[i][None], z[i][None])[0] for i in range(N)])
        return np.stack([orc.act(obs[i][None])[0] for i in range(N)])

    pol = m.fast_policy(num_envs=N)
    kw = dict(noise=z) if c.algo == "bcql" else {}
    a0, _ = pol.reset(obs, **kw)
    assert np.abs(a0 - want(o)).max() <= 1e-5
    for st in range(2, 5):  # further train steps
        gpu_step(tr, c, b, st)
        oracle_step(o, c, st)
    assert m.fast_policy(num_envs=N) is pol
    a1, _ = pol.step(obs, **kw)
    assert (a1 != a0).any() and np.abs(a1 - want(o)).max() <= 1e-5
    from cases import make_params
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_params(c).items()})
    a2, _ = pol.step(obs, **kw)
    assert m.fast_policy(num_envs=N) is pol
    assert (a2 != a1).any() and np.abs(a2 - want(build_oracle(c))).max() <= 1e-5


# ---- closed loop -------------------------------------------------------------------------------------------------------
def _env(od, ad, seed, episode_len=50):
    """A host SyntheticSafeEnv whose every ``reset()`` starts at its own noisy initial state (init_noise = 0.7, drawn
    from the environment's seed): what the trainers' ``rollout()`` sees is a plain gym-style environment."""
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv

    class Env(SyntheticSafeEnv):
        def reset(self, seed=None):
            return super().reset(seed=1000 + env_seed)

    env_seed = seed
    return Env(od, ad, episode_len, seed=seed, init_noise=0.7)


def _closed_loop_setup(name):
    """(case, trainer, oracle, env observation width): the named case, BC in multi-task mode for ``bc_vec_mt``."""
    c, m, tr, o, b = _trained(name)
    env_od = c.od
    if name == "bc_vec_mt":
        tr.bc_mode, tr.cost_limit, env_od = "multi-task", 20, c.od - 1
    return c, m, tr, o, env_od


@pytest.mark.parametrize("name", SMALL + ["bc_vec_mt", "cpq_vec_640"])
def test_rollout_many_equals_each_environment_alone(name):
    c, m, tr, o, env_od = _closed_loop_setup(name)
    m.episode_len = 30
    specs = [(21, 50), (22, 17), (23, 29), (24, 50), (25, 8)]  # (seed, the environment's own length): slots end apart
    make = lambda: [_env(env_od, c.ad, s, el) for s, el in specs]  # noqa: E731
    ids = np.array([40, 41, 42, 43, 44])
    r5, l5, c5 = tr.rollout_many(make(), episode_ids=ids)
    np.testing.assert_array_equal(l5, [30, 17, 29, 30, 8])
    assert np.unique(r5).size == 5 and c5.sum() > 0
    r8, l8, c8 = tr.rollout_many(make(), num_slots=8, episode_ids=ids)  # idle slots change nothing
    for x, y in ((r5, r8), (l5, l8), (c5, c8)):
        np.testing.assert_array_equal(x, y)
    for e, env in enumerate(make()):
        r1, l1, c1 = tr.rollout_many([env], num_slots=1, episode_ids=ids[e:e + 1])
        assert (r1[0], l1[0], c1[0]) == (r5[e], l5[e], c5[e]), (name, e)
    if c.algo == "bcql":  # the episode id is the noise key: another id, another episode
        r_other, _, _ = tr.rollout_many(make(), episode_ids=ids + 100)
        assert (r_other != r5).all()


# Environment seeds of the comparison against rollout().  The cost is an indicator at a threshold, so an episode whose
# state passes within rounding of the threshold can flip a cost between two correct fp32 policies; the gate allows that
# in <= 10 % of the episodes, and these seeds are chosen so that the inputs do not use the allowance up: for each of
# them, and each case below, the case's oracle policy (after the two train steps) evaluated in fp32 and the same
# parameters evaluated in fp64 give identical cost sequences and lengths over the episode on the CPU.  Seeds 50 .. 69 were
# screened that way with ``_screen`` below and all twenty passed for every case; the first ten are used.  The test re-runs the screen on the
# seeds it uses (it costs a few hundred small numpy forwards) and fails if a seed no longer qualifies.
ROLLOUT_SEEDS = [50, 51, 52, 53, 54, 55, 56, 57, 58, 59]
PARENT_CASES = ["bc_small", "cpq_small", "bearl_small", "coptidice_small", "bc_vec_mt", "cpq_wide"]


def _oracle_policy(c, o, dtype, append=None):
    """``obs -> action`` of oracle ``o``'s parameters evaluated in ``dtype``."""
    o2 = build_oracle(c, dtype)
    for k, v in o.p.items():
        o2.p[k][...] = v
    if c.algo == "bc":
        return lambda ob: o2.act(np.append(ob, append)[None] if append is not None else ob[None])[0]
    return lambda ob: o2.act(ob[None])[0]


def _screen(c, o, env_od, seed, EL, append=None):
    """True when the fp32 and the fp64 evaluation of the oracle's policy see the same costs on environment ``seed``."""
    out = []
    for dtype in (np.float32, np.float64):
        pol, env = _oracle_policy(c, o, dtype, append), _env(env_od, c.ad, seed, 1000)
        ob, _ = env.reset()
        costs = []
        for _ in range(EL):
            ob, r, term, trunc, info = env.step(np.asarray(pol(ob), np.float32))
            costs.append(info["cost"])
            if term or trunc:
                break
        out.append(costs)
    return out[0] == out[1]


@pytest.mark.parametrize("name", PARENT_CASES)
def test_rollout_many_matches_the_trainers_own_rollout(name):
    """Against ``rollout()`` (one act1 call per step) on equally seeded environments, at the closed-loop gate of
    test_batched_evaluate_matches_oracle_rollouts: equal lengths, returns within rtol 1e-4 / atol 1e-3, cost sums off by
    <= 1.0 in <= 10 % of the episodes.  BCQ-Lag is not in this list: its ``rollout()`` draws z keyed by the handle's call
    counter and the lockstep path, by design, by (episode id, step), so the two see different noise; its kernel is tied
    to ``FastPolicy.act`` with explicit z in test_matches_fast_policy_oracle_and_batched_actor instead."""
    c, m, tr, o, env_od = _closed_loop_setup(name)
    EL = m.episode_len = 40
    append = 20 if name == "bc_vec_mt" else None
    for s in ROLLOUT_SEEDS:
        assert _screen(c, o, env_od, s, EL, append), f"seed {s} no longer qualifies for {name}: pick another"
    envs = [_env(env_od, c.ad, s, 1000) for s in ROLLOUT_SEEDS]
    rets, lens, costs = tr.rollout_many(envs)
    ref = []
    for s in ROLLOUT_SEEDS:
        tr.env = _env(env_od, c.ad, s, 1000)
        ref.append(tr.rollout())
    tr.env = None
    ref = np.array(ref, dtype=np.float64)  # (return, length, cost sum)
    print(f"{name}: max |return diff| {np.abs(rets - ref[:, 0]).max():.3e}, cost sums differing "
          f"{(costs != ref[:, 2]).sum()} of {len(ROLLOUT_SEEDS)}, max cost diff {np.abs(costs - ref[:, 2]).max()}")
    np.testing.assert_array_equal(lens, ref[:, 1])
    assert (lens == EL).all()
    np.testing.assert_allclose(rets, ref[:, 0], rtol=1e-4, atol=1e-3)
    assert np.abs(costs - ref[:, 2]).max() <= 1.0 and (costs != ref[:, 2]).mean() <= 0.1  # indicator at a threshold
    assert np.unique(np.round(rets, 3)).size > len(ROLLOUT_SEEDS) // 2, "episodes must differ"


@pytest.mark.parametrize("name", SMALL + ["bc_vec_mt"])
def test_evaluate_over_a_list_equals_its_waves(name):
    c, m, tr, o, env_od = _closed_loop_setup(name)
    m.episode_len = 25
    rs_, cs_ = 1.0, 1.0
    if c.algo != "bc":
        rs_, cs_ = 2.0, 3.0
        tr.reward_scale, tr.cost_scale = rs_, cs_
    specs = [(31, 50), (32, 12), (33, 19)]
    make = lambda: [_env(env_od, c.ad, s, el) for s, el in specs]  # noqa: E731
    tr.env = make()
    m.train()
    got = tr.evaluate(7)
    assert m.training
    envs = make()
    waves = [tr.rollout_many(envs[:k], num_slots=3, episode_ids=np.arange(q0, q0 + k))
             for q0, k in ((0, 3), (3, 3), (6, 1))]
    r = np.concatenate([w[0] for w in waves])
    l = np.concatenate([w[1] for w in waves])
    cc = np.concatenate([w[2] for w in waves])
    assert r.shape == (7,)
    assert got == (np.mean(r) / rs_, np.mean(cc) / cs_, np.mean(l))
    if c.algo != "bcql":  # deterministic policies: waves repeat, so the means are those of 3 + 3 + 1 episodes
        np.testing.assert_array_equal(r[:3], r[3:6])
    else:
        assert (r[:3] != r[3:6]).all()  # a new episode id, new noise
    tr.env = tuple(make())
    assert tr.evaluate(7) == got
    tr.env = []
    with pytest.raises(ValueError, match="empty"):
        tr.evaluate(3)


@pytest.mark.parametrize("name", SMALL)
def test_single_environment_evaluate_is_the_plain_rollout_loop(name):
    def fresh():
        c, m, tr, o, env_od = _closed_loop_setup(name)
        m.episode_len = 20
        tr.env = _env(env_od, c.ad, 35, 1000)
        return c, m, tr

    c, m, tr = fresh()
    got = tr.evaluate(3)
    assert not m.__dict__.get("_fast_vec"), "one environment must not build a lockstep policy"
    if c.algo == "bcql":  # z is keyed by the handle's call counter: replay on an equal model built anew
        c, m, tr = fresh()
    eps = [tr.rollout() for _ in range(3)]
    want = (np.mean([e[0] for e in eps]), np.mean([e[2] for e in eps]), np.mean([e[1] for e in eps]))
    assert got == want and got[2] == 20
