"""The lockstep form of the CDT act latency path (csrc/cdt_act.hip ``osrl_cdt_policy_*_n``, engine/cdt_act.py
CDTVecFastPolicy): every slot of an N-episode handle returns, bit for bit, what a one-episode CDTFastPolicy returns for
that slot's inputs (no arithmetic in the kernels crosses rows, so this is exact, not a tolerance), at N = 5 (row tiles
straddle episodes), N = 1, N = 64 and at the domain's edge; one slot is also tied to CDT.forward (2e-5) and to the fp64
oracle (5e-5) directly.  Then the trainer wiring (rollout_many, evaluate over a list of environments,
evaluate_targets), weight freshness, handle behaviour and run-to-run determinism."""
import ctypes as C

import numpy as np
import pytest
import torch

from cases import CDT_CASES
from test_gpu_cdt_act import RefLoop, _c5, _oracle, _train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _traj(m, n_steps, seed):
    """A teacher-forced trajectory on a host SyntheticSafeEnv: the first observation and, per step, the taken action,
    the next observation, the reward and the (scaled) cost."""
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    env = SyntheticSafeEnv(m.state_dim, m.action_dim, n_steps + 1, seed=seed)
    rs = np.random.RandomState(100 + seed)
    obs0, _ = env.reset()
    steps = []
    for _ in range(n_steps):
        taken = np.clip(rs.randn(m.action_dim), -1, 1).astype(np.float32)
        obs, reward, _, _, info = env.step(taken)
        steps.append((taken, obs, reward, info["cost"] * 2.0))
    return obs0, steps


def _single(m, traj, tr, tc, n_steps, with_window=True):
    """Actions (and windows) of the one-episode policy along a trajectory."""
    pol = m.fast_policy()
    obs0, steps = traj
    acts, wins = [pol.reset(obs0, tr, tc)], []
    for s in range(n_steps):
        if with_window:
            wins.append(pol.window())
        if s + 1 < n_steps:
            taken, obs, reward, cost = steps[s]
            acts.append(pol.step(obs, reward, cost, action=taken))
    return acts, wins


def _targets(N):
    return [30.0 - 3.5 * e for e in range(N)], [5.0 + 1.25 * e for e in range(N)]


def _check_vec_vs_single(m, N, n_steps, check_steps=None, seed0=10, window_slots=None):
    trs, tcs = _targets(N)
    trajs = [_traj(m, n_steps, seed0 + e) for e in range(N)]
    check = set(range(n_steps)) if check_steps is None else set(check_steps)
    wslots = range(N) if window_slots is None else window_slots
    refs = [_single(m, trajs[e], trs[e], tcs[e], n_steps, with_window=e in wslots) for e in range(N)]
    pol = m.fast_policy(num_envs=N)
    assert m.fast_policy(num_envs=N) is pol
    act = pol.reset(np.stack([t[0] for t in trajs]), trs, tcs)
    assert act.shape == (N, m.action_dim) and act.dtype == np.float32
    for s in range(n_steps):
        if s in check:
            for e in range(N):
                np.testing.assert_array_equal(act[e], refs[e][0][s], err_msg=f"action of slot {e} at step {s}")
            for e in wslots:
                w, wr = pol.window(e), refs[e][1][s]
                for k in wr:
                    np.testing.assert_array_equal(w[k], wr[k], err_msg=f"window {k} of slot {e} at step {s}")
        if s + 1 < n_steps:
            st = [t[1][s] for t in trajs]
            act = pol.step(np.stack([x[1] for x in st]), np.array([x[2] for x in st]), np.array([x[3] for x in st]),
                           action=np.stack([x[0] for x in st]))


@pytest.mark.parametrize("name", list(CDT_CASES))
def test_five_slots_equal_five_single_episodes(name):
    from test_gpu_cdt import build_cdt_gpu
    c = CDT_CASES[name]
    m, _, _ = build_cdt_gpu(c)
    m.eval()
    n = 3 * c.T + 2
    m.episode_len = max(m.episode_len, n)
    _check_vec_vs_single(m, 5, n)


def test_five_slots_equal_five_single_episodes_c5():
    m = _c5()
    _train(m, 2)
    m.eval()
    _check_vec_vs_single(m, 5, 3 * m.seq_len + 2)


def test_a_slot_against_forward_and_oracle():
    """The existing file's two gates (CDT.forward 2e-5, fp64 oracle 5e-5), on slot 3 of a 5-slot policy directly."""
    from test_gpu_cdt import build_cdt_gpu
    c = CDT_CASES["cdt_mid"]
    m, _, _ = build_cdt_gpu(c)
    m.eval()
    N, e, n = 5, 3, 3 * c.T + 2
    o = _oracle(m, c)
    trs, tcs = _targets(N)
    trajs = [_traj(m, n, 20 + i) for i in range(N)]
    pol = m.fast_policy(num_envs=N)
    act = pol.reset(np.stack([t[0] for t in trajs]), trs, tcs)
    ref = RefLoop(m, trajs[e][0], trs[e], tcs[e])
    for s in range(n):
        w, wr = pol.window(e), ref.window(s)
        for k in wr:
            np.testing.assert_array_equal(w[k], wr[k], err_msg=f"window {k} at step {s}")
        af, ao = ref.act(s), ref.oracle_act(o, s)
        assert float(np.abs(act[e] - af).max()) <= 2e-5, (s, act[e], af)
        assert float(np.abs(act[e] - ao).max()) <= 5e-5, (s, act[e], ao)
        taken, obs, reward, cost = trajs[e][1][s]
        ref.push(s, taken, obs, reward, cost)
        if s + 1 < n:
            st = [t[1][s] for t in trajs]
            act = pol.step(np.stack([x[1] for x in st]), np.array([x[2] for x in st]), np.array([x[3] for x in st]),
                           action=np.stack([x[0] for x in st]))


def test_one_slot_through_the_n_entry_points():
    from test_gpu_cdt import build_cdt_gpu
    for name in ("cdt_small", "cdt_v_prefix_det"):
        c = CDT_CASES[name]
        m, _, _ = build_cdt_gpu(c)
        m.eval()
        m.episode_len = 3 * c.T + 2
        _check_vec_vs_single(m, 1, 3 * c.T + 2)


def test_sixty_four_slots_small_shape():
    from test_gpu_cdt import build_cdt_gpu
    c = CDT_CASES["cdt_small"]
    m, _, _ = build_cdt_gpu(c)
    m.eval()
    m.episode_len = 2 * c.T + 2
    _check_vec_vs_single(m, 64, 2 * c.T + 2, check_steps=(0, c.T - 1, c.T, c.T + 1, 2 * c.T + 1), window_slots=(0, 63))


def test_three_slots_at_the_domain_edge():
    from osrl_amd.algorithms import CDT
    torch.manual_seed(1)
    m = CDT(6, 2, 1.0, seq_len=64, episode_len=200, embedding_dim=512, num_layers=1, num_heads=4, use_rew=True,
            use_cost=True, stochastic=False, device=DEV)
    assert m.seq_repeat * m.seq_len == 256
    m.eval()
    T = m.seq_len
    _check_vec_vs_single(m, 3, T + 3, check_steps=(0, T - 1, T, T + 1, T + 2), window_slots=(1,))


# ---- the trainer ----------------------------------------------------------------------------------------------------
def _envs(m, specs):
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    return [SyntheticSafeEnv(m.state_dim, m.action_dim, el, seed=seed) for seed, el in specs]


def _trainer(m, env, **kw):
    from osrl_amd.algorithms import CDTTrainer
    from osrl_amd.common.logger import DummyLogger
    return CDTTrainer(m, env, DummyLogger(), use_graph=False, cost_scale=2.0, reward_scale=0.5, **kw)


def _mid(EL=40):
    from test_gpu_cdt import build_cdt_gpu
    m, _, _ = build_cdt_gpu(CDT_CASES["cdt_mid"])
    m.eval()
    m.episode_len = EL
    return m


def test_rollout_many_equals_single_rollouts():
    m = _mid(40)
    specs = [(31, 40), (32, 17), (33, 29), (34, 50)]  # (seed, the environment's own episode_len): slots end apart
    trs, tcs = [30.0, 20.0, 10.0, 25.0], [5.0, 2.0, 8.0, 1.0]
    tr = _trainer(m, None)
    want = [tr.rollout(m, env, trs[e], tcs[e]) for e, env in enumerate(_envs(m, specs))]
    assert [w[1] for w in want] == [40, 17, 29, 40]
    r, l, c = tr.rollout_many(m, _envs(m, specs), trs, tcs)
    assert m.__dict__["_fast_vec"][4] is not None
    np.testing.assert_array_equal(r, np.asarray([w[0] for w in want]))
    np.testing.assert_array_equal(l, np.asarray([w[1] for w in want]))
    np.testing.assert_array_equal(c, np.asarray([w[2] for w in want]))
    # scalar targets serve every environment
    r2, _, _ = tr.rollout_many(m, _envs(m, specs), 30.0, 5.0)
    assert r2[0] == want[0][0] and r2.shape == (4,)


def _single_jobs(m, tr, specs, jobs):
    """Job q alone on a fresh copy of environment q % N, in the order the environment sees its jobs."""
    envs, N = _envs(m, specs), len(specs)
    return [tr.rollout(m, envs[q % N], t[0], t[1]) for q, t in enumerate(jobs)]


def test_evaluate_over_a_list_of_environments():
    m = _mid(30)
    specs = [(41, 30), (42, 12), (43, 30)]
    tr = _trainer(m, _envs(m, specs))
    ret, cost, ln = tr.evaluate(7, 30.0, 5.0)  # waves of 3, 3 and 1
    assert m.training  # evaluate() leaves the model as the single-environment form does
    m.eval()
    want = _single_jobs(m, _trainer(m, None), specs, [(30.0, 5.0)] * 7)
    assert ret == np.mean([w[0] for w in want]) / 0.5
    assert cost == np.mean([w[2] for w in want]) / 2.0
    assert ln == np.mean([w[1] for w in want])
    assert list(m.__dict__["_fast_vec"]) == [3]  # the partial wave ran on the same 3-slot handle


def test_evaluate_targets_shares_waves_between_targets():
    m = _mid(25)
    specs = [(51, 25), (52, 25), (53, 9), (54, 25)]
    targets = [(30.0, 5.0), (20.0, 2.0), (10.0, 8.0)]
    K = 3  # 9 jobs on 4 environments: target 0's third job shares wave 0 with target 1's first, ...
    got = _trainer(m, tuple(_envs(m, specs))).evaluate_targets(K, targets)
    m.eval()
    jobs = [t for t in targets for _ in range(K)]
    want = _single_jobs(m, _trainer(m, None), specs, jobs)
    assert len(got) == 3
    for i in range(3):
        w = want[i * K:(i + 1) * K]
        assert got[i] == (np.mean([x[0] for x in w]) / 0.5, np.mean([x[2] for x in w]) / 2.0,
                          np.mean([x[1] for x in w])), i
    # a single host environment: evaluate once per target
    one = _trainer(m, _envs(m, specs[:1])[0])
    res = one.evaluate_targets(2, targets[:2])
    m.eval()
    ref = _trainer(m, _envs(m, specs[:1])[0])
    exp = []
    for t in targets[:2]:
        exp.append(ref.evaluate(2, *t))
    assert res == exp


def test_fallbacks_outside_the_domain_and_with_dropout():
    from test_gpu_cdt import build_cdt_gpu
    from osrl_amd.algorithms import CDT
    m = CDT(5, 2, 1.0, episode_len=8, num_layers=1, use_rew=True, use_cost=True, device=DEV, seq_len=10,
            embedding_dim=640, num_heads=8)
    with pytest.raises(NotImplementedError, match="embedding_dim 640"):
        m.fast_policy(num_envs=3)
    specs = [(61, 8), (62, 5), (63, 8)]
    tr = _trainer(m, _envs(m, specs))
    r, l, c = tr.rollout_many(m, _envs(m, specs), [10.0, 9.0, 8.0], 2.0)
    assert list(l) == [8, 5, 8] and np.isfinite(r).all() and np.isfinite(c).all()
    res = tr.evaluate_targets(2, [(10.0, 2.0), (5.0, 1.0)])
    assert len(res) == 2 and all(np.isfinite(x) for t in res for x in t)
    assert not m.__dict__.get("_fast_vec")
    md, _, _ = build_cdt_gpu(CDT_CASES["cdt_drop"])
    md.train()
    md.episode_len = 6
    assert not md.fast_eligible()
    r, l, c = _trainer(md, None).rollout_many(md, _envs(md, [(64, 6), (65, 6)]), 10.0, 2.0)
    assert list(l) == [6, 6] and np.isfinite(r).all() and not md.__dict__.get("_fast_vec")


def test_weights_stay_fresh(tmp_path):
    from osrl_amd.common.checkpoint import load_checkpoint, save_checkpoint
    m = _c5(seq_len=10, embedding_dim=128)
    _train(m, 1)
    m.episode_len = 30
    save_checkpoint(m, str(tmp_path / "a.pt"))

    def check(seed):
        was = m.training
        m.eval()
        _check_vec_vs_single(m, 3, 14, seed0=seed, window_slots=())
        # and the one-episode policy is itself tied to the current weights through CDT.forward
        obs0, _ = _traj(m, 1, seed)
        a = m.fast_policy(num_envs=3).reset(np.stack([obs0] * 3), 30.0, 5.0)
        assert float(np.abs(a[2] - RefLoop(m, obs0, 30.0, 5.0).act(0)).max()) <= 2e-5
        if was:
            m.train()

    check(70)
    _train(m, 3, seed=1)
    check(71)
    load_checkpoint(m, str(tmp_path / "a.pt"))
    check(72)


def test_handles_interleaved_reset_and_limits():
    from test_gpu_cdt import build_cdt_gpu
    from osrl_amd import _lib as L
    from osrl_amd.engine.cdt_act import _descriptor
    c1, c2 = CDT_CASES["cdt_small"], CDT_CASES["cdt_v_prefix_det"]
    (m1, _, _), (m2, _, _) = build_cdt_gpu(c1), build_cdt_gpu(c2)
    m1.eval()
    m2.eval()
    n = 2 * c1.T + 1
    m1.episode_len = m2.episode_len = n + 4
    N1, N2 = 3, 2
    t1, t2 = [_traj(m1, n, 80 + e) for e in range(N1)], [_traj(m2, n, 90 + e) for e in range(N2)]
    (tr1, tc1), (tr2, tc2) = _targets(N1), _targets(N2)
    ref1 = [_single(m1, t1[e], tr1[e], tc1[e], n, False)[0] for e in range(N1)]
    ref2 = [_single(m2, t2[e], tr2[e], tc2[e], n, False)[0] for e in range(N2)]
    p1, p2 = m1.fast_policy(num_envs=N1), m2.fast_policy(num_envs=N2)
    assert m1.fast_policy() is not p1 and m1.fast_policy(num_envs=2) is not p1
    with pytest.raises(RuntimeError, match="reset"):
        p1.step(np.zeros((N1, c1.od)), np.zeros(N1), np.zeros(N1))
    a1 = p1.reset(np.stack([t[0] for t in t1]), tr1, tc1)
    a2 = p2.reset(np.stack([t[0] for t in t2]), tr2, tc2)
    for s in range(n):
        for e in range(N1):
            np.testing.assert_array_equal(a1[e], ref1[e][s])
        for e in range(N2):
            np.testing.assert_array_equal(a2[e], ref2[e][s])
        if s + 1 < n:
            st1, st2 = [t[1][s] for t in t1], [t[1][s] for t in t2]
            a1 = p1.step(np.stack([x[1] for x in st1]), np.array([x[2] for x in st1]), np.array([x[3] for x in st1]),
                         action=np.stack([x[0] for x in st1]))
            a2 = p2.step(np.stack([x[1] for x in st2]), np.array([x[2] for x in st2]), np.array([x[3] for x in st2]),
                         action=np.stack([x[0] for x in st2]))
    # a reset in mid-episode starts all slots over at timestep 0
    a1 = p1.reset(np.stack([t[0] for t in t1]), tr1, tc1)
    for e in range(N1):
        np.testing.assert_array_equal(a1[e], ref1[e][0])
    assert len(p1.window(1)["returns"]) == 1
    # inactive slots: their rows are not read, their result rows are zero, the others are unaffected
    st1 = [t[1][0] for t in t1]
    obs = np.stack([x[1] for x in st1])
    obs[1] = np.nan
    act = p1.step(obs, np.array([x[2] for x in st1]), np.array([x[3] for x in st1]),
                  action=np.stack([x[0] for x in st1]), active=np.array([True, False, True]))
    np.testing.assert_array_equal(act[0], ref1[0][1])
    np.testing.assert_array_equal(act[2], ref1[2][1])
    assert (act[1] == 0).all()
    # the episode ends after episode_len actions (read at reset)
    m2.episode_len = 5
    o2 = np.stack([t[0] for t in t2])
    p2.reset(o2, 10.0, 4.0)
    for _ in range(4):
        p2.step(o2, np.full(N2, 0.5), np.zeros(N2))
    with pytest.raises(RuntimeError, match="episode is over"):
        p2.step(o2, np.full(N2, 0.5), np.zeros(N2))
    # the C call refuses n_env outside 1 .. 64; the one-episode calls refuse a wider handle
    lib = L.load()
    d, layers = _descriptor(m1)
    for bad in (0, 65, -1):
        h = C.c_void_p()
        assert lib.osrl_cdt_policy_create_n(C.byref(d), layers, bad, C.byref(h)) == -1 and not h.value
    assert lib.osrl_cdt_policy_reset(p1._h, 1.0, 1.0, p1._stream()) == -1
    assert lib.osrl_cdt_policy_step(p1._h, 0.0, 0.0, 0, p1._stream()) == -1
    n_out = C.c_int32(-1)
    assert lib.osrl_cdt_policy_window_n(p1._h, N1, None, None, None, None, None, C.byref(n_out), p1._stream()) == -1
    with pytest.raises(ValueError, match="1 .. 64"):
        m1.fast_policy(num_envs=65)


def test_two_runs_give_identical_bytes():
    m = _c5(seq_len=8, embedding_dim=128)
    m.eval()
    N, n = 16, 3 * m.seq_len
    trs, tcs = _targets(N)
    trajs = [_traj(m, n, 110 + e) for e in range(N)]
    pol = m.fast_policy(num_envs=N)
    runs = []
    for _ in range(2):
        out = [pol.reset(np.stack([t[0] for t in trajs]), trs, tcs)]
        for s in range(n - 1):
            st = [t[1][s] for t in trajs]
            out.append(pol.step(np.stack([x[1] for x in st]), np.array([x[2] for x in st]),
                                np.array([x[3] for x in st])))  # the returned actions feed back, on the device
        runs.append(np.stack(out).tobytes())
    assert runs[0] == runs[1]
    assert np.isfinite(np.frombuffer(runs[0], np.float32)).all()
