"""The CDT act latency path (csrc/cdt_act.hip, engine/cdt_act.py CDTFastPolicy) against the existing rollout loop's
torch expressions (window, bit for bit), the fp64 numpy oracle and CDT.forward (actions), plus the trainer wiring
(CDTTrainer(fast_rollout=...)), weight freshness after training / checkpoints, and handle behaviour."""
import numpy as np
import pytest
import torch

from cases import CDT_CASES, make_cdt_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _oracle(m, c=None, dtype=np.float64):
    from oracle.cdt_oracle import OracleCDT
    params = make_cdt_params(c) if c is not None else {k: v.cpu().numpy() for k, v in m.state_dict().items()}
    return OracleCDT(params, seq_len=m.seq_len, num_heads=m.num_heads, num_layers=m.num_layers,
                     cost_transform=m.cost_transform_on, stochastic=m.stochastic, time_emb=m.time_emb,
                     use_rew=m.use_rew, use_cost=m.use_cost, add_cost_feat=m.add_cost_feat,
                     mul_cost_feat=m.mul_cost_feat, cat_cost_feat=m.cat_cost_feat,
                     action_head_layers=m.action_head_layers, cost_prefix=m.cost_prefix, dtype=dtype)


class RefLoop:
    """The window tensors of CDTTrainer.rollout's own loop (cdt.py:436-518), with its exact torch expressions."""

    def __init__(self, m, obs, target_return, target_cost):
        self.m, EL, T = m, m.episode_len, m.seq_len
        self.states = torch.zeros(1, EL + 1, m.state_dim, device=DEV)
        self.actions = torch.zeros(1, EL, m.action_dim, device=DEV)
        self.returns = torch.zeros(1, EL + 1, device=DEV)
        self.costs = torch.zeros(1, EL + 1, device=DEV)
        self.time_steps = torch.arange(EL, dtype=torch.long, device=DEV).view(1, -1)
        self.states[:, 0] = torch.as_tensor(obs, device=DEV)
        self.returns[:, 0] = float(target_return)
        self.costs[:, 0] = float(target_cost)
        self.epi_cost = torch.tensor([target_cost], dtype=torch.float, device=DEV)
        self.tc = target_cost

    def sl(self, step):
        lo = max(0, step + 1 - self.m.seq_len)
        return (self.states[:, lo:step + 1], self.actions[:, lo:step + 1], self.returns[:, lo:step + 1],
                self.costs[:, lo:step + 1], self.time_steps[:, lo:step + 1])

    def window(self, step):
        s, a, r, c, t = self.sl(step)
        return dict(states=s[0].cpu().numpy(), actions=a[0].cpu().numpy(), returns=r[0].cpu().numpy(),
                    costs=c[0].cpu().numpy(), time_steps=t[0].cpu().numpy())

    def act(self, step):
        s, a, r, c, t = self.sl(step)
        acts, _, _ = self.m(s, a, r, c, t, None, self.epi_cost)
        if self.m.stochastic:
            acts = acts.mean
        return acts.clamp(-self.m.max_action, self.m.max_action)[0, -1].cpu().numpy()

    def oracle_act(self, o, step):
        w = self.window(step)
        n, T = len(w["returns"]), self.m.seq_len
        pad = lambda x: np.concatenate([x, np.zeros((T - n,) + x.shape[1:], x.dtype)])[None]  # noqa: E731
        acts = o.act_mean(pad(w["states"]), pad(w["actions"]), pad(w["returns"]), pad(w["costs"]),
                          pad(w["time_steps"]), pad(np.ones(n, np.float32)), np.array([self.tc], np.float64))
        return np.clip(acts[0, n - 1], -self.m.max_action, self.m.max_action)

    def push(self, step, act, obs_next, reward, cost):
        self.actions[:, step] = torch.as_tensor(act, device=DEV)
        self.states[:, step + 1] = torch.as_tensor(obs_next, device=DEV)
        self.returns[:, step + 1] = self.returns[:, step] - float(reward)
        self.costs[:, step + 1] = self.costs[:, step] - float(cost)


def _episode(m, n_steps, o=None, oracle_steps=None, seed=0, tr=30.0, tc=5.0, fwd_every=True, teacher=True):
    """Teacher-forced episode on a host SyntheticSafeEnv: window / action checks at every step."""
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    env = SyntheticSafeEnv(m.state_dim, m.action_dim, n_steps + 1, seed=seed)
    rs = np.random.RandomState(100 + seed)
    pol = m.fast_policy()
    obs, _ = env.reset()
    ref = RefLoop(m, obs, tr, tc)
    act = pol.reset(obs, tr, tc)
    worst_f = worst_o = 0.0
    for step in range(n_steps):
        w, wr = pol.window(), ref.window(step)
        for k in wr:
            np.testing.assert_array_equal(w[k], wr[k], err_msg=f"window {k} at step {step}")
        if fwd_every or step in (m.seq_len - 1, m.seq_len, m.seq_len + 1):
            d = float(np.abs(act - ref.act(step)).max())
            worst_f = max(worst_f, d)
            assert d <= 2e-5, (step, act, ref.act(step))
        if o is not None and (oracle_steps is None or step in oracle_steps):
            ao = ref.oracle_act(o, step)
            d = float(np.abs(act - ao).max())
            worst_o = max(worst_o, d)
            assert d <= 5e-5, (step, act, ao)
        taken = np.clip(rs.randn(m.action_dim), -1, 1).astype(np.float32) if teacher else act
        obs, reward, term, trunc, info = env.step(taken)
        cost = info["cost"] * 2.0
        ref.push(step, taken, obs, reward, cost)
        if step + 1 < n_steps:
            act = pol.step(obs, reward, cost, action=taken if teacher else None)
    return worst_f, worst_o


@pytest.mark.parametrize("name", list(CDT_CASES))
def test_golden_case_episodes(name):
    from test_gpu_cdt import build_cdt_gpu
    c = CDT_CASES[name]
    m, tr, lg = build_cdt_gpu(c)
    m.eval()
    n = 3 * c.T + 2
    m.episode_len = max(m.episode_len, n)
    _episode(m, n, o=_oracle(m, c), seed=1)


def _c5(**kw):
    from osrl_amd.algorithms import CDT
    args = dict(seq_len=20, episode_len=300, embedding_dim=256, num_layers=3, num_heads=8, use_rew=True,
                use_cost=True, cost_transform=True, stochastic=True, target_entropy=-3, device=DEV)
    args.update(kw)
    torch.manual_seed(0)
    return CDT(11, 3, 1.0, **args)


def _train(m, steps, B=8, seed=0):
    from osrl_amd.algorithms import CDTTrainer
    from osrl_amd.common.logger import DummyLogger
    tr = CDTTrainer(m, None, DummyLogger(), lr_warmup_steps=1, learning_rate=1e-3, stats_mode="sync",
                    use_graph=False)
    g = torch.Generator(device="cpu").manual_seed(seed)
    T, od, ad = m.seq_len, m.state_dim, m.action_dim
    for _ in range(steps):
        t0 = torch.randint(0, 100, (B, 1), generator=g)
        tr.train_one_step(torch.randn(B, T, od, generator=g).to(DEV), torch.rand(B, T, ad, generator=g).to(DEV) * 2 - 1,
                          torch.randn(B, T, generator=g).to(DEV) * 10, torch.rand(B, T, generator=g).to(DEV) * 20,
                          (t0 + torch.arange(T)).to(DEV), torch.ones(B, T, device=DEV),
                          torch.rand(B, generator=g).to(DEV) * 20, (torch.rand(B, T, generator=g) < 0.3).float().to(DEV))
    return tr


def test_c5_architecture_after_training():
    m = _c5()
    _train(m, 4)
    m.eval()
    _episode(m, 120, o=_oracle(m), seed=2)


def test_domain_edge_s256_e512():
    from osrl_amd.algorithms import CDT
    torch.manual_seed(1)
    m = CDT(6, 2, 1.0, seq_len=64, episode_len=200, embedding_dim=512, num_layers=1, num_heads=4, use_rew=True,
            use_cost=True, stochastic=False, device=DEV)
    assert m.seq_repeat * m.seq_len == 256
    m.eval()
    T = m.seq_len
    _episode(m, 2 * T + 2, o=_oracle(m), oracle_steps=(T - 1, T, T + 1), seed=3)


@pytest.mark.parametrize("kw", [dict(seq_len=64, embedding_dim=64, num_heads=4, cost_prefix=True),
                                dict(seq_len=10, embedding_dim=640, num_heads=8)])
def test_domain_refusals_fall_back(kw):
    from osrl_amd.algorithms import CDT, CDTTrainer
    from osrl_amd.common.logger import DummyLogger
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    m = CDT(5, 2, 1.0, episode_len=8, num_layers=1, use_rew=True, use_cost=True, device=DEV, **kw)
    with pytest.raises(NotImplementedError, match="257 tokens" if kw["embedding_dim"] == 64 else "embedding_dim 640"):
        m.fast_policy()
    tr = CDTTrainer(m, SyntheticSafeEnv(5, 2, 8, seed=0), DummyLogger(), use_graph=False)
    ret, cost, ln = tr.evaluate(1, 10.0, 2.0)
    assert ln == 8 and np.isfinite(ret) and m._fast is None


def _trainer_on_env(m, EL, fast, seed=4):
    from osrl_amd.algorithms import CDTTrainer
    from osrl_amd.common.logger import DummyLogger
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    return CDTTrainer(m, SyntheticSafeEnv(m.state_dim, m.action_dim, EL, seed=seed), DummyLogger(), use_graph=False,
                      cost_scale=2.0, fast_rollout=fast)


def test_whole_evaluations_fast_vs_loop():
    from test_gpu_cdt import build_cdt_gpu
    c = CDT_CASES["cdt_mid"]
    m, _, _ = build_cdt_gpu(c)
    EL = 50
    m.episode_len = EL
    fast = _trainer_on_env(m, EL, True).evaluate(3, 30.0, 5.0)
    slow = _trainer_on_env(m, EL, False).evaluate(3, 30.0, 5.0)
    assert m._fast is not None
    assert fast[2] == slow[2] == EL
    for a, b in zip(fast[:2], slow[:2]):
        assert abs(a - b) <= 1e-3 * max(1.0, abs(b)), (fast, slow)
    again = _trainer_on_env(m, EL, True).evaluate(3, 30.0, 5.0)
    assert again == fast


def _first_actions_match_forward(m, n=20, seed=5):
    was = m.training
    m.eval()
    _episode(m, n, seed=seed, teacher=False)
    if was:
        m.train()


def test_weights_stay_fresh(tmp_path):
    from osrl_amd.common.checkpoint import load_checkpoint, save_checkpoint
    m = _c5(seq_len=10, embedding_dim=128)
    tr = _train(m, 1)
    tr.env = _trainer_on_env(m, 30, True).env
    m.episode_len = 30
    save_checkpoint(m, str(tmp_path / "a.pt"))
    tr.evaluate(1, 30.0, 5.0)
    _first_actions_match_forward(m)
    _train(m, 3, seed=1)
    _first_actions_match_forward(m)
    load_checkpoint(m, str(tmp_path / "a.pt"))
    _first_actions_match_forward(m)


def test_handles_interleaved_reset_and_end():
    from test_gpu_cdt import build_cdt_gpu
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    c1, c2 = CDT_CASES["cdt_small"], CDT_CASES["cdt_v_prefix_det"]
    (m1, _, _), (m2, _, _) = build_cdt_gpu(c1), build_cdt_gpu(c2)
    m1.eval()
    m2.eval()
    p1, p2 = m1.fast_policy(), m2.fast_policy()
    assert m1.fast_policy() is p1
    e1, e2 = SyntheticSafeEnv(c1.od, c1.ad, 50, seed=6), SyntheticSafeEnv(c2.od, c2.ad, 50, seed=7)
    o1, _ = e1.reset()
    o2, _ = e2.reset()
    r1, r2 = RefLoop(m1, o1, 20.0, 3.0), RefLoop(m2, o2, 10.0, 4.0)
    a1, a2 = p1.reset(o1, 20.0, 3.0), p2.reset(o2, 10.0, 4.0)
    for step in range(2 * c1.T):
        assert np.abs(a1 - r1.act(step)).max() <= 2e-5 and np.abs(a2 - r2.act(step)).max() <= 2e-5, step
        o1, rw1, _, _, i1 = e1.step(a1)
        o2, rw2, _, _, i2 = e2.step(a2)
        r1.push(step, a1, o1, rw1, i1["cost"])
        r2.push(step, a2, o2, rw2, i2["cost"])
        a1, a2 = p1.step(o1, rw1, i1["cost"]), p2.step(o2, rw2, i2["cost"])
    # a reset in mid-episode starts over at timestep 0
    o1, _ = e1.reset()
    r1 = RefLoop(m1, o1, 15.0, 1.0)
    a1 = p1.reset(o1, 15.0, 1.0)
    assert np.abs(a1 - r1.act(0)).max() <= 2e-5
    assert len(p1.window()["returns"]) == 1
    # the episode ends after episode_len actions (read at reset)
    m2.episode_len = 5
    p2.reset(o2, 10.0, 4.0)
    for _ in range(4):
        p2.step(o2, 0.5, 0.0)
    with pytest.raises(RuntimeError, match="episode is over"):
        p2.step(o2, 0.5, 0.0)
