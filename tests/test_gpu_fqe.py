"""Fitted Q evaluation on the GPU against its fp64 restatement (tests/fqe_oracle.py).

Bound: max |gpu - oracle| <= 1e-4 of each tensor's scale (scale = max |oracle tensor|; for a scalar its magnitude), for the
parameters, the targets, both Adam moments and both loss statistics.  lr = 1e-4 (the other trainers' default): Adam's
first steps move every element by about lr whatever its gradient's size, so a wrong update shows as >= 1e-5 against bounds
of 4e-6 .. 4e-5, while the moments pin the gradients themselves.  Shapes: (od, ad) = (5, 2); B = 50 = three full 16-row
tiles and one of 2 rows; hidden [32, 24] (4-wave tile), [160, 32] (8-wave tile), [512, 32] (wide path).
Every parity test prints its worst diff / scale.  Observed on MI355X: 1.31e-5 .. 1.35e-5 in every step-parity case (the
size of the one known fp32 term: 1 - beta2 rounded to fp32 is 1.3e-5 off 0.001, which Adam's second moment carries);
the estimates 7e-8 (cpq, num_q 1) and 1.7e-7 (bcql, num_q 2)."""
import numpy as np
import pytest
import torch

from fqe_oracle import OracleFQE, policy_action

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OD, AD, MAXA = 5, 2, 1.5
RS, CS = 0.1, 2.0            # reward_scale / cost_scale: a swap of the reward and cost pointers cannot pass
GAMMA, TAU, LR = 0.9, 0.05, 1e-4
BOUND = 1e-4
PH = [16, 12]                # the policies' hidden sizes


def _note(msg):
    print(msg)


def make_policy(kind, seed=3):
    from osrl_amd.algorithms import BC, BCQL, CPQ, COptiDICE
    torch.manual_seed(seed)
    if kind == "bc":
        return BC(OD, AD, MAXA, PH, device=DEV)
    if kind == "cpq":
        return CPQ(OD, AD, MAXA, PH, PH, 16, 2, device=DEV)
    if kind == "dice":
        return COptiDICE(OD, AD, MAXA, "softchi", 0.15, np.ones((1, OD), np.float32), np.ones((1, AD), np.float32), PH, PH,
                         device=DEV)
    return BCQL(OD, AD, MAXA, PH, PH, 16, 2, device=DEV)


def policy_oracle(kind, sd):
    p = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in sd.items()}
    kw = {}
    if kind == "dice":
        kw = dict(f_type="softchi", init_state_propotion=0.15, observations_std=np.ones((1, OD)),
                  actions_std=np.ones((1, AD)))
    return policy_action(kind, p, MAXA, **kw)


def make_fqe(policy, hidden, num_q, seed=11, **trainer_kw):
    from osrl_amd.algorithms import FQE, FQETrainer
    from osrl_amd.common.logger import DummyLogger
    torch.manual_seed(seed)
    fqe = FQE(policy, hidden, gamma=GAMMA, tau=TAU, num_q=num_q, device=DEV)
    lg = DummyLogger()
    kw = dict(critic_lr=LR, reward_scale=RS, cost_scale=CS, stats_mode="sync", use_graph=False)
    kw.update(trainer_kw)
    return fqe, FQETrainer(fqe, logger=lg, **kw), lg


def transitions(n, seed=1):
    """synthetic_transitions with ``done`` forced to a 0/1 mix."""
    from osrl_amd.common.replay import synthetic_transitions
    d = synthetic_transitions(n, OD, AD, seed=seed, max_action=MAXA)
    d["terminals"] = (np.arange(n) % 3 == 1).astype(np.float32)
    return d


def batch(d, s, B):
    """Minibatch ``s`` as the store would hand it out: rewards and costs scaled; numpy fp32."""
    sl = slice(s * B, (s + 1) * B)
    return (d["observations"][sl], d["next_observations"][sl], d["actions"][sl], d["rewards"][sl] * np.float32(RS),
            d["costs"][sl] * np.float32(CS), d["terminals"][sl])


def to_dev(b):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in b]


def _worst(gpu, ref, what, worst):
    ref = np.asarray(ref, np.float64)
    d = float(np.abs(np.asarray(gpu, np.float64) - ref).max())
    scale = float(np.abs(ref).max())
    worst[0] = max(worst[0], d / scale if scale > 0 else (0.0 if d == 0 else np.inf))
    assert d <= BOUND * scale, f"{what}: max diff {d:.3e} vs scale {scale:.3e} ({d / max(scale, 1e-300):.2e} of it)"


def compare_state(fqe, o, worst, tag):
    sd = fqe.state_dict()
    assert set(sd) == set(o.p)
    for k, v in sd.items():
        _worst(v.detach().cpu().numpy(), o.p[k].numpy(), f"{tag} {k}", worst)
    st = fqe.groups["critic"].optim_state()
    for k in o.train_keys:
        _worst(st["exp_avg"][k].numpy(), o.m[k].numpy(), f"{tag} exp_avg {k}", worst)
        _worst(st["exp_avg_sq"][k].numpy(), o.v[k].numpy(), f"{tag} exp_avg_sq {k}", worst)


def run_parity(kind, B, hidden, num_q, steps=3):
    pol = make_policy(kind)
    fqe, tr, lg = make_fqe(pol, hidden, num_q)
    o = OracleFQE(fqe.state_dict(), policy_oracle(kind, pol.state_dict()), GAMMA, TAU, LR)
    d = transitions(steps * B)
    rs = np.random.RandomState(7)
    worst = [0.0]
    for s in range(steps):
        b = batch(d, s, B)
        z = rs.randn(B, pol.latent_dim).astype(np.float32) if kind == "bcql" else None
        tr.train_one_step(*to_dev(b), noise=None if z is None else {"z": torch.from_numpy(z).to(DEV)})
        ost = o.step(*b, z=z)
        for k, r in ost.items():
            _worst(lg.last(k), r, f"step {s + 1} {k}", worst)
        compare_state(fqe, o, worst, f"step {s + 1}")
    _note(f"fqe parity {kind} B={B} hidden={hidden} num_q={num_q}: worst diff / scale {worst[0]:.2e}")


@pytest.mark.parametrize("kind", ["bc", "cpq", "dice", "bcql"])
@pytest.mark.parametrize("num_q", [1, 2])
def test_step_parity(kind, num_q):
    run_parity(kind, 50, [32, 24], num_q)


def test_step_parity_8wave_tile():
    run_parity("cpq", 33, [160, 32], 2)


def test_step_parity_wide_path():
    run_parity("cpq", 33, [512, 32], 1)


def test_step_parity_four_members():
    run_parity("bcql", 50, [32, 24], 4)


def test_members_are_independent():
    """Only online cost member 1 sees a change of target cost member 1; everything else keeps its bits."""
    pol = make_policy("bc")
    b = to_dev(batch(transitions(50), 0, 50))
    out = []
    for perturb in (False, True):
        fqe, tr, _ = make_fqe(pol, [32, 24], 2)
        if perturb:
            with torch.no_grad():
                fqe.cost_critic_old.q_nets[1][4].bias += 0.25
            fqe.repack()
        tr.train_one_step(*b)
        out.append({k: v.detach().cpu().clone() for k, v in fqe.state_dict().items()})
    moved = [k for k in out[0] if not torch.equal(out[0][k], out[1][k])]
    assert moved and all(k.startswith(("cost_critic.q_nets.1.", "cost_critic_old.q_nets.1.")) for k in moved), moved
    assert any(k.startswith("cost_critic.q_nets.1.") for k in moved)


def test_graph_replay_equals_eager_uniform_and_weighted():
    from osrl_amd.common.replay import ReplayStore
    pol = make_policy("bcql")
    n, B = 256, 33
    store = ReplayStore(transitions(n), DEV, reward_scale=RS, cost_scale=CS, seed=5, state_init=True)
    runs = []
    for _ in range(2):
        fqe, tr, _ = make_fqe(pol, [32, 24], 2)
        eng = fqe.engine(B)
        eng.attach_replay(store)
        runs.append((fqe, eng))

    def same(tag):
        a, b = (r[0].state_dict() for r in runs)
        for k in a:
            assert torch.equal(a[k], b[k]), f"{tag}: {k}"
        ga, gb = (r[0].groups["critic"] for r in runs)
        assert torch.equal(ga.m, gb.m) and torch.equal(ga.v, gb.v), tag

    for use_graph, (fqe, eng) in zip((True, False), runs):
        for _ in range(4):
            eng.step_replay(use_graph)
    same("uniform")
    before = {k: v.clone() for k, v in runs[0][0].state_dict().items()}
    graph0 = runs[0][1].graph
    assert graph0 is not None and runs[1][1].graph is None
    w = np.linspace(0.0, 1.0, n) ** 2
    store.set_sample_prob(w)
    for use_graph, (fqe, eng) in zip((True, False), runs):
        for _ in range(4):
            eng.step_replay(use_graph)
    same("weighted")
    assert runs[0][1].graph is not None and runs[0][1].graph is not graph0  # the switch recaptured
    assert any(not torch.equal(before[k], v) for k, v in runs[0][0].state_dict().items())
    store.set_sample_prob(None)


def test_policy_is_read_in_place():
    """Other weights loaded into the policy between two (graph-replayed) steps are what the second step acts by."""
    pol, other = make_policy("cpq", seed=3), make_policy("cpq", seed=4)
    sd0 = {k: v.detach().cpu().clone() for k, v in pol.state_dict().items()}
    sd1 = {k: v.detach().cpu().clone() for k, v in other.state_dict().items()}
    fqe, tr, lg = make_fqe(pol, [32, 24], 2, use_graph=True)
    acts = [policy_oracle("cpq", sd0), policy_oracle("cpq", sd1)]
    cur = [0]
    o = OracleFQE(fqe.state_dict(), lambda obs, z=None: acts[cur[0]](obs, z), GAMMA, TAU, LR)
    d = transitions(100)
    worst = [0.0]
    for s in range(2):
        if s == 1:
            pol.load_state_dict(sd1)
            cur[0] = 1
        b = batch(d, s, 50)
        tr.train_one_step(*to_dev(b))
        ost = o.step(*b)
        for k, r in ost.items():
            _worst(lg.last(k), r, f"step {s + 1} {k}", worst)
    compare_state(fqe, o, worst, "after the policy changed")
    # ... and the two policies do act differently enough for the check to mean something
    x = d["next_observations"][:50].astype(np.float64)
    assert np.abs(acts[0](x) - acts[1](x)).max() > 1e-2
    _note(f"fqe policy-in-place: worst diff / scale {worst[0]:.2e}")


def _store_with_7_initial_states(n=64, state_init=True):
    from osrl_amd.common.replay import ReplayStore
    d = transitions(n)
    term = np.zeros(n, np.float32)
    term[[4, 9, 17, 30, 31, 50]] = 1.0  # + row 0: seven initial states
    d["terminals"] = term
    return d, ReplayStore(d, DEV, reward_scale=RS, cost_scale=CS, state_init=state_init)


@pytest.mark.parametrize("kind,num_q", [("cpq", 1), ("bcql", 2)])
def test_estimate(kind, num_q):
    pol = make_policy(kind)
    fqe, tr, _ = make_fqe(pol, [32, 24], num_q)
    d, store = _store_with_7_initial_states()
    tr.train_one_step(*to_dev(batch(d, 0, 50)))  # (the read-out follows the trained parameters)
    init = np.concatenate([[1.0], d["terminals"][:-1]]) == 1
    s0 = d["observations"][init]
    assert s0.shape[0] == 7
    z = np.random.RandomState(9).randn(7, pol.latent_dim).astype(np.float32) if kind == "bcql" else None
    e4, e1024 = tr.estimate(store, rows=4, z=z), tr.estimate(store, rows=1024, z=z)
    assert e4 == e1024 and e4.n_init == 7
    if kind == "bcql":  # the decode noise drawn on device is a function of the seed alone
        assert tr.estimate(store, rows=4) == tr.estimate(store, rows=1024) == tr.estimate(store, rows=3)
    o = OracleFQE(fqe.state_dict(), policy_oracle(kind, pol.state_dict()), GAMMA, TAU, LR)
    ref = o.estimate(s0, z, RS, CS)
    worst = [0.0]
    for name, got, r in zip(e4._fields[:4], e4[:4], ref[:4]):
        if num_q == 1 and name.endswith("_std"):
            assert got == 0.0 and r == 0.0
        else:
            _worst(got, r, f"estimate {name}", worst)
    assert ref[4] == 7
    _note(f"fqe estimate {kind} num_q={num_q}: {e4}; worst diff / scale {worst[0]:.2e}")


def test_checkpoint_resume_is_bit_identical(tmp_path):
    from osrl_amd.common.checkpoint import load_checkpoint, save_checkpoint
    pol = make_policy("bcql")
    d = transitions(200)
    bs = [to_dev(batch(d, s, 50)) for s in range(4)]

    def state(fqe):
        g = fqe.groups["critic"]
        return [v.detach().clone() for v in fqe.state_dict().values()] + [g.m.clone(), g.v.clone()]

    a, tra, _ = make_fqe(pol, [32, 24], 2, seed=21)
    for b in bs:
        tra.train_one_step(*b)  # (the decode noise is drawn on device: a function of seed and step)
    b_, trb, _ = make_fqe(pol, [32, 24], 2, seed=21)
    for b in bs[:2]:
        trb.train_one_step(*b)
    path = str(tmp_path / "fqe.pt")
    save_checkpoint(b_, path)
    c, trc, _ = make_fqe(pol, [32, 24], 2, seed=21)
    with torch.no_grad():
        for p in c.parameters():
            p.add_(1.0)  # a fresh model that is NOT the saved one until the checkpoint is loaded
    load_checkpoint(c, path)
    for b in bs[2:]:
        trc.train_one_step(*b)
    for x, y in zip(state(a), state(c)):
        assert torch.equal(x, y)
    assert c.engine(50).st.device_step() == 4
    assert not any(k.startswith(("actor", "vae", "policy")) for k in c.state_dict())  # the policy is not saved


def test_refusals():
    from osrl_amd.algorithms import CDT, FQE
    pol = make_policy("bc")
    cdt = CDT(OD, AD, MAXA, seq_len=4, episode_len=20, embedding_dim=16, num_layers=1, num_heads=2, device=DEV)
    with pytest.raises(TypeError):
        FQE(cdt, [32, 24], device=DEV)
    with pytest.raises(ValueError):
        FQE(pol, [32, 24], num_q=5, device=DEV)
    with pytest.raises(ValueError):
        FQE(pol, [32, 24], device=DEV, state_dim=OD - 1)  # (BC multi-task: the policy's input is wider than the state)
    fqe, tr, _ = make_fqe(pol, [32, 24], 1)
    d, plain = _store_with_7_initial_states(state_init=False)
    with pytest.raises(ValueError):
        tr.estimate(plain)
    with pytest.raises(ValueError):
        fqe.engine(50, dist=object())
    eng = fqe.engine(50)
    eng.attach_replay(plain)
    with pytest.raises(RuntimeError):
        eng.step(*to_dev(batch(d, 0, 50)))
    eng.step_replay(False)  # (what the message asks for works)
