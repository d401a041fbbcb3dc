"""The Gaussian dynamics ensemble's oracle (tests/gauss_dynamics_oracle.py) and cases (tests/gauss_dynamics_cases.py) on the
CPU: the oracle's loss and written-out backward against torch autograd in fp64 (1e-10 relative), and the conditions the
GPU tests (tests/test_gpu_gauss_dynamics.py) rely on, checked with the oracle alone on its own 12-step rollouts:

  * at least 5 % of the raw log-variances lie above ``hi`` and at least 5 % below ``lo`` in every case;
  * both cost values occur, and at most 2 % of the rows lie within 1e-3 of the 0.5 threshold, with ``sample`` on and off;
  * with the noise at +-3 some but not all next states hit the clamp.
"""
import numpy as np
import pytest
import torch

import gauss_dynamics_cases as GC
import model_env_cases as MC
from gauss_dynamics_oracle import GaussOracleDynamics

IDS = lambda c: f"od{c[0]}-h{len(c[2])}x{c[2][0]}-M{c[3]}"  # noqa: E731


def _batch(n, od, ad, seed=1):
    rs = np.random.RandomState(seed)
    obs = rs.randn(n, od)
    return obs, obs + 0.3 * rs.randn(n, od), rs.uniform(-1, 1, (n, ad)), 2.0 + 3.0 * rs.randn(n), \
        (np.arange(n) % 3 == 0).astype(np.float64)


def _torch_loss(o, p, b):
    F = torch.nn.functional
    x = torch.from_numpy(o.inputs(b[0], b[2]))
    tg = torch.from_numpy(o.targets(b[0], b[1], b[3], b[4]))
    od, P = o.od, o.P
    loss = 0.0
    for m in range(o.M):
        h = x
        for i in range(o.n_layers):
            h = h @ p[f"members.{m}.{2 * i}.weight"].T + p[f"members.{m}.{2 * i}.bias"]
            if i < o.n_layers - 1:
                h = torch.relu(h)
        mu, cost, raw = h[:, :P], h[:, od + 1], h[:, od + 2:]
        lv = o.hi - F.softplus(o.hi - raw)
        lv = o.lo + F.softplus(lv - o.lo)
        loss = loss + (((mu - tg[:, :P]) ** 2 * torch.exp(-lv) + lv).sum() + ((cost - tg[:, od + 1]) ** 2).sum()) / tg.numel()
    return loss


@pytest.mark.parametrize("shape", GC.SHAPES, ids=IDS)
def test_oracle_loss_and_grads_equal_autograd(shape):
    od, ad, hidden, M = shape
    o = GaussOracleDynamics(GC.gauss_state_dict(od, ad, hidden, M))
    b = _batch(48, od, ad)
    loss, g = o.loss_and_grads(*b)
    p = {k: torch.from_numpy(v.copy()).requires_grad_(k.startswith("members.")) for k, v in o.p.items()}
    tl = _torch_loss(o, p, b)
    tl.backward()
    assert abs(loss - tl.item()) <= 1e-10 * abs(tl.item())
    for k in o.train_keys:
        ref = p[k].grad.numpy()
        assert np.abs(g[k] - ref).max() <= 1e-10 * np.abs(ref).max(), k
    last = 2 * (o.n_layers - 1)
    assert np.abs(g[f"members.0.{last}.bias"][od + 2:]).max() > 0.0  # the log-variance columns carry gradient


def _rollout(case, sample, eps):
    E, od, ad, hidden, M, mode, member, clamp, lam, unc, seed = case
    o = GaussOracleDynamics(GC.gauss_state_dict(od, ad, hidden, M, seed))
    s, acts = MC.start_rows(E, od).astype(np.float64), MC.actions(E, ad)
    out = []
    for t in range(GC.T_STEPS):
        ref = o.env_step(s, acts[t], mode, member, GC.members_in(E, M), clamp, lam, GC.MAX_ACTION, sample, unc, eps)
        out.append(ref)
        s = ref["s_next"]
    return o, out


@pytest.mark.parametrize("case", GC.PARITY, ids=lambda c: f"E{c[0]}-od{c[1]}-M{c[4]}-{c[5]}-c{int(c[7])}-{c[9]}")
def test_cases_reach_what_the_gpu_tests_rely_on(case):
    E, od, ad, hidden, M, mode, member, clamp, lam, unc, seed = case
    for sample in (False, True):
        o, steps = _rollout(case, sample, GC.noise(E, od + 1))
        raw = np.concatenate([r["y"][:, :, od + 2:].reshape(-1) for r in steps])
        assert (raw > o.hi).mean() >= 0.05 and (raw < o.lo).mean() >= 0.05, ((raw > o.hi).mean(), (raw < o.lo).mean())
        cost = np.concatenate([r["cost"] for r in steps])
        near = np.concatenate([np.abs(r["cost_raw"] - 0.5) <= 1e-3 for r in steps])
        assert near.mean() <= 0.02, near.mean()
        assert set(np.unique(cost)) == {0.0, 1.0}
        assert np.isfinite(np.concatenate([r["s_next"].reshape(-1) for r in steps])).all()
    _, steps = _rollout(case, True, GC.noise_pm3(E, od + 1))
    un = np.concatenate([r["s_unclamped"].reshape(-1) for r in steps])
    hit = (un < -0.8) | (un > 0.8)
    assert 0.0 < hit.mean() < 1.0, hit.mean()


def test_signals_and_sampling_of_the_oracle():
    """max_std is the largest member's rms sigma; sample off ignores eps; the mean model's first od + 2 rows are the
    Gaussian model's."""
    od, ad, hidden, M = GC.SHAPES[1]
    sd = GC.gauss_state_dict(od, ad, hidden, M)
    o = GaussOracleDynamics(sd)
    s, a = MC.start_rows(19, od), MC.actions(19, ad)[0]
    r0 = o.env_step(s, a, "member", 1, uncertainty="max_std")
    assert np.allclose(r0["u"], np.sqrt((r0["sigma"][:, :, :od] ** 2).mean(2)).max(0)) and (r0["u"] == r0["a"]).all()
    r1 = o.env_step(s, a, "member", 1, sample=True, eps=GC.noise(19, od + 1), clamp=False)
    exp = r0["mean_s_next"] + o.p["sd_d"] * r1["sigma"][1][:, :od] * GC.noise(19, od + 1)[:, :od]
    assert np.allclose(r1["s_next"], exp, rtol=0, atol=1e-12)
    assert (r1["cost"] == r0["cost"]).all()  # the cost column is never sampled
    lo, hi = o.lo, o.hi
    lv = np.exp(0.5 * o.logvar(np.array([-1e3, 1e3]))[0]) ** 2
    assert np.isclose(np.log(lv[0]), lo, atol=1e-3) and np.isclose(np.log(lv[1]), hi, atol=1e-3)
    det = GC.mean_state_dict(od, ad, hidden, M)
    last = 2 * len(hidden)
    for m in range(M):
        assert np.array_equal(det[f"members.{m}.{last}.weight"], sd[f"members.{m}.{last}.weight"][:od + 2])
        assert np.array_equal(det[f"members.{m}.{last}.bias"], sd[f"members.{m}.{last}.bias"][:od + 2])
