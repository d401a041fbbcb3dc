"""Quantile critics of fitted Q evaluation on the GPU (csrc/fqe_quantile.hip, engine/fqe.py ``QuantileFQEEngine`` /
``QuantileReadout``, ``FQETrainer.estimate_risk``) against plain fp64 numpy restatements of include/osrl_amd.h's formulas.

Gates: the loss launch and the step 1e-4 of each tensor's scale (the project's parity gate); the read-out 1e-12 relative
(inputs are offset so that no sum cancels).  Observed on MI355X (every case prints its figure): loss launch 8.7e-9 .. 8.9e-7,
read-out 0 in all 32 cases (these fp64 sums of fp32 values are exact), the step 1.9e-7 eager and graph.
The file's name sorts behind test_gpu_pipeline.py on purpose: that file's overlap control depends on how many streams and
graphs the process made before it (engine/core.py, the comment above CAPTURE_TRIES), and this file makes some."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from fqe_oracle import policy_action
from optim_oracle import tick_words
from test_gpu_fqe import CS, DEV, GAMMA, LR, MAXA, RS, TAU, batch, make_policy, to_dev, transitions

pytestmark = pytest.mark.gpu
MS = [2, 5, 33, 64]  # the smallest, an odd packing (12 rows in 60 lanes), just past half a wave, a full wave


def ref_loss(theta, theta_t, rew, cost, done, n_r, gamma, kappa, scale):
    """(dy [N, B, M], row_loss [N, B], stat_r, stat_c) in fp64."""
    th, tt, rew, cost, done = (np.asarray(a, np.float64) for a in (theta, theta_t, rew, cost, done))
    N, B, M = th.shape
    x = np.where(np.arange(N)[:, None] < n_r, rew[None], cost[None])
    T = x[..., None] + gamma * (1.0 - done)[None, :, None] * tt
    u = T[:, :, None, :] - th[:, :, :, None]  # [N, B, i, j]
    w = np.abs(((np.arange(M) + 0.5) / M)[None, None, :, None] - (u < 0))
    huber = np.where(np.abs(u) <= kappa, 0.5 * u * u, kappa * (np.abs(u) - 0.5 * kappa))
    row = (w * huber).sum(3).sum(2) / M / kappa
    dy = -(scale / M) * (w * np.clip(u, -kappa, kappa)).sum(3) / kappa
    return dy, row, row[:n_r].sum() * scale, row[n_r:].sum() * scale


def run_loss(theta, theta_t, rew, cost, done, n_r, gamma, kappa, scale=None):
    from osrl_amd.engine.fqe import quantile_loss, quantile_loss_desc
    N, B, M = theta.shape
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (theta, theta_t, rew, cost, done)]
    dy = torch.full((N, B, M), float("nan"), device=DEV)
    rl, stat = torch.full((N, B), float("nan"), device=DEV), torch.zeros(2, device=DEV)
    d = quantile_loss_desc(t[0], t[1], n_r, N - n_r, t[2], t[3], t[4], B, M, gamma, kappa, scale or 1.0 / B, dy=dy,
                           row_loss=rl, stat_r=stat.data_ptr(), stat_c=stat.data_ptr() + 4)
    quantile_loss(d)
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in (dy, rl, stat)]


def close(got, ref, what, worst):
    ref = np.asarray(ref, np.float64)
    d, scale = float(np.abs(np.asarray(got, np.float64) - ref).max()), float(np.abs(ref).max())
    worst[0] = max(worst[0], d / scale if scale > 0 else float(d > 0))
    assert d <= 1e-4 * scale, f"{what}: max diff {d:.3e} against scale {scale:.3e}"


@pytest.mark.parametrize("kappa", [1.0, 0.25])
@pytest.mark.parametrize("num_q", [1, 4])
@pytest.mark.parametrize("rows", [1, 7, 67])
@pytest.mark.parametrize("M", MS)
def test_loss_launch(M, rows, num_q, kappa):
    rs, N = np.random.RandomState(M * 1000 + rows), 2 * num_q
    th, tt = (rs.randn(N, rows, M).astype(np.float32) * 2 for _ in range(2))
    rew, cost = rs.randn(rows).astype(np.float32), rs.rand(rows).astype(np.float32)
    done = (np.arange(rows) % 3 == 1).astype(np.float32)
    r0 = min(3, rows - 1)  # u = 0 exactly: theta_t == theta (= 0), x = 0, done = 1 (reward net 0)
    th[0, r0], tt[0, r0], rew[r0], done[r0] = 0.0, 0.0, 0.0, 1.0
    th[N - 1, rows - 1] += 50.0  # |u| far beyond kappa (the last cost net)
    args = (th, tt, rew, cost, done, num_q, 0.9, kappa)
    got, again, worst = run_loss(*args), run_loss(*args), [0.0]
    for g, r, name in zip(got[:2] + list(got[2]), ref_loss(*args, 1.0 / rows), ("dy", "row_loss", "stat_r", "stat_c")):
        close(g, r, name, worst)
    print(f"quantile loss M={M} rows={rows} num_q={num_q} kappa={kappa}: worst diff / scale {worst[0]:.2e}")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), "a second launch gave other bits"
    if rows == 67:  # a row's dy / row_loss: the bits of the same row computed alone (at the same scale)
        for b in (0, 5, 66):
            sl = slice(b, b + 1)
            alone = run_loss(th[:, sl], tt[:, sl], rew[sl], cost[sl], done[sl], num_q, 0.9, kappa, scale=1.0 / 67)
            for a, g, name in zip(alone[:2], got[:2], ("dy", "row_loss")):
                assert a.tobytes() == np.ascontiguousarray(g[:, sl]).tobytes(), f"row {b}: {name} depends on its place"


@pytest.mark.parametrize("alpha", ["1/M", 0.1, 0.5, 1.0])
@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("M", MS)
def test_readout_sums(M, rows, alpha):
    from osrl_amd import _lib as L
    k = min(M, max(1, math.ceil((1.0 / M if alpha == "1/M" else alpha) * M - 1e-9)))
    rs = np.random.RandomState(M + rows)
    th = (rs.randn(3, rows, M) + 4.0).astype(np.float32)  # unsorted: crossing quantiles are legal input
    th[:, :, 1] = th[:, :, 0]                              # duplicates
    th[:, ::2] = np.round(th[:, ::2])                      # many more
    n_lo = 2  # two reward nets, one cost net
    acc, t = torch.zeros(3, 2, dtype=torch.float64, device=DEV), torch.from_numpy(th).to(DEV)
    L.check(L.load().osrl_fqe_quantile_sums(t.data_ptr(), 3, n_lo, rows, M, k, k, acc.data_ptr(), None), "sums")
    got = acc.cpu().numpy()
    s = np.sort(th.astype(np.float64), axis=2)
    ref = np.stack([s.sum((1, 2)), np.concatenate([s[:n_lo, :, :k].sum((1, 2)), s[n_lo:, :, M - k:].sum((1, 2))])], 1)
    rel = float(np.abs(got / ref - 1.0).max())
    print(f"quantile read-out M={M} rows={rows} k={k}: worst relative error {rel:.2e}")
    assert rel <= 1e-12
    if k == M:
        assert np.array_equal(got[:, 0], got[:, 1])  # alpha = 1: both CVaRs are the mean


def f64_dict(sd):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in sd.items()}


class RefStep:
    """One quantile-FQE step in fp64 numpy: forward, the loss above, backward, Adam + Polyak (optim_oracle's formulas)."""

    def __init__(self, sd, act, kappa):
        self.p = f64_dict(sd)
        self.keys = [k for k in self.p if "_old" not in k]
        self.m, self.v = ({k: np.zeros_like(self.p[k]) for k in self.keys} for _ in range(2))
        self.act, self.kappa, self.t = act, kappa, 0

    def fwd(self, pre, x):
        hs = [x]
        for l in range(3):
            z = hs[-1] @ self.p[f"{pre}.{2 * l}.weight"].T + self.p[f"{pre}.{2 * l}.bias"]
            hs.append(np.maximum(z, 0.0) if l < 2 else z)
        return hs

    def step(self, obs, nobs, act, rew, cost, done):
        f = lambda a: np.asarray(a, np.float64)  # noqa: E731
        x, xn = np.concatenate([f(obs), f(act)], 1), np.concatenate([f(nobs), f(self.act(f(nobs)))], 1)
        g, stats = {}, {}
        for ens, xs in (("critic", rew), ("cost_critic", cost)):
            for e in range(2):
                pre = f"{ens}.q_nets.{e}"
                hs, tt = self.fwd(pre, x), self.fwd(f"{ens}_old.q_nets.{e}", xn)[-1]
                d, _, st, _ = ref_loss(hs[-1][None], tt[None], xs, xs, done, 1, GAMMA, self.kappa, 1.0 / len(x))
                stats[ens], d = stats.get(ens, 0.0) + st, d[0]
                for l in (2, 1, 0):
                    g[f"{pre}.{2 * l}.weight"], g[f"{pre}.{2 * l}.bias"] = d.T @ hs[l], d.sum(0)
                    d = (d @ self.p[f"{pre}.{2 * l}.weight"]) * (hs[l] > 0)
        self.t += 1
        bc1, bc2s, _ = tick_words(self.t, 0.9, 0.999, 0)  # (1 - b1^t, sqrt(1 - b2^t)) of the fp32 betas
        b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
        for k in self.keys:
            self.m[k] = b1 * self.m[k] + (1 - b1) * g[k]
            self.v[k] = b2 * self.v[k] + (1 - b2) * g[k] * g[k]
            self.p[k] = self.p[k] - (LR / bc1) * self.m[k] / (np.sqrt(self.v[k]) / bc2s + 1e-8)
            kt = k.replace(".q_nets", "_old.q_nets")
            self.p[kt] = TAU * self.p[k] + (1 - TAU) * self.p[kt]
        return {"loss/fqe_reward_loss": stats["critic"], "loss/fqe_cost_loss": stats["cost_critic"]}


def make_qfqe(pol, use_graph=False, **kw):
    from osrl_amd.algorithms import FQE, FQETrainer
    from osrl_amd.common.logger import DummyLogger
    torch.manual_seed(11)
    fqe, lg = FQE(pol, [32, 32], gamma=GAMMA, tau=TAU, num_q=2, device=DEV, **kw), DummyLogger()
    return fqe, FQETrainer(fqe, logger=lg, critic_lr=LR, reward_scale=RS, cost_scale=CS, stats_mode="sync",
                           use_graph=use_graph), lg


@pytest.mark.parametrize("use_graph", [False, True])
def test_step_parity(use_graph):
    pol = make_policy("cpq")
    fqe, tr, lg = make_qfqe(pol, use_graph, num_quantiles=8, kappa=0.5)
    o = RefStep(fqe.state_dict(), policy_action("cpq", f64_dict(pol.state_dict()), MAXA), 0.5)
    d, worst = transitions(72), [0.0]
    for s in range(3):
        b = batch(d, s, 24)
        tr.train_one_step(*to_dev(b))
        for k, r in o.step(*b).items():
            close(lg.last(k), r, f"step {s + 1} {k}", worst)
        assert set(fqe.state_dict()) == set(o.p)
        for k, v in fqe.state_dict().items():
            close(v.detach().cpu().numpy(), o.p[k], f"step {s + 1} {k}", worst)
    print(f"quantile fqe step parity graph={use_graph}: worst diff / scale {worst[0]:.2e}")


def test_estimate_risk_and_refusals():
    from osrl_amd.common.replay import ReplayStore
    from osrl_amd.engine.mpc import check_terminal
    pol = make_policy("cpq")
    store = ReplayStore(transitions(200), DEV, reward_scale=RS, cost_scale=CS, seed=5, state_init=True)
    fqe, tr, _ = make_qfqe(pol, num_quantiles=8)
    r1, e = tr.estimate_risk(store, alpha=1.0), tr.estimate(store)
    assert tuple(e) == (r1.value, r1.value_std, r1.cost_value, r1.cost_value_std, r1.n_init) and r1.n_init > 7
    assert r1.value_cvar == r1.value and r1.cost_cvar == r1.cost_value  # alpha = 1: the tail is everything
    r = tr.estimate_risk(store, alpha=0.25)
    assert r == tr.estimate_risk(store, alpha=0.25) and r.value_cvar < r.value and r.cost_cvar > r.cost_value
    assert np.allclose(r[:8], tr.estimate_risk(store, alpha=0.25, rows=7)[:8], rtol=1e-12, atol=0)
    pytest.raises(TypeError, check_terminal, pol, None, "cpq", fqe, GAMMA)
    scalar, tr_s, _ = make_qfqe(pol)
    pytest.raises(TypeError, tr_s.estimate_risk, store)
    for bad in (dict(num_quantiles=1), dict(num_quantiles=65), dict(num_quantiles=8, kappa=0.0), dict(kappa=-1.0)):
        pytest.raises(ValueError, make_qfqe, pol, **bad)
    # a default model: the parent's keys and shapes; a quantile model: the same keys, the last layer M wide
    want = {f"{ens}.q_nets.{e}.{2 * l}.{w}": (o,) + ((i,) if w == "weight" else ())
            for ens in ("critic", "cost_critic", "critic_old", "cost_critic_old") for e in range(2)
            for l, (i, o) in enumerate([(7, 32), (32, 32), (32, 1)]) for w in ("weight", "bias")}
    assert {k: tuple(v.shape) for k, v in scalar.state_dict().items()} == want
    assert type(scalar.engine(24)).__name__ == "FQEEngine"
    qs = {k: tuple(v.shape) for k, v in fqe.state_dict().items()}
    assert set(qs) == set(want) and all(v == want[k] or (k.split(".")[3] == "4" and v[0] == 8) for k, v in qs.items())


def test_checkpoint_round_trip(tmp_path):
    from osrl_amd.common.checkpoint import load_checkpoint, save_checkpoint
    pol = make_policy("cpq")
    fqe, tr, _ = make_qfqe(pol, num_quantiles=8)
    tr.train_one_step(*to_dev(batch(transitions(24), 0, 24)))
    save_checkpoint(fqe, str(tmp_path / "q.pt"))
    other, _, _ = make_qfqe(pol, num_quantiles=8)
    load_checkpoint(other, str(tmp_path / "q.pt"))
    a, b, ga, gb = fqe.state_dict(), other.state_dict(), fqe.groups["critic"], other.groups["critic"]
    assert all(torch.equal(a[k], b[k]) for k in a) and torch.equal(ga.m, gb.m) and torch.equal(ga.v, gb.v)


def test_entry_points_refuse_bad_arguments():
    from osrl_amd import _lib as L
    from osrl_amd.engine.fqe import quantile_loss_desc
    lib = L.load()
    t, v = torch.zeros(2, 3, 4, device=DEV), torch.zeros(3, device=DEV)

    def loss(n_r=1, n_c=1, rows=3, M=4, kappa=1.0, theta=t, rew=v):
        d = quantile_loss_desc(theta, t, n_r, n_c, rew, v, v, rows, M, 0.9, kappa, 1.0, dy=torch.zeros_like(t))
        return lib.osrl_fqe_quantile_loss(C.byref(d), None)

    assert loss() == 0 and lib.osrl_fqe_quantile_loss(None, None) == -1
    for bad in (dict(M=1), dict(M=65), dict(kappa=0.0), dict(kappa=-1.0), dict(rows=0), dict(n_r=5, n_c=4),
                dict(theta=None), dict(rew=None)):
        assert loss(**bad) == -1, bad
    acc = torch.zeros(4, dtype=torch.float64, device=DEV)
    sums = lambda p=t.data_ptr(), n=2, rows=3, M=4, k=1, a=acc.data_ptr(): lib.osrl_fqe_quantile_sums(  # noqa: E731
        p, n, 1, rows, M, k, k, a, None)
    bad = [sums(p=None), sums(a=None), sums(n=9), sums(rows=0), sums(M=1), sums(M=65), sums(k=0), sums(k=5)]
    assert sums() == 0 and bad == [-1] * 8
    torch.cuda.synchronize()
