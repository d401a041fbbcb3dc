"""Numpy fp64 restatement of the Gaussian dynamics ensemble (TEST INFRASTRUCTURE ONLY): ``OracleDynamics`` with members
``[od + ad, *hidden, 2 od + 3]`` = (od + 1 means | raw cost | od + 1 raw log-variances).

Bounded log-variance (PETS' soft clamp, fixed bounds lo < hi), P = od + 1, column k < P:

    raw_k = y[od + 2 + k];  lv1 = hi - softplus(hi - raw_k);  lv_k = lo + softplus(lv1 - lo);  sigma_k = exp(0.5 lv_k)
    softplus(x) = max(x, 0) + log1p(exp(-|x|))

Train step, with s = 1 / (B (od + 2)) and t the target table of ``OracleDynamics.targets``:

    loss = sum_m s sum_rows [ sum_{c < P} ((mu_c - t_c)^2 exp(-lv_c) + lv_c) + (y_{od+1} - t_{od+1})^2 ]
    dmu_c = 2 (mu_c - t_c) exp(-lv_c) s;   dy_cost = 2 (y - t) s
    draw_c = (1 - (mu_c - t_c)^2 exp(-lv_c)) sigmoid(hi - raw_c) sigmoid(lv1_c - lo) s

with the backward pass through the layers written out as the base class does (tests/test_gauss_dynamics_cpu.py holds it
against autograd).

Environment step: the base class's on the first od + 2 columns, plus

    a = max_m sqrt(sum_{k < od} sigma_m[k]^2 / od);  u = d | a
    sample: v = sigma_f^2 (member / random) | mean_m sigma_m^2 (mean);  yh[k] += sqrt(v[k]) eps[k], k < P
"""
from __future__ import annotations

import numpy as np

from model_env_oracle import OracleDynamics, _f64


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


class GaussOracleDynamics(OracleDynamics):
    def __init__(self, state_dict, lr: float = 1e-3):
        super().__init__(state_dict, lr)
        self.lo, self.hi = float(self.p["logvar_min"][0]), float(self.p["logvar_max"][0])
        self.P = self.od + 1

    def logvar(self, raw):
        """(lv, lv1) of raw log-variances."""
        lv1 = self.hi - softplus(self.hi - raw)
        return self.lo + softplus(lv1 - self.lo), lv1

    def split(self, y):
        """(means incl. reward [.., P], cost [..], raw log-variances [.., P]) of output rows ``y``."""
        od = self.od
        return y[..., :od + 1], y[..., od + 1], y[..., od + 2:]

    # ---- the train step -----------------------------------------------------------------------------------------------
    def nll_terms(self, y, tg):
        """(loss, dY) of one member's output rows against the target table."""
        od, P = self.od, self.P
        s = 1.0 / tg.size  # tg is [B, od + 2]
        mu, cost, raw = self.split(y)
        lv, lv1 = self.logvar(raw)
        d, iv = mu - tg[:, :P], np.exp(-lv)
        dc = cost - tg[:, od + 1]
        loss = s * float((d * d * iv + lv).sum() + (dc * dc).sum())
        dy = np.zeros_like(y)
        dy[:, :P] = 2.0 * d * iv * s
        dy[:, od + 1] = 2.0 * dc * s
        dy[:, od + 2:] = (1.0 - d * d * iv) * sigmoid(self.hi - raw) * sigmoid(lv1 - self.lo) * s
        return loss, dy

    def loss_and_grads(self, obs, nobs, act, rew, cost):
        x, tg = self.inputs(obs, act), self.targets(obs, nobs, rew, cost)
        loss, g = 0.0, {}
        for m in range(self.M):
            keep: list = []
            y = self.net(m, x, keep)
            lm, dz = self.nll_terms(y, tg)
            loss += lm
            for i in reversed(range(self.n_layers)):
                W, _ = self._wb(m, i)
                g[f"members.{m}.{2 * i}.weight"] = dz.T @ keep[i]
                g[f"members.{m}.{2 * i}.bias"] = dz.sum(0)
                if i > 0:
                    dz = (dz @ W) * (keep[i] > 0.0)
        return loss, g

    def calibration(self, obs, nobs, act, rew, cost, member=None):
        """mean over rows, state columns and members of (t - mu)^2 exp(-lv): 1 for a calibrated model."""
        x, tg = self.inputs(obs, act), self.targets(obs, nobs, rew, cost)
        od, out = self.od, []
        for m in (range(self.M) if member is None else [member]):
            mu, _, raw = self.split(self.net(m, x))
            lv, _ = self.logvar(raw)
            out.append(((tg[:, :od] - mu[:, :od]) ** 2 * np.exp(-lv[:, :od])).mean())
        return float(np.mean(out))

    # ---- the environment step -----------------------------------------------------------------------------------------
    def env_step(self, s, a, mode: str = "mean", member: int = 0, members=None, clamp: bool = True, lam: float = 0.0,
                 max_action: float = 1.0, sample: bool = False, uncertainty: str = "disagreement", eps=None):
        """The base class's dict plus ``a`` (the largest predicted std), ``u`` (the signal in use), ``sigma`` [M, rows, P]
        and ``mean_s_next`` (the noise-free next state before the clamp); ``eps`` [rows, P] with ``sample``."""
        s, od, P = _f64(s), self.od, self.P
        n = s.shape[0]
        x = self.inputs(s, np.clip(_f64(a), -max_action, max_action))
        y = np.stack([self.net(m, x) for m in range(self.M)])
        ybar = y[0, :, :od + 2].copy()
        for m in range(1, self.M):
            ybar = ybar + y[m, :, :od + 2]
        ybar = ybar / self.M
        d = np.sqrt(((y[:, :, :od] - ybar[None, :, :od]) ** 2).sum(2) / od).max(0)
        lv, _ = self.logvar(y[:, :, od + 2:])
        sigma = np.exp(0.5 * lv)
        amax = np.sqrt((sigma[:, :, :od] ** 2).sum(2) / od).max(0)
        u = d if uncertainty == "disagreement" else amax
        if mode == "mean":
            yh, v = ybar.copy(), (sigma ** 2).sum(0) / self.M
        else:
            idx = np.full(n, member, np.int64) if mode == "member" else np.asarray(members, np.int64)
            yh, v = y[idx, np.arange(n), :od + 2].copy(), sigma[idx, np.arange(n)] ** 2
        mean_next = s + (self.p["mu_d"] + self.p["sd_d"] * yh[:, :od])
        if sample:
            yh[:, :P] = yh[:, :P] + np.sqrt(v) * _f64(eps)
        sn = s + (self.p["mu_d"] + self.p["sd_d"] * yh[:, :od])
        raw_next = sn
        if clamp:
            sn = np.minimum(np.maximum(sn, self.p["s_lo"]), self.p["s_hi"])
        r = self.p["mu_r"][0] + self.p["sd_r"][0] * yh[:, od]
        if lam != 0.0:
            r = r - lam * u
        return dict(s_next=sn, s_unclamped=raw_next, mean_s_next=mean_next, reward=r, d=d, a=amax, u=u, sigma=sigma,
                    cost_raw=yh[:, od + 1], cost=(yh[:, od + 1] > 0.5).astype(np.float64), y=y)
