"""Numpy fp64 restatement of the ensemble dynamics model: its train step and the environment step (TEST INFRASTRUCTURE ONLY).

Train step (engine/dynamics.py), every member m against the same normalised target:

    x      = [(s - mu_s) / sd_s, a]
    target = [(s' - s - mu_d) / sd_d, (r - mu_r) / sd_r, cost]
    loss   = sum_m mean_{rows, columns} (net_m(x) - target)^2

with the backward pass written out (tests/test_model_env_cpu.py holds it against autograd), then Adam (betas 0.9 / 0.999,
eps 1e-8, bias-corrected as torch.optim.Adam).

Environment step (csrc/model_env.hip), per episode:

    y_m = net_m([(s - mu_s) / sd_s, clip(a)]);  ybar = mean_m y_m;  d = max_m sqrt(mean_{k < od} (y_m[k] - ybar[k])^2)
    yh = ybar | y_member | y_j;  s' = clamp(s + mu_d + sd_d yh[:od]);  r = mu_r + sd_r yh[od] - lambda d;  cost = yh[od+1] > 0.5
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

TABLES = ("mu_s", "sd_s", "mu_d", "sd_d", "mu_r", "sd_r", "s_lo", "s_hi")


def _f64(v) -> np.ndarray:
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.array(v, dtype=np.float64)


class OracleDynamics:
    def __init__(self, state_dict: Dict[str, "np.ndarray"], lr: float = 1e-3):
        self.p = {k: _f64(v) for k, v in state_dict.items()}
        self.lr = float(lr)
        self.M = len({k.split(".")[1] for k in self.p if k.startswith("members.")})
        self.n_layers = len({k.split(".")[2] for k in self.p if k.startswith("members.0.")})
        self.train_keys = [k for k in self.p if k.startswith("members.")]
        self.m = {k: np.zeros_like(self.p[k]) for k in self.train_keys}
        self.v = {k: np.zeros_like(self.p[k]) for k in self.train_keys}
        self.t = 0
        self.od = self.p["mu_s"].shape[0]

    # ---- the members --------------------------------------------------------------------------------------------------
    def _wb(self, m: int, i: int, p=None):
        p = self.p if p is None else p
        return p[f"members.{m}.{2 * i}.weight"], p[f"members.{m}.{2 * i}.bias"]

    def net(self, m: int, x: np.ndarray, keep: Optional[list] = None) -> np.ndarray:
        """Member ``m`` on rows ``x`` (ReLU hidden layers, identity output); ``keep`` receives every layer's input."""
        for i in range(self.n_layers):
            W, b = self._wb(m, i)
            if keep is not None:
                keep.append(x)
            x = x @ W.T + b
            if i < self.n_layers - 1:
                x = np.maximum(x, 0.0)
        return x

    def inputs(self, obs, act) -> np.ndarray:
        return np.concatenate([(_f64(obs) - self.p["mu_s"]) / self.p["sd_s"], _f64(act)], 1)

    def targets(self, obs, nobs, rew, cost) -> np.ndarray:
        obs, nobs = _f64(obs), _f64(nobs)
        return np.concatenate([(nobs - obs - self.p["mu_d"]) / self.p["sd_d"],
                               ((_f64(rew).reshape(-1) - self.p["mu_r"][0]) / self.p["sd_r"][0])[:, None],
                               _f64(cost).reshape(-1, 1)], 1)

    # ---- the train step -----------------------------------------------------------------------------------------------
    def loss_and_grads(self, obs, nobs, act, rew, cost):
        x, tg = self.inputs(obs, act), self.targets(obs, nobs, rew, cost)
        n = tg.size
        loss, g = 0.0, {}
        for m in range(self.M):
            keep: list = []
            y = self.net(m, x, keep)
            diff = y - tg
            loss += float((diff ** 2).sum() / n)
            dz = 2.0 * diff / n
            for i in reversed(range(self.n_layers)):
                W, _ = self._wb(m, i)
                g[f"members.{m}.{2 * i}.weight"] = dz.T @ keep[i]
                g[f"members.{m}.{2 * i}.bias"] = dz.sum(0)
                if i > 0:
                    dz = (dz @ W) * (keep[i] > 0.0)  # keep[i] = relu(z_{i-1}): positive exactly where the ReLU passed
        return loss, g

    def step(self, obs, nobs, act, rew, cost, done=None) -> Dict[str, float]:
        loss, g = self.loss_and_grads(obs, nobs, act, rew, cost)
        self.t += 1
        b1, b2, eps = 0.9, 0.999, 1e-8
        bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
        for k in self.train_keys:
            self.m[k] = b1 * self.m[k] + (1 - b1) * g[k]
            self.v[k] = b2 * self.v[k] + (1 - b2) * g[k] * g[k]
            self.p[k] = self.p[k] - (self.lr / bc1) * self.m[k] / (np.sqrt(self.v[k]) / math.sqrt(bc2) + eps)
        return {"loss/dynamics_loss": loss}

    # ---- the environment step -----------------------------------------------------------------------------------------
    def env_step(self, s, a, mode: str = "mean", member: int = 0, members=None, clamp: bool = True, lam: float = 0.0,
                 max_action: float = 1.0):
        """One step of every row from state ``s`` under action ``a``: a dict with ``s_next``, ``reward`` (penalty applied),
        ``d`` (the disagreement), ``cost_raw`` (yh[od + 1]), ``cost`` (0 / 1) and ``y`` [M, rows, od + 2].
        ``members`` (mode "random"): the member index of every row."""
        s, od = _f64(s), self.od
        x = self.inputs(s, np.clip(_f64(a), -max_action, max_action))
        y = np.stack([self.net(m, x) for m in range(self.M)])
        ybar = y[0].copy()
        for m in range(1, self.M):
            ybar = ybar + y[m]
        ybar = ybar / self.M
        d = np.sqrt(((y[:, :, :od] - ybar[None, :, :od]) ** 2).sum(2) / od).max(0)
        if mode == "mean":
            yh = ybar
        elif mode == "member":
            yh = y[member]
        else:
            yh = y[np.asarray(members, np.int64), np.arange(s.shape[0])]
        sn = s + (self.p["mu_d"] + self.p["sd_d"] * yh[:, :od])
        if clamp:
            sn = np.minimum(np.maximum(sn, self.p["s_lo"]), self.p["s_hi"])
        r = self.p["mu_r"][0] + self.p["sd_r"][0] * yh[:, od]
        if lam != 0.0:
            r = r - lam * d
        return dict(s_next=sn, reward=r, d=d, cost_raw=yh[:, od + 1], cost=(yh[:, od + 1] > 0.5).astype(np.float64), y=y)

    def one_step_mse(self, obs, nobs, act, rew, cost) -> float:
        """The ensemble mean's normalised one-step squared error, averaged over rows and columns."""
        x, tg = self.inputs(obs, act), self.targets(obs, nobs, rew, cost)
        ybar = sum(self.net(m, x) for m in range(self.M)) / self.M
        return float(((ybar - tg) ** 2).mean())
