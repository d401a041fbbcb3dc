"""Numpy fp64 restatement of the bootstrap weights, the weighted member loss, the weighted train step, the holdout loss and
elite selection of the dynamics ensemble (TEST INFRASTRUCTURE ONLY; csrc/dyn_loss.hip, engine/dynamics.py
``BootDynamicsEngine``, algorithms/dynamics.py ``validate`` / ``select_elites``).

Bootstrap weight of dataset row i for member m under the 64-bit seed S:

    word = word x of Philox4x32-10(counter {i, m, 0, 17}, key {S & 0xFFFFFFFF, S >> 32})
    w    = #{k in 0 .. 7 : word >= T_k},   T_k = floor(2^32 sum_{j <= k} e^-1 / j!)

Per-row loss l and dY of member m's output row y against the target row t (s = the launch's ``scale``):

    MSE:       l = sum_c (y_c - t_c)^2,                                      dy_c = w 2 (y_c - t_c) s
    Gaussian:  l = sum_{c < od+1} ((y_c - t_c)^2 exp(-lv_c) + lv_c) + (y_{od+1} - t_{od+1})^2, dY as
               ``GaussOracleDynamics.nll_terms`` states it, every component times w

The weighted train step: loss = sum_m sum_r w_m(r) l_m(r) / (B (od + 2)) -- divided by the batch, not by sum w -- the
backward pass through the layers and Adam exactly as the two base oracles do them.
"""
from __future__ import annotations

import math

import numpy as np

from gauss_dynamics_oracle import GaussOracleDynamics, sigmoid
from model_env_oracle import OracleDynamics, _f64
from replay_weighted_util import philox4x32_10

BOOT_STREAM = 17
POISSON_P = [math.exp(-1.0) / math.factorial(k) for k in range(8)]  # P(w = k), k = 0 .. 7 (the rest, ~1e-6, is w = 8)
BOOT_T = [int(math.floor(4294967296.0 * sum(POISSON_P[:k + 1]))) for k in range(8)]


def boot_weights(seed: int, idx, n_members: int) -> np.ndarray:
    """``[n_members, len(idx)]`` float64 bootstrap weights of the dataset rows ``idx``."""
    idx = np.asarray(idx, np.int64).reshape(-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = np.zeros((n_members, idx.size))
    thr = np.asarray(BOOT_T, np.uint64)
    for m in range(n_members):
        ctr = np.stack([idx & 0xFFFFFFFF, np.full(idx.size, m), np.zeros(idx.size, np.int64),
                        np.full(idx.size, BOOT_STREAM)], 1).astype(np.uint32)
        word = philox4x32_10(ctr, seed & 0xFFFFFFFF, seed >> 32)[:, 0].astype(np.uint64)
        out[m] = (word[:, None] >= thr[None, :]).sum(1)
    return out


def member_loss(y, target, kind: str, scale: float, w=None, lo: float = 0.0, hi: float = 0.0):
    """(row_loss ``[M, rows]`` unweighted, dy ``[M, rows, NL]`` weighted) of the members' outputs ``y [M, rows, NL]``
    against ``target [rows, od + 2]``; ``w`` ``[M, rows]`` or None (every weight 1); ``kind`` "mse" | "gauss"."""
    y, t = _f64(y), _f64(target)
    M, rows, _ = y.shape
    no = t.shape[1]
    w = np.ones((M, rows)) if w is None else _f64(w)
    dy = np.zeros_like(y)
    if kind == "mse":
        d = y - t[None]
        l = (d * d).sum(2)
        dy = 2.0 * d * scale
    else:
        P = no - 1
        mu, cost, raw = y[..., :P], y[..., P], y[..., no:]
        lv1 = hi - (np.maximum(hi - raw, 0.0) + np.log1p(np.exp(-np.abs(hi - raw))))
        x = lv1 - lo
        lv = lo + (np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x))))
        d, iv = mu - t[None, :, :P], np.exp(-lv)
        dc = cost - t[None, :, P]
        l = (d * d * iv + lv).sum(2) + dc * dc
        dy[..., :P] = 2.0 * d * iv * scale
        dy[..., P] = 2.0 * dc * scale
        dy[..., no:] = (1.0 - d * d * iv) * sigmoid(hi - raw) * sigmoid(lv1 - lo) * scale
    return l, dy * w[..., None]


def weighted_stat(row_loss, w, stat_scale: float) -> float:
    return float(stat_scale * (np.asarray(row_loss) * np.asarray(w)).sum())


def elite_indices(losses, k: int):
    """The k members of lowest loss, ties to the lower index, ascending."""
    order = sorted(range(len(losses)), key=lambda i: (float(losses[i]), i))[:k]
    return sorted(order)


class _Ensemble:
    """What the deterministic and the Gaussian oracle share here (mixed into both)."""
    kind = "mse"
    boot_seed = None  # None: every weight is 1 (a model without bootstrap)

    def _bounds(self):
        return (self.lo, self.hi) if self.kind == "gauss" else (0.0, 0.0)

    def weights(self, row_ids, rows: int) -> np.ndarray:
        if self.boot_seed is None or row_ids is None:
            return np.ones((self.M, rows))
        return boot_weights(self.boot_seed, row_ids, self.M)

    def outputs(self, obs, act, keep=None) -> np.ndarray:
        x = self.inputs(obs, act)
        ys = []
        for m in range(self.M):
            k: list = []
            ys.append(self.net(m, x, k))
            if keep is not None:
                keep.append(k)
        return np.stack(ys)

    def weighted_loss_and_grads(self, obs, nobs, act, rew, cost, row_ids=None):
        tg = self.targets(obs, nobs, rew, cost)
        s = 1.0 / tg.size
        keep: list = []
        y = self.outputs(obs, act, keep)
        w = self.weights(row_ids, tg.shape[0])
        l, dy = member_loss(y, tg, self.kind, s, w, *self._bounds())
        g = {}
        for m in range(self.M):
            dz = dy[m]
            for i in reversed(range(self.n_layers)):
                W, _ = self._wb(m, i)
                g[f"members.{m}.{2 * i}.weight"] = dz.T @ keep[m][i]
                g[f"members.{m}.{2 * i}.bias"] = dz.sum(0)
                if i > 0:
                    dz = (dz @ W) * (keep[m][i] > 0.0)
        return weighted_stat(l, w, s), g

    def boot_step(self, obs, nobs, act, rew, cost, row_ids=None):
        """One weighted train step (Adam as the base oracle's ``step``)."""
        loss, g = self.weighted_loss_and_grads(obs, nobs, act, rew, cost, row_ids)
        self.t += 1
        b1, b2, eps = 0.9, 0.999, 1e-8
        bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
        for k in self.train_keys:
            self.m[k] = b1 * self.m[k] + (1 - b1) * g[k]
            self.v[k] = b2 * self.v[k] + (1 - b2) * g[k] * g[k]
            self.p[k] = self.p[k] - (self.lr / bc1) * self.m[k] / (np.sqrt(self.v[k]) / math.sqrt(bc2) + eps)
        return {"loss/dynamics_loss": loss}

    def validate(self, obs, nobs, act, rew, cost) -> np.ndarray:
        """Per member the unweighted mean loss sum_r l_m(r) / (rows (od + 2))."""
        tg = self.targets(obs, nobs, rew, cost)
        l, _ = member_loss(self.outputs(obs, act), tg, self.kind, 1.0, None, *self._bounds())
        return l.sum(1) / tg.size

    def select_elites(self, k: int, *batch):
        return elite_indices(self.validate(*batch), k)


class EnsembleOracle(_Ensemble, OracleDynamics):
    kind = "mse"

    def __init__(self, state_dict, lr: float = 1e-3, boot_seed=None):
        sd = {k: v for k, v in state_dict.items() if k not in ("boot_seed", "elites")}
        OracleDynamics.__init__(self, sd, lr)
        self.boot_seed = boot_seed


class GaussEnsembleOracle(_Ensemble, GaussOracleDynamics):
    kind = "gauss"

    def __init__(self, state_dict, lr: float = 1e-3, boot_seed=None):
        sd = {k: v for k, v in state_dict.items() if k not in ("boot_seed", "elites")}
        GaussOracleDynamics.__init__(self, sd, lr)
        self.boot_seed = boot_seed


def make_oracle(state_dict, lr: float = 1e-3, boot_seed=None):
    return (GaussEnsembleOracle if "logvar_min" in state_dict else EnsembleOracle)(state_dict, lr, boot_seed)
