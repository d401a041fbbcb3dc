"""Torch-CPU fp64 restatement of fitted Q evaluation: one step and the value read-out (TEST INFRASTRUCTURE ONLY).

One step, for the reward ensemble (x = rewards) and the cost ensemble (x = costs), member e against its OWN target member:

    backup_e = x + gamma (1 - done) Q_targ_e(s', pi(s'))              (no gradient)
    loss     = sum_e mean_rows (Q_e(s, a) - backup_e)^2               (EnsembleQCritic.loss, osrl/common/net.py:240-242)

then Adam (betas 0.9 / 0.999, eps 1e-8, bias-corrected as torch.optim.Adam) and the Polyak step
``target <- tau * theta_new + (1 - tau) * target`` -- the order of the fused optimizer kernel (csrc/adam.h).  Gradients come
from autograd; the optimizer is written out.  The policy's action is a callable: ``policy_action`` builds it from the numpy
policy restatements of oracle/osrl_oracle.py and oracle/coptidice_oracle.py.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional

import numpy as np
import torch

ENSEMBLES = ("critic", "cost_critic")


def policy_action(kind: str, params: Dict[str, np.ndarray], max_action: float, **kw) -> Callable:
    """``f(obs [n, od], z) -> action [n, ad]`` (fp64 numpy): what ``model.act`` does deterministically for ``kind``."""
    from oracle.coptidice_oracle import OracleCOptiDICE
    from oracle.osrl_oracle import OracleBC, OracleBCQL, OracleCPQ
    f64 = np.float64
    if kind == "bc":
        o = OracleBC(params, max_action, dtype=f64)
        return lambda obs, z=None: o.act(obs)
    if kind == "cpq":
        o = OracleCPQ(params, max_action=max_action, dtype=f64)
        return lambda obs, z=None: o.act(obs)
    if kind == "dice":
        o = OracleCOptiDICE(params, max_action=max_action, dtype=f64, **kw)
        return lambda obs, z=None: o.act(obs)
    if kind == "bcql":
        o = OracleBCQL(params, max_action=max_action, dtype=f64, **kw)
        return lambda obs, z: o.act(obs, z)  # (clamps z to +-0.5 itself)
    raise ValueError(kind)


def _f64(v) -> torch.Tensor:
    if torch.is_tensor(v):
        return v.detach().to(device="cpu", dtype=torch.float64).clone()
    return torch.as_tensor(np.asarray(v), dtype=torch.float64).clone()


def _n_layers(sd, prefix: str) -> int:
    return len({k[len(prefix) + 1:].split(".")[0] for k in sd if k.startswith(prefix + ".")})


class OracleFQE:
    def __init__(self, state_dict: Dict[str, "np.ndarray | torch.Tensor"], act: Callable, gamma: float = 0.99,
                 tau: float = 0.005, lr: float = 1e-3):
        self.p = {k: _f64(v) for k, v in state_dict.items()}
        self.act, self.gamma, self.tau, self.lr = act, float(gamma), float(tau), float(lr)
        self.num_q = len({k.split(".")[2] for k in self.p if k.startswith("critic.q_nets.")})
        self.train_keys = [k for k in self.p if k.split(".")[0] in ENSEMBLES]
        self.m = {k: torch.zeros_like(self.p[k]) for k in self.train_keys}
        self.v = {k: torch.zeros_like(self.p[k]) for k in self.train_keys}
        self.t = 0

    def q(self, ens: str, e: int, x: torch.Tensor, p=None) -> torch.Tensor:
        """Member ``e`` of ensemble ``ens`` on rows ``x`` -> [rows]  (mlp() of net.py:12-30, ReLU hidden layers)."""
        p = self.p if p is None else p
        pre = f"{ens}.q_nets.{e}"
        n = _n_layers(p, pre)
        for i in range(n):
            x = x @ p[f"{pre}.{2 * i}.weight"].T + p[f"{pre}.{2 * i}.bias"]
            if i < n - 1:
                x = torch.relu(x)
        return x[:, 0]

    def backups(self, nobs, rew, cost, done, z=None):
        """{ensemble: [num_q, rows]} -- member e bootstraps from target member e."""
        a_next = torch.as_tensor(np.asarray(self.act(np.asarray(nobs, np.float64), z)), dtype=torch.float64)
        xn = torch.cat([torch.as_tensor(np.asarray(nobs), dtype=torch.float64), a_next], 1)
        out = {}
        with torch.no_grad():
            for ens, x in zip(ENSEMBLES, (rew, cost)):
                x = torch.as_tensor(np.asarray(x), dtype=torch.float64).reshape(-1)
                nd = 1.0 - torch.as_tensor(np.asarray(done), dtype=torch.float64).reshape(-1)
                out[ens] = torch.stack([x + self.gamma * nd * self.q(ens + "_old", e, xn) for e in range(self.num_q)])
        return out

    def losses_and_grads(self, obs, nobs, act, rew, cost, done, z=None):
        leaves = {k: self.p[k].clone().requires_grad_(True) for k in self.train_keys}
        x = torch.cat([torch.as_tensor(np.asarray(obs), dtype=torch.float64),
                       torch.as_tensor(np.asarray(act), dtype=torch.float64)], 1)
        bk = self.backups(nobs, rew, cost, done, z)
        loss = {ens: sum(((self.q(ens, e, x, leaves) - bk[ens][e]) ** 2).mean() for e in range(self.num_q))
                for ens in ENSEMBLES}
        (loss["critic"] + loss["cost_critic"]).backward()
        return {k: float(v.detach()) for k, v in loss.items()}, {k: leaves[k].grad for k in self.train_keys}

    def step(self, obs, nobs, act, rew, cost, done, z=None) -> Dict[str, float]:
        loss, g = self.losses_and_grads(obs, nobs, act, rew, cost, done, z)
        self.t += 1
        b1, b2, eps = 0.9, 0.999, 1e-8
        bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
        for k in self.train_keys:
            self.m[k] = b1 * self.m[k] + (1 - b1) * g[k]
            self.v[k] = b2 * self.v[k] + (1 - b2) * g[k] * g[k]
            self.p[k] = self.p[k] - (self.lr / bc1) * self.m[k] / (self.v[k].sqrt() / math.sqrt(bc2) + eps)
            ens, rest = k.split(".", 1)
            kt = f"{ens}_old.{rest}"
            self.p[kt] = self.tau * self.p[k] + (1 - self.tau) * self.p[kt]
        return {"loss/fqe_reward_loss": loss["critic"], "loss/fqe_cost_loss": loss["cost_critic"]}

    def estimate(self, s0, z=None, reward_scale: float = 1.0, cost_scale: float = 1.0):
        """(value, value_std, cost_value, cost_value_std, n_init): mean / population std over members of the members'
        mean Q(s0, pi(s0)), rescaled."""
        s0 = np.asarray(s0, np.float64)
        a0 = torch.as_tensor(np.asarray(self.act(s0, z)), dtype=torch.float64)
        x = torch.cat([torch.as_tensor(s0), a0], 1)
        with torch.no_grad():
            r = np.array([float(self.q("critic", e, x).mean()) for e in range(self.num_q)]) / reward_scale
            c = np.array([float(self.q("cost_critic", e, x).mean()) for e in range(self.num_q)]) / cost_scale
        return float(r.mean()), float(r.std()), float(c.mean()), float(c.std()), int(s0.shape[0])
