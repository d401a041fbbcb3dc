"""Numpy restatement of ``CDTTrainer.collect_targets`` (TEST INFRASTRUCTURE ONLY): the closed loop of
tests/test_gpu_data_eval.py::test_cdt_batched_evaluate_matches_oracle_rollouts over the scalar ``SyntheticSafeEnv``, with
``OracleCDT.forward``'s ``mu`` / ``ls``, per-episode targets and injected noise, recorded like tests/collect_oracle.py.

Episode e starts at ``env.reset(seed=base_seed + e)``; at step t the oracle sees the last ``T`` steps (zero padded on the
right, as the device window is) and the action is ``clip(fp32(mu + s * eps[t, e]))`` at the last filled position, with
``s = sigma_e`` or, with ``sample``, ``exp(ls)``; ``eps`` is not read where ``s == 0``.  The to-go values follow
``R <- R - reward`` and ``C <- C - cost * cost_scale`` (``1 - cost`` under ``cost_reverse``), rounded to fp32 per step.

Also here: the shapes and seeds the CPU and the GPU tests of the feature share, and ``teacher_forced``, which rebuilds every
step's window from recorded rows and returns the oracle's head values there."""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np

from cases import CDT_CASES, CDTCase
from collect_oracle import OracleCollected

EL = 23           # one 20-step graph replay and one that overshoots by 17; the windows (T = 4, 5) slide from step T on
ENV_SEED = 3      # (test_cdt_collect_cpu.py checks this env's margin at the cost threshold for both stochastic shapes)
BASE_SEED = 100
COST_SCALE = 2.0
TARGETS = (30.0, 5.0)

# od 70: two waves in the environment step; ad 6: a second Philox counter for columns 4-5; the prefix token reads the
# per-episode cost target; 33 episodes fill no tile
BIG = CDTCase("cdt_collect_big", od=70, ad=6, B=33, T=5, E=16, heads=2, layers=1, episode_len=EL, cost_prefix=True, seed=21)
EPISODES = {"cdt_small": 5, "cdt_collect_big": 33, "cdt_v_prefix_det": 5}


def case(name: str) -> CDTCase:
    """The case with a time-step table long enough for ``EL`` steps (its weights are then this file's own draw)."""
    return BIG if name == BIG.name else dataclasses.replace(CDT_CASES[name], episode_len=EL)


def make_env(c: CDTCase, init_noise: float = 0.5):
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    return SyntheticSafeEnv(c.od, c.ad, EL, seed=ENV_SEED, init_noise=init_noise)


def _heads(o, S, A, R, C, TS, M, ec):
    res, _ = o.forward(S, A, R, C, TS, M, episode_cost=ec)
    return (res["mu"], res["ls"]) if o.stochastic else (res["act"], None)


def collect(o, make_env, base_seed: int, episodes: int, episode_len: int, target_return, target_cost, sigma=0.0,
            sample: bool = False, eps: Optional[np.ndarray] = None, gamma: float = 1.0, cost_scale: float = 1.0,
            cost_reverse: bool = False) -> OracleCollected:
    """``o``: an ``OracleCDT``; ``make_env()`` -> a fresh ``SyntheticSafeEnv``.  Targets: scalars or one per episode."""
    E, L, T = int(episodes), int(episode_len), o.T
    f = np.float32
    trs = np.broadcast_to(np.asarray(target_return, f), (E,))
    tcs = np.broadcast_to(np.asarray(target_cost, f), (E,))
    sigma = np.broadcast_to(np.asarray(sigma, np.float64), (E,))
    if eps is None and (sample or (sigma != 0).any()):
        raise ValueError("noise needs the injected eps [L, E, ad]")
    env = make_env()
    od, ad = env.state_dim, env.action_dim
    d = dict(observations=np.zeros((E * L, od), f), actions=np.zeros((E * L, ad), f),
             next_observations=np.zeros((E * L, od), f), rewards=np.zeros(E * L, f), costs=np.zeros(E * L, f),
             terminals=np.zeros(E * L, f), timeouts=np.zeros(E * L, f))
    tot = np.zeros((5, E))
    for e in range(E):
        env = make_env()
        S, A = np.zeros((L + 1, od), f), np.zeros((L, ad), f)
        R, C = np.zeros(L + 1, f), np.zeros(L + 1, f)
        obs, _ = env.reset(seed=base_seed + e)
        S[0], R[0], C[0] = obs, trs[e], tcs[e]
        for step in range(L):
            lo = max(0, step + 1 - T)
            n = step + 1 - lo
            pad = lambda x: np.concatenate([x, np.zeros((T - n,) + x.shape[1:], x.dtype)])[None]  # noqa: E731
            mu, ls = _heads(o, pad(S[lo:step + 1]), pad(A[lo:step + 1]), pad(R[lo:step + 1]), pad(C[lo:step + 1]),
                            pad(np.arange(lo, step + 1)), pad(np.ones(n, f)), np.array([tcs[e]], f))
            a = mu[0, n - 1]
            s = np.exp(ls[0, n - 1].astype(np.float64)) if sample else np.full(ad, sigma[e])
            if (s != 0).any():
                a64 = a.astype(np.float64)
                nz = s != 0
                a64[nz] += s[nz] * np.asarray(eps[step, e], np.float64)[nz]
                a = a64.astype(f)
            act = np.clip(a, -env.max_action, env.max_action).astype(f)
            o2, reward, term, trunc, info = env.step(act)
            row = e * L + step
            d["observations"][row], d["actions"][row], d["next_observations"][row] = S[step], act, o2
            d["rewards"][row], d["costs"][row] = reward, info["cost"]
            d["timeouts"][row] = float(step + 1 >= L)
            A[step], S[step + 1] = act, o2
            cw = ((1.0 - info["cost"]) if cost_reverse else info["cost"]) * cost_scale
            R[step + 1], C[step + 1] = R[step] - reward, C[step] - cw
            r32, c32 = float(d["rewards"][row]), float(d["costs"][row])
            tot[:, e] += (r32, c32 * cost_scale, 1.0, gamma ** step * r32, gamma ** step * c32 * cost_scale)
    return OracleCollected(d, tot[0], tot[1], tot[2], tot[3], tot[4])


def teacher_forced(o, d, episodes: int, episode_len: int, target_return, target_cost, cost_scale: float = 1.0,
                   cost_reverse: bool = False):
    """(mu [E, L, ad], ls [E, L, ad] or None): the oracle's head at the position acted from, on the window rebuilt at
    every step from the recorded rows ``d`` -- states, recorded actions, ``R[t+1] = fp32(R[t] - r)``,
    ``C[t+1] = fp32(C[t] - cost_scale * c)`` from the episode's own targets, time steps."""
    E, L, T = int(episodes), int(episode_len), o.T
    f = np.float32
    S = d["observations"].reshape(E, L, -1)
    A = d["actions"].reshape(E, L, -1)
    r, c = d["rewards"].reshape(E, L), d["costs"].reshape(E, L)
    cw = ((1 - c) if cost_reverse else c).astype(f) * f(cost_scale)
    tcs = np.broadcast_to(np.asarray(target_cost, f), (E,)).copy()
    R, C = np.zeros((E, L + 1), f), np.zeros((E, L + 1), f)
    R[:, 0], C[:, 0] = np.broadcast_to(np.asarray(target_return, f), (E,)), tcs
    for t in range(L):
        R[:, t + 1], C[:, t + 1] = R[:, t] - r[:, t], C[:, t] - cw[:, t]
    mu, ls = np.zeros(A.shape), np.zeros(A.shape)
    for step in range(L):
        lo = max(0, step + 1 - T)
        n = step + 1 - lo
        pad = lambda x: np.concatenate([x, np.zeros((E, T - n) + x.shape[2:], x.dtype)], 1)  # noqa: E731
        Aw = A[:, lo:step + 1].copy()
        Aw[:, n - 1] = 0  # the step being decided holds the zero dummy action
        m, s = _heads(o, pad(S[:, lo:step + 1]), pad(Aw), pad(R[:, lo:step + 1]), pad(C[:, lo:step + 1]),
                      pad(np.broadcast_to(np.arange(lo, step + 1), (E, n))), pad(np.ones((E, n), f)), tcs)
        mu[:, step] = m[:, n - 1]
        if s is not None:
            ls[:, step] = s[:, n - 1]
    return mu, (ls if o.stochastic else None)
