"""Numpy restatement of the on-device collection (TEST INFRASTRUCTURE ONLY): the scalar ``SyntheticSafeEnv``, a policy
callable ``f(obs [n, od]) -> action [n, ad]`` (e.g. ``fqe_oracle.policy_action``) and injected noise.

Episode e starts at ``env.reset(seed=base_seed + e)``; at step t it applies ``a = clip(fp32(pi(s) + sigma_e * eps[t, e]))``
(``eps`` is not read where ``sigma_e == 0``) and records the row ``e * L + t`` of a DSRL-layout dataset: the state before
the step, the clipped action, the next state, reward, raw 0 / 1 cost, ``terminals = 0``, ``timeouts = (t + 1 >= L)``.
The sums are fp64: returns, cost returns * cost_scale, lengths, and both weighed by ``gamma ** t``."""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional

import numpy as np


class OracleCollected(NamedTuple):
    dataset: Dict[str, np.ndarray]
    returns: np.ndarray
    cost_returns: np.ndarray
    lengths: np.ndarray
    disc_returns: np.ndarray
    disc_cost_returns: np.ndarray


def collect(make_env: Callable, policy: Callable, base_seed: int, episodes: int, episode_len: int, sigma=0.0,
            eps: Optional[np.ndarray] = None, gamma: float = 1.0, cost_scale: float = 1.0,
            extra_obs: Optional[float] = None) -> OracleCollected:
    """``make_env()`` -> a fresh ``SyntheticSafeEnv`` (one per episode); ``extra_obs``: a value appended to what the
    policy sees (BC multi-task's cost limit), never to what is recorded."""
    E, L = int(episodes), int(episode_len)
    envs = [make_env() for _ in range(E)]
    od, ad = envs[0].state_dim, envs[0].action_dim
    sigma = np.broadcast_to(np.asarray(sigma, np.float64), (E,))
    if eps is None and (sigma != 0).any():
        raise ValueError("sigma > 0 needs the injected noise eps [L, E, ad]")
    f = np.float32
    d = dict(observations=np.zeros((E * L, od), f), actions=np.zeros((E * L, ad), f),
             next_observations=np.zeros((E * L, od), f), rewards=np.zeros(E * L, f), costs=np.zeros(E * L, f),
             terminals=np.zeros(E * L, f), timeouts=np.zeros(E * L, f))
    obs = np.stack([env.reset(seed=base_seed + e)[0] for e, env in enumerate(envs)])
    tot = np.zeros((5, E))
    for t in range(L):
        x = obs if extra_obs is None else np.concatenate([obs, np.full((E, 1), extra_obs, obs.dtype)], 1)
        a = np.asarray(policy(x.astype(np.float64)), np.float64)
        for e, env in enumerate(envs):
            ae = a[e] + sigma[e] * np.asarray(eps[t, e], np.float64) if sigma[e] != 0 else a[e]
            ae = np.clip(ae.astype(f), -env.max_action, env.max_action).astype(f)
            o2, r, term, trunc, info = env.step(ae)
            row = e * L + t
            d["observations"][row], d["actions"][row], d["next_observations"][row] = obs[e], ae, o2
            d["rewards"][row], d["costs"][row] = r, info["cost"]
            d["timeouts"][row] = float(t + 1 >= L)
            r32, c32 = float(d["rewards"][row]), float(d["costs"][row])
            tot[:, e] += (r32, c32 * cost_scale, 1.0, gamma ** t * r32, gamma ** t * c32 * cost_scale)
            obs[e] = o2
    return OracleCollected(d, tot[0], tot[1], tot[2], tot[3], tot[4])
