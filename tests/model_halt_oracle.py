"""Numpy fp64 restatement of the pessimistic environment step and of a halting rollout (TEST INFRASTRUCTURE ONLY):
``OracleDynamics`` / ``GaussOracleDynamics`` with csrc/model_env.hip's kPess semantics on top of ``env_step``.

Per row, u the signal in use (d, or the largest predicted std under "max_std") and c = yh[od + 1]:

    cost = (c + kappa u if kappa != 0 else c) > 0.5
    halt = u > threshold                                   (strict; +inf never halts)
    on halt: reward = halt_reward, cost = halt_cost, the episode ends after this step, halt_step = the step;
             a recorded row has terminals = 1, timeouts = 0 -- also at the last step
    the next state, and u in the (max, sum) pair and per row, are the halting step's own

``rollout`` runs E episodes T steps under given actions and returns the padded episode-major tables, the totals, the
lengths, ``halt_step``, the offsets and the dense tables by plain slicing.
"""
from __future__ import annotations

import numpy as np

from gauss_dynamics_oracle import GaussOracleDynamics
from model_env_oracle import OracleDynamics, _f64

KEYS = ("observations", "actions", "next_observations", "rewards", "costs", "terminals", "timeouts")


class _Halting:
    def pess_step(self, s, a, threshold=np.inf, halt_reward=0.0, halt_cost=1.0, kappa=0.0, **kw):
        """``env_step``'s dict plus ``u``, ``cost_eff`` (what is held against 0.5), ``halt``; ``reward`` / ``cost`` are
        the pessimistic step's."""
        out = self.env_step(s, a, **kw)
        u = out["u"] if "u" in out else out["d"]
        eff = out["cost_raw"] + kappa * u if kappa != 0.0 else out["cost_raw"]
        halt = u > threshold
        out.update(u=u, cost_eff=eff, halt=halt, model_reward=out["reward"],
                   reward=np.where(halt, float(halt_reward), out["reward"]),
                   cost=np.where(halt, float(halt_cost), (eff > 0.5).astype(np.float64)))
        return out

    def rollout(self, s0, actions, threshold=np.inf, halt_reward=0.0, halt_cost=1.0, kappa=0.0, cost_scale=1.0,
                gamma=1.0, max_action=1.0, **kw):
        """``actions`` [T, E, ad] (clipped here as the step clips them).  Padded tables [E, T, ..] (rows past an
        episode's end are NaN), ``acc`` [E, 4], ``unc`` [E, 2], ``disc`` [E, 2], ``lengths``, ``halt_step``, ``offsets``
        [E + 1], ``row_u`` / ``cost_eff`` [E, T], ``state`` (the last one written), and ``dense``: the live rows."""
        s = _f64(s0).copy()
        T, E, ad = actions.shape
        od = self.od
        pad = {k: np.full((E, T) + ((od,) if "obs" in k else (ad,) if k == "actions" else ()), np.nan) for k in KEYS}
        row_u, eff = np.full((E, T), np.nan), np.full((E, T), np.nan)
        acc, unc, disc = np.zeros((E, 4)), np.zeros((E, 2)), np.zeros((E, 2))
        halt_step = np.full(E, -1, np.int32)
        for t in range(T):
            live = np.flatnonzero(acc[:, 3] == 0.0)
            if live.size == 0:
                break
            a = np.clip(_f64(actions[t]), -max_action, max_action)
            sub = {k: (v[live] if v is not None and np.ndim(v) else v) for k, v in kw.items()}
            o = self.pess_step(s[live], a[live], threshold, halt_reward, halt_cost, kappa, max_action=max_action, **sub)
            last = t + 1 >= T
            pad["observations"][live, t], pad["actions"][live, t] = s[live], a[live]
            pad["next_observations"][live, t] = o["s_next"]
            pad["rewards"][live, t], pad["costs"][live, t] = o["reward"], o["cost"]
            pad["terminals"][live, t] = o["halt"].astype(np.float64)
            pad["timeouts"][live, t] = np.where(o["halt"], 0.0, float(last))
            row_u[live, t], eff[live, t] = o["u"], o["cost_eff"]
            s[live] = o["s_next"]
            acc[live, 0] += o["reward"]
            acc[live, 1] += o["cost"] * cost_scale
            acc[live, 2] += 1.0
            acc[live, 3] = np.where(o["halt"] | last, 1.0, 0.0)
            disc[live, 0] += gamma ** t * o["reward"]
            disc[live, 1] += gamma ** t * o["cost"] * cost_scale
            unc[live, 0] = np.maximum(unc[live, 0], o["u"])
            unc[live, 1] += o["u"]
            halt_step[live[o["halt"]]] = t
        lengths = acc[:, 2].astype(np.int64)
        return dict(pad=pad, acc=acc, unc=unc, disc=disc, lengths=lengths, halt_step=halt_step, row_u=row_u,
                    cost_eff=eff, state=s, **compact(pad, lengths, dict(row_u=row_u, cost_eff=eff)))


def compact(pad, lengths, extra=None):
    """Plain slicing: ``offsets`` [E + 1] and the live rows of every [E, T, ..] table, episode-major."""
    lengths = np.asarray(lengths, np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    cat = lambda v: np.concatenate([v[e, :n] for e, n in enumerate(lengths)], 0)
    return dict(offsets=offsets, dense={k: cat(v) for k, v in pad.items()},
                **{"dense_" + k: cat(v) for k, v in (extra or {}).items()})


class HaltOracleDynamics(_Halting, OracleDynamics):
    pass


class GaussHaltOracleDynamics(_Halting, GaussOracleDynamics):
    pass
