"""fp64 numpy restatement of the planning kernels (csrc/plan.hip; TEST INFRASTRUCTURE ONLY): the select rule of
``osrl_plan_select`` and the stores of ``osrl_plan_fanout``, written from DESIGN.md "Planning at act time" with plain loops.

The rule, per slot n with candidates k = 0 .. K - 1, J_k the discounted penalised return and C_k the discounted cost:
  valid k: neither J_k nor C_k is a NaN;  F = {valid k : C_k <= budget_n}.
  1. F non-empty, temperature == 0: k* = argmax_F J, ties to the lowest k; the action is row k*.
  2. F non-empty, temperature > 0 (MPPI): w_k = exp((J_k - J_k*) / temperature) on F (1 where J_k == J_k*),
     a = sum_F w_k a0_k / sum_F w_k; chosen is still k*.
  3. F empty: k* = argmin over the valid k of C, ties to the larger J, then to the lower k; the action is row k*.
  4. no valid k: k* = 0.
"""
import numpy as np


def select_slot(J, C, a0, budget, temperature):
    """One slot: ``J``, ``C`` ``[K]``, ``a0`` ``[K, ad]``.  Returns (action fp64 ``[ad]``, k*, |F|, copied) -- ``copied``
    says that the action is row k* itself (to be compared bit for bit)."""
    J, C, a0 = np.asarray(J, np.float64), np.asarray(C, np.float64), np.asarray(a0, np.float64)
    K = J.shape[0]
    valid = [k for k in range(K) if not (np.isnan(J[k]) or np.isnan(C[k]))]
    F = [k for k in valid if C[k] <= budget]
    if F:
        best = F[0]
        for k in F[1:]:
            if J[k] > J[best]:
                best = k
        if temperature > 0:
            num, den = np.zeros(a0.shape[1]), 0.0
            for k in F:
                with np.errstate(over="ignore", invalid="ignore"):
                    w = 1.0 if J[k] == J[best] else float(np.exp((J[k] - J[best]) / temperature))
                w = float(np.float32(w))  # (the device keeps the weight in fp32)
                if w == 0.0:
                    continue
                den += w
                num += w * a0[k]
            return num / den, best, len(F), False
        return a0[best].copy(), best, len(F), True
    if not valid:
        return a0[0].copy(), 0, 0, True
    best = valid[0]
    for k in valid[1:]:
        if C[k] < C[best] or (C[k] == C[best] and J[k] > J[best]):
            best = k
    return a0[best].copy(), best, 0, True


def select(J, C, a0, budget, temperature):
    """``J``, ``C`` ``[N, K]``, ``a0`` ``[N, K, ad]``, ``budget`` ``[N]``: (action fp64 ``[N, ad]``, chosen int32 ``[N]``,
    n_feasible int32 ``[N]``, copied bool ``[N]``)."""
    out = [select_slot(J[n], C[n], a0[n], float(budget[n]), float(temperature)) for n in range(len(budget))]
    return (np.stack([o[0] for o in out]), np.asarray([o[1] for o in out], np.int32),
            np.asarray([o[2] for o in out], np.int32), np.asarray([o[3] for o in out], bool))


def fanout(states, K, obs_before, halting):
    """What ``osrl_plan_fanout`` leaves: episode ``n * K + k`` holds ``states[n]`` as its state and in the first ``od``
    columns of its observation row (the other columns of ``obs_before`` stay), zero totals and disagreement sums,
    ``(0, 0, 1, 0)`` discounted sums and, on an environment that can halt, ``halt_step = -1`` (None otherwise: untouched)."""
    states = np.asarray(states, np.float32)
    N, od = states.shape
    E = N * K
    rows = np.repeat(states, K, axis=0)
    obs = np.array(obs_before, np.float32, copy=True)
    obs[:, :od] = rows
    disc = np.zeros((E, 4), np.float32)
    disc[:, 2] = 1.0
    return dict(state=rows, obs=obs, acc=np.zeros((E, 4), np.float32), unc=np.zeros((E, 2), np.float32), disc=disc,
                halt_step=np.full(E, -1, np.int32) if halting else None)
