"""Case data of the halting model rollouts' tests (TEST INFRASTRUCTURE ONLY), plain numpy: tests/test_model_halt_cpu.py
checks with the oracle alone what tests/test_gpu_model_halt.py relies on.

Weights, start rows and actions are tests/model_env_cases.py's / model_collect_cases.py's:
    A = (od 11, ad 3, [40, 40], M 3);  B = (od 37, ad 6, [24, 40], M 3): od > 32 is a thread's second kept column, 24 no
    multiple of 16.  Both: E = 19 (two tiles, the second partial), 12 steps, ``MC.actions``, mode "mean", clamp on,
    lambda = 0.5.
    G = A's shape as a Gaussian ensemble (gauss_dynamics_cases.py), uncertainty "max_std", ``sample`` with injected draws.

The threshold is not tuned by hand: it is the midpoint of the widest gap between consecutive sorted u values between the
80th and the 93rd percentile of the NON-halting oracle rollout, so that no halt decision sits near it.
"""
import functools

import numpy as np

import gauss_dynamics_cases as GC
import model_collect_cases as K
import model_env_cases as MC
from model_halt_oracle import GaussHaltOracleDynamics, HaltOracleDynamics

E = K.E
T = MC.T_STEPS
LAMBDA = K.LAMBDA
KAPPA = 0.5
HALT_REWARD = -2.5
HALT_COST = 1.0
CS = 2.0
GAMMA = float(np.float32(0.9))
CASES = dict(K.CASES, G=dict(K.CASES["A"]))
NAMES = ("A", "B", "G")


def state_dict(case):
    c = CASES[case]
    if case == "G":
        return GC.gauss_state_dict(c["od"], c["ad"], c["hidden"], c["M"])
    return MC.dyn_state_dict(c["od"], c["ad"], c["hidden"], c["M"], K.DYN_SEED[case])


def step_kw(case, n=E):
    """What every step of the case takes beside the pessimistic arguments (oracle keywords)."""
    kw = dict(mode="mean", clamp=True, lam=LAMBDA)
    if case == "G":
        kw.update(sample=True, uncertainty="max_std", eps=GC.noise(n, CASES[case]["od"] + 1))
    return kw


def oracle(case):
    return (GaussHaltOracleDynamics if case == "G" else HaltOracleDynamics)(state_dict(case))


def actions(case, n=E, steps=T, acts="mc"):
    """[steps, n, ad]: ``MC.actions`` ("mc"), or what the constant BC policy of model_collect_cases.py outputs ("const")."""
    ad = CASES[case]["ad"]
    if acts == "const":
        return np.broadcast_to(K.policy_out(ad, MC.MAX_ACTION), (steps, n, ad)).copy()
    return MC.actions(n, ad, steps=steps)


def starts(case, n=E):
    return MC.start_rows(n, CASES[case]["od"])


@functools.lru_cache(maxsize=None)
def free_rollout(case, n=E, acts="mc"):
    """The non-halting oracle rollout (threshold +inf, kappa 0)."""
    return oracle(case).rollout(starts(case, n), actions(case, n, acts=acts), cost_scale=CS, gamma=GAMMA,
                                max_action=MC.MAX_ACTION, **step_kw(case, n))


@functools.lru_cache(maxsize=None)
def threshold(case, acts="mc"):
    u = np.sort(free_rollout(case, acts=acts)["row_u"].reshape(-1))
    lo, hi = int(round(0.80 * (u.size - 1))), int(round(0.93 * (u.size - 1)))
    gaps = np.diff(u[lo:hi + 1])
    i = lo + int(np.argmax(gaps))
    return float(0.5 * (u[i] + u[i + 1]))


@functools.lru_cache(maxsize=None)
def halting_rollout(case, n=E, kappa=KAPPA, thr=None, acts="mc", cost_scale=CS):
    """The oracle rollout the GPU tests compare against: the case's threshold, kappa, halt reward and cost."""
    return oracle(case).rollout(starts(case, n), actions(case, n, acts=acts),
                                threshold(case, acts) if thr is None else thr, HALT_REWARD, HALT_COST, kappa,
                                cost_scale=cost_scale, gamma=GAMMA, max_action=MC.MAX_ACTION, **step_kw(case, n))
