"""Weights, noise and cases of the Gaussian dynamics ensemble's tests (TEST INFRASTRUCTURE ONLY), as plain numpy so that
tests/test_gauss_dynamics_cpu.py can check with the oracle alone what the GPU tests rely on.

The members are ``model_env_cases.dyn_state_dict``'s -- the same first od + 2 output rows, bit for bit -- with od + 1
log-variance rows appended to the last layer.  Those rows are scaled so that the raw log-variances cross both bounds
(LOGVAR_MIN / LOGVAR_MAX, the model's defaults): biases spread over [lo - 5, hi + 5] column by column, weights at three
times nn.Linear's range so that a column moves with the input too.

Shapes, the smallest that reach every edge (output width 2 od + 3):
    (11, 3, [40, 40]) M = 1 and 3   25 wide: the log-variance block straddles a 16-column tile
    (15, 2, [40, 40]) M = 3         33 wide: P = od + 1 = 16, the cost column opens a tile
    (17, 6, [272, 64, 40]) M = 5    37 wide
    (40, 2, [48]) M = 2             83 wide: od > 32, a thread of the step's epilogue owns more than one column
"""
import numpy as np

import model_env_cases as MC

T_STEPS = MC.T_STEPS
MAX_ACTION = MC.MAX_ACTION
SEED = MC.SEED
LOGVAR_MIN, LOGVAR_MAX = -10.0, 0.5
E_ALL = (3, 19, 40)

SHAPES = [
    (11, 3, [40, 40], 1),
    (11, 3, [40, 40], 3),
    (15, 2, [40, 40], 3),
    (17, 6, [272, 64, 40], 5),
    (40, 2, [48], 2),
]
# (E, od, ad, hidden, M, mode, member, clamp, lambda, uncertainty, seed of the weights): every shape and E; MEAN, MEMBER
# and RANDOM (with member_in), both signals, with and without the clamp, lambda 0 and 0.5.  (The first case has 36 rows:
# the 2 % cap on rows near the cost threshold allows none, and seed 7 has one; seed 8 leaves 1 % of its 12 log-variance
# columns above the upper bound.)
PARITY = [
    (3, 11, 3, [40, 40], 1, "mean", 0, True, 0.5, "max_std", SEED + 2),
    (19, 11, 3, [40, 40], 3, "member", 2, False, 0.5, "disagreement", SEED),
    (40, 11, 3, [40, 40], 3, "random", 0, True, 0.0, "max_std", SEED),
    (19, 15, 2, [40, 40], 3, "mean", 0, True, 0.5, "disagreement", SEED),
    (40, 15, 2, [40, 40], 3, "random", 0, False, 0.5, "max_std", SEED),
    (40, 17, 6, [272, 64, 40], 5, "mean", 0, True, 0.5, "max_std", SEED),
    (3, 17, 6, [272, 64, 40], 5, "member", 4, False, 0.0, "disagreement", SEED),
    (19, 40, 2, [48], 2, "random", 0, True, 0.5, "max_std", SEED),
    (40, 40, 2, [48], 2, "mean", 0, False, 0.0, "disagreement", SEED),
]


def logvar_rows(od, width, M, seed=SEED):
    """Per member the (weight [od + 1, width], bias [od + 1]) of the raw log-variance columns."""
    rs = np.random.RandomState(seed + 100)
    out = []
    for _ in range(M):
        k = 3.0 * 1.7 / np.sqrt(width)
        W = rs.uniform(-k, k, (od + 1, width))
        b = rs.uniform(LOGVAR_MIN - 5.0, LOGVAR_MAX + 5.0, od + 1)
        out.append((W.astype(np.float32), b.astype(np.float32)))
    return out


def with_logvar_rows(sd, od, M, seed=SEED):
    """``sd`` (a deterministic model's fp32 numpy state_dict) with the log-variance rows appended and the bounds added."""
    sd = dict(sd)
    last = max(int(k.split(".")[2]) for k in sd if k.startswith("members.0."))
    width = sd[f"members.0.{last}.weight"].shape[1]
    for m, (W, b) in enumerate(logvar_rows(od, width, M, seed)):
        kw, kb = f"members.{m}.{last}.weight", f"members.{m}.{last}.bias"
        sd[kw] = np.concatenate([np.asarray(sd[kw], np.float32)[:od + 2], W], 0)
        sd[kb] = np.concatenate([np.asarray(sd[kb], np.float32)[:od + 2], b], 0)
    sd["logvar_min"] = np.array([LOGVAR_MIN], np.float32)
    sd["logvar_max"] = np.array([LOGVAR_MAX], np.float32)
    return sd


def gauss_state_dict(od, ad, hidden, M, seed=SEED):
    return with_logvar_rows(MC.dyn_state_dict(od, ad, hidden, M, seed), od, M, seed)


def mean_state_dict(od, ad, hidden, M, seed=SEED):
    """The deterministic model that holds the first od + 2 rows of every member's last layer."""
    return MC.dyn_state_dict(od, ad, hidden, M, seed)


def noise(E, P, seed=SEED):
    """[E, P] standard-normal draws; episode e's do not depend on E."""
    return np.random.RandomState(seed + 3).randn(64, P).astype(np.float32)[:E]


def noise_pm3(E, P, seed=SEED):
    """[E, P] draws at +-3: three predicted standard deviations either way."""
    return (3.0 * np.sign(np.random.RandomState(seed + 4).randn(64, P))).astype(np.float32)[:E]


def members_in(E, M):
    return ((np.arange(E) * 2 + 1) % M).astype(np.int32)
