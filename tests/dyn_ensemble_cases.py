"""Inputs and cases of the dynamics ensemble's bootstrap / holdout / elite tests (TEST INFRASTRUCTURE ONLY), plain numpy so
that tests/test_dyn_ensemble_cpu.py can check with the oracle alone what the GPU tests rely on.

Kernel cases ``(rows, od, n_nets)``, each run for both kinds -- the smallest shapes at which ``osrl_dyn_member_loss`` can
go wrong:
    rows   1, 17, 40, 333: one row, a partial 4-row workgroup (17 = 4 * 4 + 1, 333 = 4 * 83 + 1), 84 workgroups, so the
           statistic's last workgroup sums more partials than it has waves
    od     1, 17, 76, 256: the Gaussian's output width NL = 2 od + 3 is odd in every one; at od = 76 the Gaussian's NL = 155 needs a lane's second
           and third column; at od = 256 NL = 515 exceeds 512 and a lane owns five target columns
    nets   1, 5, 8 (OSRL_MAX_NETS)
The Gaussian cases carry raw log-variances at and beyond both clamp edges (the bounds of tests/gauss_dynamics_cases.py, and
+-50 / +-60 where exp overflows fp32 without the soft clamp's form).  ``idx`` holds 0, 2^24 - 1 and a duplicated row.
"""
import numpy as np

import gauss_dynamics_cases as GC
from dyn_ensemble_oracle import boot_weights

LOGVAR_MIN, LOGVAR_MAX = GC.LOGVAR_MIN, GC.LOGVAR_MAX
BOOT_SEED = 0x5DEECE66D1234567 & 0x7FFFFFFFFFFFFFFF  # both key halves non-zero
IDX_MAX = (1 << 24) - 1

KERNEL_CASES = [
    (1, 1, 1),
    (1, 256, 8),
    (17, 17, 5),
    (17, 256, 1),
    (40, 76, 8),
    (40, 1, 5),
    (333, 17, 8),
    (333, 76, 5),
    (333, 256, 5),
]
KINDS = ("mse", "gauss")


def width(od, kind):
    return 2 * od + 3 if kind == "gauss" else od + 2


def kernel_inputs(rows, od, n_nets, kind, seed=3):
    """(y [n_nets, rows, NL], target [rows, od + 2], idx int32 [rows]) of a kernel case."""
    rs = np.random.RandomState(seed + 1000 * rows + od)
    no = od + 2
    y = rs.randn(n_nets, rows, width(od, kind)).astype(np.float32)
    target = rs.randn(rows, no).astype(np.float32)
    target[:, no - 1] = (rs.rand(rows) > 0.5).astype(np.float32)  # the raw 0 / 1 cost
    if kind == "gauss":
        raw = rs.uniform(LOGVAR_MIN - 5.0, LOGVAR_MAX + 5.0, (n_nets, rows, od + 1)).astype(np.float32)
        edges = np.array([LOGVAR_MIN, LOGVAR_MAX, 50.0, -50.0, 60.0, -60.0, 0.0], np.float32)
        flat = raw.reshape(-1)
        flat[:min(flat.size, edges.size)] = edges[:flat.size]  # (row 0 of member 0 first: the rows = 1 case has them too)
        y[:, :, no:] = raw
    idx = rs.randint(0, IDX_MAX + 1, rows).astype(np.int32)
    idx[0] = 0
    idx[-1] = IDX_MAX if rows > 1 else 0
    if rows >= 3:
        idx[2] = idx[1]  # a row drawn twice
    return y, target, idx


# ---- a batch in which one member's weights are all zero -------------------------------------------------------------------
ZERO_MEMBER, ZERO_NETS, ZERO_ROWS, ZERO_OD = 2, 5, 17, 17


def zero_member_idx(rows=ZERO_ROWS, member=ZERO_MEMBER, n_nets=ZERO_NETS, seed=BOOT_SEED):
    """The first ``rows`` dataset rows i < 4096 with ``w_member(i) = 0`` under ``seed`` (host search): a batch of them
    leaves that member without a single weighted row."""
    w = boot_weights(seed, np.arange(4096), n_nets)
    idx = np.nonzero(w[member] == 0)[0][:rows]
    assert idx.size == rows
    return idx.astype(np.int32)


# ---- the statistical check of the weights ---------------------------------------------------------------------------------
MEAN_SEED, MEAN_ROWS, MEAN_NETS = 20240607, 12500, 8  # 100 000 (idx, m) pairs

# ---- the train step -------------------------------------------------------------------------------------------------------
TRAIN = dict(od=5, ad=2, hidden=[32, 32], M=3, B=40, steps=3, lr=1e-4)


def transitions(n, od, ad, seed=1):
    """A DSRL-layout dataset of ``n`` rows (fp32): smooth next states, shifted rewards, a third of the costs 1."""
    rs = np.random.RandomState(seed)
    obs = rs.randn(n, od).astype(np.float32)
    act = rs.uniform(-1.0, 1.0, (n, ad)).astype(np.float32)
    nobs = (obs + 0.3 * np.tanh(obs[:, ::-1] + act.sum(1, keepdims=True)) + 0.05 * rs.randn(n, od)).astype(np.float32)
    rew = (2.0 + 3.0 * np.sin(obs.sum(1)) + act[:, 0]).astype(np.float32)
    cost = (np.arange(n) % 3 == 0).astype(np.float32)
    z = np.zeros(n, np.float32)
    return dict(observations=obs, next_observations=nobs, actions=act, rewards=rew, costs=cost, terminals=z.copy(),
                timeouts=z.copy())


BATCH_KEYS = ("observations", "next_observations", "actions", "rewards", "costs")


# ---- elites in the environment --------------------------------------------------------------------------------------------
ENV = dict(od=11, ad=3, hidden=[40, 40], M=4, elites=[3, 0], E=17, steps=5)


def subset_state_dict(sd, members):
    """``sd`` restricted to ``members`` (ascending), renumbered 0 .. k-1: the small model that holds copies of them."""
    out = {k: v for k, v in sd.items() if not k.startswith("members.")}
    for j, m in enumerate(sorted(members)):
        for k, v in sd.items():
            if k.startswith(f"members.{m}."):
                out[f"members.{j}." + k.split(".", 2)[2]] = v
    return out
