"""The weights, tables, initial states and actions of the learned-dynamics environment's GPU parity tests (TEST
INFRASTRUCTURE ONLY), as plain numpy so that tests/test_model_env_cpu.py can check on the CPU, with the oracle alone, what the
GPU tests rely on: both cost values occur and at most 2 % of the rows sit within 1e-3 of the 0.5 threshold."""
import numpy as np

T_STEPS = 12
MAX_ACTION = 1.0
N_INIT = 7  # initial-state rows: fewer than any E of interest but 3, so episodes wrap around them
# (E, od, ad, hidden, M, mode, member, clamp, lambda): every E, shape, depth and M of the issue; MEAN and MEMBER, with
# and without the clamp, with lambda = 0 and 0.5
PARITY = [
    (3, 11, 3, [40, 40], 1, "mean", 0, True, 0.0),
    (19, 11, 3, [40, 40], 3, "member", 2, False, 0.5),
    (40, 17, 6, [272, 64, 40], 5, "mean", 0, True, 0.5),
    (40, 11, 3, [40, 40, 40], 3, "member", 1, True, 0.0),
    (19, 17, 6, [40, 40], 5, "mean", 0, False, 0.0),
    (3, 17, 6, [272, 64, 40], 3, "member", 0, False, 0.5),
]
SEED = 7


def dyn_state_dict(od, ad, hidden, M, seed=SEED):
    """fp32 numpy ``state_dict`` of a ``Dynamics``: nn.Linear-style uniform weights, the cost head spread around the
    threshold (bias 0.5, weights x 3; every layer at gain 1.7 so that the rows differ), random normaliser tables, bounds that the free rollout reaches."""
    rs = np.random.RandomState(seed)
    sizes = [od + ad] + list(hidden) + [od + 2]
    sd = {}
    for m in range(M):
        for i in range(len(sizes) - 1):
            k = 1.7 / np.sqrt(sizes[i])
            W = rs.uniform(-k, k, (sizes[i + 1], sizes[i]))
            b = rs.uniform(-k, k, sizes[i + 1])
            if i == len(sizes) - 2:
                W[od + 1] *= 3.0
                b[od + 1] = 0.5
            sd[f"members.{m}.{2 * i}.weight"], sd[f"members.{m}.{2 * i}.bias"] = W, b
    sd.update(mu_s=0.3 * rs.randn(od), sd_s=0.5 + rs.rand(od), mu_d=0.05 * rs.randn(od), sd_d=0.1 + 0.3 * rs.rand(od),
              mu_r=rs.randn(1), sd_r=0.5 + rs.rand(1), s_lo=-0.8 * np.ones(od), s_hi=0.8 * np.ones(od))
    return {k: np.asarray(v, np.float32) for k, v in sd.items()}


def init_states(od, seed=SEED):
    return (0.6 * np.random.RandomState(seed + 1).randn(N_INIT, od)).astype(np.float32)


def actions(E, ad, seed=SEED, steps=T_STEPS):
    """[steps, E, ad] in +-1.5: a third of them are clipped.  Episode e's actions do not depend on E."""
    return np.random.RandomState(seed + 2).uniform(-1.5, 1.5, (steps, 64, ad)).astype(np.float32)[:, :E]


def start_rows(E, od, base_seed=0, seed=SEED):
    return init_states(od, seed)[(base_seed + np.arange(E)) % N_INIT]
