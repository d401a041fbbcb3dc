"""Inputs of the planning tests (TEST INFRASTRUCTURE ONLY), as plain numpy: the synthetic (J, C, a0, budget) tables of the
select kernel's cases and the shapes of the fan-out and planner tests.

Every C is a multiple of 0.25 and every budget an integer plus 0.125, so no feasibility comparison sits on a rounding
edge; J values are multiples of 1/64 (exact in fp32) unless a case says otherwise."""
import numpy as np

N = 3
KS = (1, 5, 64, 65, 1024)   # 65 crosses a wave boundary, 1024 is OSRL_PLAN_MAX_CANDIDATES (four candidates per thread)
ADS = (1, 3)
H_TABLE = 2                 # rows per candidate in the synthetic action table: row 1 is poison and must not be read
MAX_ACTION = 1.0
SELECT_CASES = ("all_feasible", "one_feasible_last", "none_feasible", "equal_j", "spread_200", "nan_one", "all_nan")
# the fan-out and planner shapes
OD, AD, FAN_N, FAN_K = 5, 3, 3, 5
HORIZONS = (1, 3)
CS = 2.0                    # the collector's cost_scale in the planner tests


def _j(rs, n, k):
    return (rs.randint(-640, 640, (n, k)) / 64.0).astype(np.float32)


def select_case(name, K, ad, seed=0):
    """-> dict(J [N, K], C [N, K], a0 [N, K, ad], budget [N], temperatures: the values to run the case at)."""
    rs = np.random.RandomState(seed + 1000 * K + ad)
    a0 = rs.uniform(-MAX_ACTION, MAX_ACTION, (N, K, ad)).astype(np.float32)
    k = np.arange(K)[None, :] + np.arange(N)[:, None]  # (the pattern shifts with the slot)
    J = _j(rs, N, K)
    temps = (0.0, 0.5)
    if name == "all_feasible":
        C, budget = 0.25 * (k % 4), np.full(N, 3.125)
    elif name == "one_feasible_last":
        C = 0.25 * (1 + k % 5)
        C[:, K - 1] = 0.0
        budget = np.full(N, 0.125)
        J[:, K - 1] = -20.0  # (the worst return of all: feasibility decides, not J)
    elif name == "none_feasible":
        # the cheapest cost 1.25 is shared by the candidates with k % 5 in (1, 2, 3); among them J = 2 is shared by
        # k % 5 in (2, 3): the lowest such k wins.  The candidates with the best J cost more.
        m = k % 5
        C = np.where((m >= 1) & (m <= 3), 1.25, 1.5)
        J = np.where(m == 1, 1.0, np.where((m == 2) | (m == 3), 2.0, 9.0)).astype(np.float32)
        budget, temps = np.full(N, 1.125), (0.0, 1.0)  # (a temperature changes nothing on an empty feasible set)
    elif name == "equal_j":
        C, budget = 0.25 * ((k * 7) % 6), np.array([0.125, 1.125, 2.125])
        C[:, K // 2] = 0.0  # (at least one feasible candidate per slot)
        J = np.full((N, K), 1.5, np.float32)
    elif name == "spread_200":
        # J falls from 0 to -200 over the candidates: at temperature 1 the far weights underflow to 0, the best has 1
        C, budget = 0.25 * (k % 3), np.full(N, 1.125)
        J = (-200.0 * np.arange(K)[None, :] / max(K - 1, 1) + np.zeros((N, 1))).astype(np.float32)
        J = J[:, ::-1].copy() if K > 1 else J  # (the best is the LAST candidate: the sum meets it at its end)
        temps = (0.0, 1.0)
    elif name == "nan_one":
        C, budget = 0.25 * (k % 4), np.array([3.125, 0.125, 3.125])
        bad = min(K - 1, 2)
        J[0, bad] = np.nan                     # a NaN return where the cost is fine
        C[1, bad], J[1, bad] = np.nan, 50.0    # a NaN cost on what would be the best return
        J[2, bad], C[2, bad] = np.nan, np.nan
    elif name == "all_nan":
        C, budget = np.full((N, K), np.nan), np.full(N, 3.125)
        J[:, ::2] = np.nan
    else:
        raise KeyError(name)
    return dict(J=J.astype(np.float32), C=np.asarray(C, np.float32), a0=a0, budget=budget.astype(np.float32), temperatures=temps)


def action_table(a0):
    """The recorder's layout: ``[N * K * H_TABLE, ad]``, candidate e's first action in row ``e * H_TABLE``, NaN elsewhere."""
    n, k, ad = a0.shape
    t = np.full((n * k, H_TABLE, ad), np.nan, np.float32)
    t[:, 0] = a0.reshape(n * k, ad)
    return t.reshape(n * k * H_TABLE, ad)


def disc_table(J, C):
    """``[N * K, 4]``: (J, C, a gamma^t, a pad) -- the last two are not read."""
    d = np.full((J.size, 4), 7.0, np.float32)
    d[:, 0], d[:, 1] = J.reshape(-1), C.reshape(-1)
    return d


def fan_states(n=FAN_N, od=OD, seed=3):
    return (0.5 * np.random.RandomState(seed).randn(n, od)).astype(np.float32)


def hand_model_state_dict(sd, od, ad, hidden):
    """A ``Dynamics`` state dict (one hidden layer, any number of members, the default normaliser) rewritten so that the
    state delta is 0, reward = a_0 and the raw cost = clamp(10 a_0, 0, 1) -- the cost bit is ``a_0 > 0.05``:
      h_0 = relu(a_0), h_1 = relu(-a_0), h_2 = relu(10 a_0), h_3 = relu(10 a_0 - 1);
      reward = h_0 - h_1, cost = h_2 - h_3, every other weight and bias 0."""
    out = {k: np.zeros_like(np.asarray(v)) if k.startswith("members.") else np.asarray(v) for k, v in sd.items()}
    members = sorted({k.split(".")[1] for k in sd if k.startswith("members.")})
    for m in members:
        W0, b0 = out[f"members.{m}.0.weight"], out[f"members.{m}.0.bias"]
        W1 = out[f"members.{m}.2.weight"]
        assert W0.shape == (hidden, od + ad) and W1.shape == (od + 2, hidden) and hidden >= 4
        W0[0, od], W0[1, od], W0[2, od], W0[3, od] = 1.0, -1.0, 10.0, 10.0
        b0[3] = -1.0
        W1[od, 0], W1[od, 1] = 1.0, -1.0
        W1[od + 1, 2], W1[od + 1, 3] = 1.0, -1.0
    return out
