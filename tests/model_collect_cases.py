"""Case data of the recorded model rollouts' tests (TEST INFRASTRUCTURE ONLY), as plain numpy, so that
tests/test_model_collect_cpu.py can check with the oracle alone what tests/test_gpu_model_collect.py relies on.  The
dynamics weights, initial states and their seeds are tests/model_env_cases.py's.

Case A: (od, ad) = (11, 3), hidden [40, 40]; case B: (37, 6), hidden [24, 40] -- od > 32 is the first size at which a
thread of the step kernel keeps a second state column, 24 is no multiple of 16, ad = 6 reaches the second Philox block.
Both: 3 members, E = 19 (two tiles, the second partial), horizon 3."""
import numpy as np

import model_env_cases as MC

CASES = {"A": dict(od=11, ad=3, hidden=[40, 40], M=3), "B": dict(od=37, ad=6, hidden=[24, 40], M=3)}
E = 19
HORIZON = 3
LAMBDA = 0.5
POLICY_HIDDEN = [16]
DYN_SEED = {"A": MC.SEED, "B": MC.SEED}  # (B's: tests/test_model_collect_cpu.py holds the cost margin for it)
NOISE_SEED = 21


def policy_pre(ad):
    """The constant policy's pre-activation output: the actor's last bias, all its weights zero."""
    return np.linspace(-0.9, 0.7, ad).astype(np.float32)


def policy_out(ad, max_action=1.0):
    """What that policy outputs in fp64 (``max_action * tanh``)."""
    return max_action * np.tanh(policy_pre(ad).astype(np.float64))


def bc_const_state_dict(od, ad):
    sizes = [od] + POLICY_HIDDEN + [ad]
    sd = {}
    for i in range(len(sizes) - 1):
        sd[f"actor.pi.{2 * i}.weight"] = np.zeros((sizes[i + 1], sizes[i]), np.float32)
        sd[f"actor.pi.{2 * i}.bias"] = np.zeros(sizes[i + 1], np.float32)
    sd[f"actor.pi.{2 * (len(sizes) - 2)}.bias"] = policy_pre(ad)
    return sd


def sigma(n=E):
    """Per-episode noise scales; every third episode is deterministic."""
    s = (0.1 + 0.05 * (np.arange(n) % 7)).astype(np.float32)
    s[::3] = 0.0
    return s


def eps_rows(ad, n=E, steps=HORIZON, poison=False):
    """Injected noise [steps, n, ad]; ``poison``: NaN in the rows of the deterministic episodes (they are not read)."""
    eps = np.random.RandomState(NOISE_SEED).randn(steps, 64, ad).astype(np.float32)[:, :n]
    if poison:
        eps[:, sigma(n) == 0.0] = np.nan
    return eps


def host_actions(ad, n=E, steps=HORIZON, max_action=MC.MAX_ACTION):
    """clip(pi + sigma_e * eps) of the constant policy under ``eps_rows``, fp64 [steps, n, ad]."""
    a = policy_out(ad)[None, None, :] + sigma(n).astype(np.float64)[None, :, None] * eps_rows(ad, n, steps).astype(np.float64)
    return np.clip(a, -max_action, max_action)


def store_rows(n, od, ad, seed=5):
    """A dataset of ``n`` transitions whose observations lie inside the model's clamp range: branch starts."""
    rs = np.random.RandomState(seed)
    f = np.float32
    return dict(observations=rs.uniform(-0.7, 0.7, (n, od)).astype(f), next_observations=rs.uniform(-0.7, 0.7, (n, od)).astype(f),
                actions=rs.uniform(-1, 1, (n, ad)).astype(f), rewards=rs.randn(n).astype(f),
                costs=(rs.uniform(size=n) < 0.2).astype(f), terminals=np.zeros(n, f), timeouts=np.zeros(n, f))
