"""The FQE-against-the-truth study's fixed setup, shared by the GPU test (tests/test_gpu_collect.py) and the CPU fp64 run
that measures its absolute bound (tools/collect_fqe_truth.py -> profiles/collect_fqe_truth.json).  Torch and numpy only:
nothing here needs a device."""
from __future__ import annotations

import numpy as np
import torch

OD, AD, EL, GAMMA, INIT_NOISE = 6, 2, 40, 0.8, 0.5
ENV_SEED, BASE_SEED, EPISODES = 6, 3000, 256
POLICY_HIDDEN, POLICY_SEED, LAST_LAYER_SCALE = [32, 32], 1, 8.0
SIGMAS = (0.0, 0.1, 0.3, 0.5)           # sigma of episode e = SIGMAS[e % 4]
NOISE_SEEDS = {"A": 101, "mirror": 202}  # the injected exploration noise of each policy's collection
FQE_HIDDEN, FQE_NUM_Q, FQE_STEPS, FQE_BATCH, FQE_LR, FQE_TAU = [64, 64], 2, 4000, 256, 1e-3, 0.005
TRUTH_JSON = "profiles/collect_fqe_truth.json"


def make_env():
    from osrl_amd.common.synthetic_env import SyntheticSafeEnv
    return SyntheticSafeEnv(OD, AD, EL, seed=ENV_SEED, init_noise=INIT_NOISE)


def bc_state_dict(od, ad, hidden, seed, last_scale=1.0, sign=1.0):
    """A BC actor's state_dict in ``nn.Linear``'s default init under ``torch.manual_seed(seed)``; the last layer times
    ``sign * last_scale`` (tanh is odd: ``sign = -1`` is the policy that always acts the opposite way)."""
    torch.manual_seed(seed)
    sizes = [od] + list(hidden) + [ad]
    sd = {}
    for i in range(len(sizes) - 1):
        lin = torch.nn.Linear(sizes[i], sizes[i + 1])
        f = sign * last_scale if i == len(sizes) - 2 else 1.0
        sd[f"actor.pi.{2 * i}.weight"] = (lin.weight.data * f).clone()
        sd[f"actor.pi.{2 * i}.bias"] = (lin.bias.data * f).clone()
    return sd


def policies():
    """{"A": state_dict, "mirror": state_dict}"""
    return {"A": bc_state_dict(OD, AD, POLICY_HIDDEN, POLICY_SEED, LAST_LAYER_SCALE, 1.0),
            "mirror": bc_state_dict(OD, AD, POLICY_HIDDEN, POLICY_SEED, LAST_LAYER_SCALE, -1.0)}


def sigmas() -> np.ndarray:
    return np.array([SIGMAS[e % len(SIGMAS)] for e in range(EPISODES)], np.float32)


def injected_noise(name: str) -> np.ndarray:
    return np.random.RandomState(NOISE_SEEDS[name]).randn(EL, EPISODES, AD).astype(np.float32)
