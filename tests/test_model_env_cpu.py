"""CPU-side checks of the learned-dynamics environment: the oracle's written-out backward against autograd, the limits
named at construction without a device, the ctypes mirror of the new descriptor against the compiled header, and the
normaliser tables through ``fit_normalizer`` / ``state_dict``."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from model_env_oracle import TABLES, OracleDynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OD, AD = 5, 2


def _random_state(M, hidden, seed=0):
    rs = np.random.RandomState(seed)
    sizes = [OD + AD] + hidden + [OD + 2]
    sd = {}
    for m in range(M):
        for i in range(len(sizes) - 1):
            sd[f"members.{m}.{2 * i}.weight"] = rs.randn(sizes[i + 1], sizes[i]) / np.sqrt(sizes[i])
            sd[f"members.{m}.{2 * i}.bias"] = 0.1 * rs.randn(sizes[i + 1])
    sd.update(mu_s=rs.randn(OD), sd_s=0.5 + rs.rand(OD), mu_d=0.1 * rs.randn(OD), sd_d=0.2 + rs.rand(OD),
              mu_r=rs.randn(1), sd_r=0.5 + rs.rand(1), s_lo=-5.0 * np.ones(OD), s_hi=5.0 * np.ones(OD))
    return sd


def _batch(B, seed=1):
    rs = np.random.RandomState(seed)
    return (rs.randn(B, OD), rs.randn(B, OD), rs.uniform(-1, 1, (B, AD)), rs.randn(B), (rs.rand(B) < 0.3).astype(np.float64))


@pytest.mark.parametrize("M,hidden", [(1, [8]), (3, [12, 9]), (2, [6, 7, 5])])
def test_oracle_step_matches_autograd(M, hidden):
    sd = _random_state(M, hidden)
    lr = 1e-3
    o = OracleDynamics(sd, lr)
    leaves = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items() if k.startswith("members.")}
    opt = torch.optim.Adam(list(leaves.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8)
    t = lambda v: torch.tensor(np.asarray(v), dtype=torch.float64)  # noqa: E731
    nl = len(hidden) + 1
    for s in range(3):
        obs, nobs, act, rew, cost = _batch(11, seed=s)
        x = torch.cat([(t(obs) - t(sd["mu_s"])) / t(sd["sd_s"]), t(act)], 1)
        tg = torch.cat([(t(nobs) - t(obs) - t(sd["mu_d"])) / t(sd["sd_d"]), ((t(rew) - t(sd["mu_r"])) / t(sd["sd_r"]))[:, None],
                        t(cost)[:, None]], 1)
        loss = 0.0
        for m in range(M):
            h = x
            for i in range(nl):
                h = h @ leaves[f"members.{m}.{2 * i}.weight"].T + leaves[f"members.{m}.{2 * i}.bias"]
                if i < nl - 1:
                    h = torch.relu(h)
            loss = loss + ((h - tg) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        l_o, g_o = o.loss_and_grads(obs, nobs, act, rew, cost)
        assert abs(l_o - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
        for k, v in leaves.items():
            np.testing.assert_allclose(g_o[k], v.grad.numpy(), rtol=1e-10, atol=1e-13)
        opt.step()
        assert o.step(obs, nobs, act, rew, cost)["loss/dynamics_loss"] == l_o
        for k, v in leaves.items():
            np.testing.assert_allclose(o.p[k], v.detach().numpy(), rtol=1e-9, atol=1e-12)


def test_oracle_env_step_modes():
    sd = _random_state(3, [12, 9])
    o = OracleDynamics(sd)
    s, _, a, _, _ = _batch(7)
    mean = o.env_step(s, 2.0 * a, "mean", clamp=False)
    np.testing.assert_allclose(mean["y"].mean(0)[:, :OD] * sd["sd_d"] + sd["mu_d"] + s, mean["s_next"], rtol=1e-12)
    picks = np.arange(7) % 3
    rnd = o.env_step(s, 2.0 * a, "random", members=picks, clamp=False)
    for k in range(3):
        mem = o.env_step(s, 2.0 * a, "member", member=k, clamp=False)
        rows = picks == k
        assert np.array_equal(mem["s_next"][rows], rnd["s_next"][rows]) and np.array_equal(mem["d"], mean["d"])
    pen = o.env_step(s, 2.0 * a, "mean", lam=0.5)
    np.testing.assert_allclose(pen["reward"], mean["reward"] - 0.5 * mean["d"], rtol=1e-12)
    assert (pen["s_next"] <= 5.0).all() and (pen["s_next"] >= -5.0).all() and (mean["d"] > 0).all()


def test_constructor_limits_are_named():
    """Refused before any device is touched (device="cpu" would itself be refused after these checks)."""
    from osrl_amd.algorithms import Dynamics
    with pytest.raises(ValueError, match="513"):
        Dynamics(11, 3, [513, 64], device="cpu")
    with pytest.raises(ValueError, match="513"):
        Dynamics(256, 257, [64], device="cpu")  # the input row itself
    with pytest.raises(ValueError, match="state_dim 257"):
        Dynamics(257, 3, [64], device="cpu")
    with pytest.raises(ValueError, match="num_models = 9"):
        Dynamics(11, 3, [64], num_models=9, device="cpu")
    with pytest.raises(ValueError, match="Linear layers"):
        Dynamics(11, 3, [8, 8, 8, 8], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Dynamics(11, 3, [64], device="cpu")


def test_descriptor_mirror_matches_the_header(tmp_path):
    import ctypes as C
    from osrl_amd import _lib as L
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src, exe = str(tmp_path / "sz.c"), str(tmp_path / "sz")
    pairs = [("osrl_model_env_t", L.ModelEnvT), ("osrl_gemv_net_t", L.GemvNetT)]
    with open(src, "w") as f:
        f.write('#include "osrl_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n')
        for cname, cls in pairs:
            f.write(f'  printf("%zu", sizeof({cname}));\n')
            for fname, _ in cls._fields_:
                f.write(f'  printf(" %zu", offsetof({cname}, {fname}));\n')
            f.write('  printf("\\n");\n')
        f.write('  printf("%d %d %d %d %d\\n", OSRL_MODEL_ENV_MEAN, OSRL_MODEL_ENV_MEMBER, OSRL_MODEL_ENV_RANDOM, '
                'OSRL_MODEL_ENV_MAX_WIDTH, OSRL_MODEL_ENV_MAX_STATE);\n')
        f.write("  return 0;\n}\n")
    subprocess.run([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line, (cname, cls) in zip(out, pairs):
        want = [C.sizeof(cls)] + [getattr(cls, fname).offset for fname, _ in cls._fields_]
        assert [int(x) for x in line.split()] == want, cname
    assert [int(x) for x in out[2].split()] == [L.MODEL_ENV_MEAN, L.MODEL_ENV_MEMBER, L.MODEL_ENV_RANDOM,
                                                L.MODEL_ENV_MAX_WIDTH, L.MODEL_ENV_MAX_STATE]
    assert L.MODEL_ENV_MODES == {"mean": 0, "member": 1, "random": 2}


@pytest.fixture
def layout_only():
    import osrl_amd.engine.core as core
    core.LAYOUT_ONLY_OK = True
    try:
        yield
    finally:
        core.LAYOUT_ONLY_OK = False


def test_fit_normalizer_and_state_dict_round_trip(layout_only):
    from osrl_amd.algorithms import Dynamics
    rs = np.random.RandomState(3)
    n = 40
    d = dict(observations=rs.randn(n, OD).astype(np.float32), next_observations=rs.randn(n, OD).astype(np.float32),
             actions=rs.randn(n, AD).astype(np.float32), rewards=(3.0 + 2.0 * rs.randn(n)).astype(np.float32))
    d["observations"][:, 2] = d["next_observations"][:, 2] = 0.25  # a constant column: its sigmas sit at the floor
    torch.manual_seed(0)
    a = Dynamics(OD, AD, [8, 8], num_models=2, device="cpu")
    assert set(TABLES) <= set(a.state_dict()) and a.state_dict()["mu_r"].shape == (1,)
    assert set(a.state_dict()) == set(TABLES) | {f"members.{m}.{2 * i}.{w}" for m in range(2) for i in range(3)
                                                 for w in ("weight", "bias")}
    a.fit_normalizer(d)
    o64 = {k: v.astype(np.float64) for k, v in d.items()}
    dl = o64["next_observations"] - o64["observations"]
    both = np.concatenate([o64["observations"], o64["next_observations"]])
    want = dict(mu_s=o64["observations"].mean(0), sd_s=np.maximum(o64["observations"].std(0), 1e-6), mu_d=dl.mean(0),
                sd_d=np.maximum(dl.std(0), 1e-6), mu_r=o64["rewards"].mean(keepdims=True),
                sd_r=np.maximum(o64["rewards"].std(keepdims=True), 1e-6), s_lo=both.min(0), s_hi=both.max(0))
    for k, v in want.items():
        np.testing.assert_allclose(getattr(a, k).numpy(), v.astype(np.float32), rtol=1e-6, atol=1e-7, err_msg=k)
    assert a.sd_s[2].item() == np.float32(1e-6) and a.sd_d[2].item() == np.float32(1e-6)
    torch.manual_seed(1)
    b = Dynamics(OD, AD, [8, 8], num_models=2, device="cpu")
    ptrs = {k: getattr(b, k).data_ptr() for k in TABLES}
    assert not torch.equal(b.mu_s, a.mu_s)
    b.load_state_dict({k: v.clone() for k, v in a.state_dict().items()})
    for k, v in a.state_dict().items():
        assert torch.equal(b.state_dict()[k], v), k
    assert ptrs == {k: getattr(b, k).data_ptr() for k in TABLES}  # written in place: captured launches follow


def test_checkpoint_carries_the_tables(layout_only, tmp_path):
    from osrl_amd.algorithms import Dynamics
    from osrl_amd.common.checkpoint import load_checkpoint, save_checkpoint
    torch.manual_seed(0)
    a = Dynamics(OD, AD, [8], num_models=2, device="cpu")
    with torch.no_grad():
        for i, k in enumerate(TABLES):
            getattr(a, k).add_(0.5 + i)
    path = str(tmp_path / "dyn.pt")
    save_checkpoint(a, path)
    torch.manual_seed(1)
    b = Dynamics(OD, AD, [8], num_models=2, device="cpu")
    load_checkpoint(b, path)
    for k, v in a.state_dict().items():
        assert torch.equal(b.state_dict()[k], v), k


def test_device_env_marker_and_exports():
    from osrl_amd import algorithms
    from osrl_amd.common.model_env import ModelVecEnv
    from osrl_amd.common.synthetic_env import DeviceVecEnv, VecSyntheticSafeEnv
    assert issubclass(VecSyntheticSafeEnv, DeviceVecEnv) and issubclass(ModelVecEnv, DeviceVecEnv)
    assert {"Dynamics", "DynamicsTrainer"} <= set(algorithms.__all__)


def test_parity_cases_keep_clear_of_the_cost_threshold():
    """What tests/test_gpu_model_env.py relies on, with the oracle alone: along the free 12-step rollout of every parity
    case both cost values occur and at most 2 % of the rows lie within 1e-3 of the 0.5 threshold."""
    import model_env_cases as MC
    for E, od, ad, hidden, M, mode, member, clamp, lam in MC.PARITY:
        o = OracleDynamics(MC.dyn_state_dict(od, ad, hidden, M))
        s, acts = MC.start_rows(E, od).astype(np.float64), MC.actions(E, ad)
        raw = []
        for t in range(MC.T_STEPS):
            out = o.env_step(s, acts[t], mode, member, clamp=clamp, lam=lam, max_action=MC.MAX_ACTION)
            raw.append(out["cost_raw"])
            s = out["s_next"]
        raw = np.concatenate(raw)
        near = np.abs(raw - 0.5) <= 1e-3
        assert near.mean() <= 0.02, (E, od, hidden, M, near.mean())
        assert 0.03 <= (raw > 0.5).mean() <= 0.97, (E, od, hidden, M, (raw > 0.5).mean())
        assert np.isfinite(s).all() and np.abs(s).max() < 50.0
