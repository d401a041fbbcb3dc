"""CPU-side checks of the lockstep act path of the MLP policies: the ``osrl_policy_*_n`` entry points are declared in
the header, mirrored in ``_lib.PROTOTYPES`` and exported by the library; act_vec.hip compiles for gfx950 without scratch,
within the LDS bound, on fp32 MFMA; VecFastPolicy's argument checks raise before any device call; the five trainers'
``rollout_many`` / ``evaluate`` follow the documented schedule on fake environments with a stub policy."""
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"osrl_policy_create_n": 3, "osrl_policy_io_n": 7, "osrl_policy_act_n": 5, "osrl_policy_destroy_n": 1}


def test_header_prototypes_and_library_agree_on_the_new_entry_points():
    import ctypes as C
    from osrl_amd import _lib as L
    from osrl_amd import build as b
    hdr = open(os.path.join(ROOT, "include", "osrl_amd.h")).read()
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/osrl_amd.h"
        assert len(m.group(1).split(",")) == nargs == len(L.PROTOTYPES[name]), name
    m = re.search(r"#define\s+OSRL_POLICY_MAX_ENVS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == L.POLICY_MAX_ENVS == 64
    m = re.search(r"#define\s+OSRL_POLICY_MAX_ROWS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == L.POLICY_MAX_ROWS == 4  # the GEMV path keeps its own limit
    assert "act_vec.hip" in b.SOURCES
    lib = C.CDLL(b.build())
    for name in NEW:
        assert hasattr(lib, name), f"libosrl_amd.so does not export {name}"


def test_header_stays_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc is required to compile the header as C")
    src = str(tmp_path / "h.c")
    with open(src, "w") as f:
        f.write('#include "osrl_amd.h"\n'
                "int (*p)(void*, int32_t, int32_t, uint64_t, void*) = osrl_policy_act_n;\n"
                "int (*q)(const osrl_policy_t*, int32_t, void**) = osrl_policy_create_n;\n"
                "int n = OSRL_POLICY_MAX_ENVS;\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                    str(tmp_path / "h.o")], check=True, capture_output=True)


def test_kernels_no_scratch_lds_bound_mfma(tmp_path):
    from osrl_amd.build import FILE_FLAGS, FLAGS
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.fail("hipcc is required to cross-compile the gfx950 listing")
    out = str(tmp_path / "act_vec.s")
    cmd = [hipcc] + FLAGS + FILE_FLAGS.get("act_vec.hip", []) + \
        ["-S", "--cuda-device-only", os.path.join(ROOT, "osrl_amd", "csrc", "act_vec.hip"), "-o", out]
    assert subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    text = open(out).read()
    blocks = re.findall(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    # ONE kernel, two instantiations by LDS row width (512 and OSRL_MAX_WIDTH = 1024)
    assert len(blocks) == 2, [b[0] for b in blocks]
    for w in (512, 1024):
        assert sum(f"policy_vec_kernelILi{w}E" in name for name, _ in blocks) == 1, (w, [b[0] for b in blocks])
    for name, body in blocks:
        assert "policy_act_kernel" not in name  # tests/test_isa_mlp_wide_cpu.py pins act.hip's kernels by that needle
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0, name
        assert 0 < int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", body).group(1)) <= 160 * 1024, name
    assert len(re.findall(r"\bv_mfma_f32_16x16x4", text)) >= 2
    assert not re.search(r"\bs_sleep\b", text)


# ---- VecFastPolicy without a device ---------------------------------------------------------------------------------
class _Boom:
    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the argument checks")


def _stub_policy(kind="gauss", N=3, od=4, ad=2, nd=2):
    """A VecFastPolicy without a device: every C call fails the test."""
    from osrl_amd.engine.act import VecFastPolicy
    p = object.__new__(VecFastPolicy)
    p.num_envs, p.obs_dim, p.act_dim, p.noise_dim, p.kind, p.seed = N, od, ad, nd, kind, 0
    p._h, p._lib = object(), _Boom()
    p._started = True
    p._raw_stream, p._dev_index = None, 0
    p._meta = np.zeros((N, 2), np.int32)
    return p


def test_num_envs_range_is_checked_first(monkeypatch):
    from osrl_amd import _lib as L
    from osrl_amd.engine import act as A
    monkeypatch.setattr(L, "load", lambda: _Boom())
    monkeypatch.setattr(A, "require_cuda", lambda d: (_ for _ in ()).throw(AssertionError("device before num_envs")))
    assert A.MAX_ENVS == 64
    for bad in (0, -1, 65):
        with pytest.raises(ValueError, match="1 .. 64"):
            A.VecFastPolicy("mlp", "cuda:0", 4, 2, None, num_envs=bad)
    for bad in (2.0, "4", None, True):
        with pytest.raises(ValueError, match="integer"):
            A.VecFastPolicy("mlp", "cuda:0", 4, 2, None, num_envs=bad)
    # the models' caches check the width the same way, before building anything
    for bad in (0, 65, 1.5):
        with pytest.raises(ValueError):
            A.cached_vec_policy(SimpleNamespace(), bad, lambda n: (_ for _ in ()).throw(AssertionError("built")))


def test_shapes_are_checked_before_any_device_call():
    p = _stub_policy()
    N, od, nd = 3, 4, 2
    obs = np.zeros((N, od), np.float32)
    for bad in (np.zeros(od), np.zeros((N + 1, od)), np.zeros((N, od + 1)), 0.0):
        with pytest.raises(ValueError, match="obs of shape"):
            p.reset(bad)
        with pytest.raises(ValueError, match="obs of shape"):
            p.step(bad)
    for bad in (np.zeros(nd), np.zeros((N, nd + 1)), np.zeros((N - 1, nd))):
        with pytest.raises(ValueError, match="noise of shape"):
            p.step(obs, noise=bad)
        with pytest.raises(ValueError, match="noise of shape"):
            p.reset(obs, noise=bad)
    for bad in (True, np.ones(N + 1, bool), np.ones((N, 1), bool)):
        with pytest.raises(ValueError, match="active of shape"):
            p.step(obs, active=bad)
    with pytest.raises(ValueError, match="booleans"):
        p.step(obs, active=np.ones(N))
    for bad in (np.zeros(N + 1, np.int64), 3):
        with pytest.raises(ValueError, match="episode_ids of shape"):
            p.reset(obs, episode_ids=bad)
    for bad in (np.zeros(N), np.array([0, -1, 2]), np.array([0, 1, 2 ** 31])):
        with pytest.raises(ValueError, match="episode_ids as integers"):
            p.reset(obs, episode_ids=bad)
    with pytest.raises(ValueError, match="takes no noise"):
        _stub_policy("mlp", nd=0).step(obs, noise=np.zeros((N, 1)))
    assert (p._meta == 0).all()  # nothing was recorded by a rejected call
    p._started = False
    with pytest.raises(RuntimeError, match="reset"):
        p.step(obs)
    p._h = None
    with pytest.raises(RuntimeError, match="closed"):
        p.reset(obs)
    p.close()  # closing a closed policy is a no-op


def test_vector_policy_is_not_copyable():
    import copy
    import pickle
    p = _stub_policy()
    assert copy.deepcopy(p) is None
    assert pickle.loads(pickle.dumps(p)) is None


# ---- the trainers' schedule on fake environments --------------------------------------------------------------------
class _FakeEnv:
    """Observation = (environment tag, step, 0 ..); reward 1 + tag, cost from a table; ends by `term` / `trunc` step."""

    def __init__(self, tag, od, term=None, trunc=None, log=None):
        self.tag, self.od, self.term, self.trunc, self.log = tag, od, term, trunc, log
        self.resets, self.t = 0, 0

    def _obs(self):
        o = np.zeros(self.od)
        o[0], o[1] = self.tag, self.t
        return o

    def reset(self):
        self.resets += 1
        self.t = 0
        return self._obs(), {}

    def step(self, act):
        self.t += 1
        if self.log is not None:
            self.log.append((self.tag, self.t, np.array(act, copy=True)))
        return (self._obs(), 1.0 + self.tag, self.term == self.t, self.trunc == self.t, {"cost": 0.25 * (self.tag + 1)})


class _StubVec:
    """Stands in for VecFastPolicy: records every call; the action of a slot is (obs[0], obs[1], episode id)."""

    def __init__(self, N, od):
        self.num_envs, self.obs_dim, self.calls = N, od, []
        self.ids = np.zeros(N, np.int64)

    def _act(self, obs, active):
        a = np.zeros((self.num_envs, 3), np.float32)
        a[:, 0], a[:, 1], a[:, 2] = obs[:, 0], obs[:, 1], self.ids
        a[~active] = np.nan  # an idle slot's action must never reach an environment
        return a, None

    def reset(self, obs, episode_ids=None, active=None):
        assert obs.shape == (self.num_envs, self.obs_dim) and active.dtype == np.bool_
        self.ids[active] = np.asarray(episode_ids)[active]
        self.calls.append(("reset", obs.copy(), active.copy(), np.array(episode_ids, copy=True)))
        return self._act(obs, active)

    def step(self, obs, active=None):
        self.calls.append(("step", obs.copy(), active.copy()))
        return self._act(obs, active)


def _trainer(algo, EL=6, od=4, **kw):
    from osrl_amd import algorithms as alg
    cls = {"bc": alg.BCTrainer, "cpq": alg.CPQTrainer, "bcql": alg.BCQLTrainer, "bearl": alg.BEARLTrainer,
           "coptidice": alg.COptiDICETrainer}[algo]
    tr = object.__new__(cls)
    stubs, modes = {}, []

    def fast_policy(num_envs=None):
        assert num_envs is not None, "the lockstep loop must ask for the vector policy"
        return stubs.setdefault(num_envs, _StubVec(num_envs, od + (1 if kw.get("bc_mode") == "multi-task" else 0)))

    tr.model = SimpleNamespace(episode_len=EL, fast_policy=fast_policy, eval=lambda: modes.append("eval"),
                               train=lambda: modes.append("train"), _engine=None)
    tr.reward_scale, tr.cost_scale = kw.get("reward_scale", 1.0), kw.get("cost_scale", 1.0)
    tr.bc_mode, tr.cost_limit = kw.get("bc_mode", "all"), kw.get("cost_limit", 10)
    tr.env = None
    return tr, stubs, modes


ALGOS = ["bc", "cpq", "bcql", "bearl", "coptidice"]


@pytest.mark.parametrize("algo", ALGOS)
def test_rollout_many_retires_slots_and_accumulates_like_rollout(algo):
    EL, od = 6, 4
    tr, stubs, _ = _trainer(algo, EL, od, cost_scale=3.0, reward_scale=2.0)
    log = []
    envs = [_FakeEnv(0, od, term=2, log=log), _FakeEnv(1, od, trunc=4, log=log), _FakeEnv(2, od, log=log)]
    ret, length, cost = tr.rollout_many(envs, num_slots=5, episode_ids=[7, 8, 9])
    np.testing.assert_array_equal(length, [2, 4, EL])  # terminate, truncate, episode_len
    assert length.dtype == np.int64
    np.testing.assert_array_equal(ret, [2 * 1.0, 4 * 2.0, EL * 3.0])  # rewards are summed unscaled
    scale = 1.0 if algo == "bc" else 3.0  # BC sums info["cost"] as it is, the others info["cost"] * cost_scale
    np.testing.assert_array_equal(cost, [2 * 0.25 * scale, 4 * 0.5 * scale, EL * 0.75 * scale])
    pol = stubs[5]
    assert [c[0] for c in pol.calls] == ["reset"] + ["step"] * (EL - 1)  # no call after the last environment step
    np.testing.assert_array_equal(pol.calls[0][2], [True, True, True, False, False])  # slots past len(envs) idle
    np.testing.assert_array_equal(pol.calls[0][3][:3], [7, 8, 9])
    np.testing.assert_array_equal(pol.calls[2][2], [False, True, True, False, False])  # env 0 left after step 2
    np.testing.assert_array_equal(pol.calls[4][2], [False, False, True, False, False])  # env 1 left after step 4
    # every environment saw the action computed from ITS latest observation and its episode id, and one reset
    for tag, t, act in log:
        np.testing.assert_array_equal(act, [tag, t - 1, 7 + tag])
    assert [e.resets for e in envs] == [1, 1, 1]
    assert sorted(set(t for tag, t, _ in log if tag == 0)) == [1, 2]
    with pytest.raises(ValueError, match="do not fit"):
        tr.rollout_many(envs, num_slots=2)
    with pytest.raises(ValueError, match="episode_ids"):
        tr.rollout_many(envs, episode_ids=[1, 2])
    r, l, c = tr.rollout_many([])
    assert r.shape == l.shape == c.shape == (0,)
    # default: as many slots as environments, episode ids 0 .. n - 1
    tr.rollout_many(envs)
    np.testing.assert_array_equal(stubs[3].calls[0][3], [0, 1, 2])


def test_bc_multitask_appends_the_cost_limit_to_every_observation():
    EL, od = 4, 3
    tr, stubs, _ = _trainer("bc", EL, od, bc_mode="multi-task", cost_limit=20)
    tr.rollout_many([_FakeEnv(0, od), _FakeEnv(1, od)])
    calls = stubs[2].calls
    assert len(calls) == EL
    for t, c in enumerate(calls):
        assert c[1].shape == (2, od + 1)
        np.testing.assert_array_equal(c[1][:, od], [20.0, 20.0])
        np.testing.assert_array_equal(c[1][:, 1], [t, t])
    tr2, stubs2, _ = _trainer("bc", EL, od)  # every other mode: observations as they come
    tr2.rollout_many([_FakeEnv(0, od)])
    assert stubs2[1].calls[0][1].shape == (1, od)


@pytest.mark.parametrize("algo", ALGOS)
def test_evaluate_over_a_list_runs_job_q_in_wave_q_div_n_on_env_q_mod_n(algo):
    EL, od, N, jobs = 5, 4, 3, 7
    tr, stubs, modes = _trainer(algo, EL, od, cost_scale=2.0, reward_scale=4.0)
    log = []
    # environment e ends after 2 + e steps: the episode lengths tell which environment a job ran on
    tr.env = [_FakeEnv(e, od, trunc=2 + e, log=log) for e in range(N)]
    ret, cost, length = tr.evaluate(jobs)
    assert modes == ["eval", "train"]
    pol = stubs[N]  # every wave, the short last one included, uses the N-wide policy
    assert list(stubs) == [N]
    resets = [c for c in pol.calls if c[0] == "reset"]
    assert len(resets) == 3  # waves 0, 1, 2
    for w, c in enumerate(resets):
        k = min(N, jobs - w * N)
        np.testing.assert_array_equal(c[2], [True] * k + [False] * (N - k))
        np.testing.assert_array_equal(c[3][:k], np.arange(w * N, w * N + k))  # episode id = job number
    assert [e.resets for e in tr.env] == [3, 2, 2]  # jobs 0 3 6 | 1 4 | 2 5
    for tag, t, act in log:
        assert act[2] % N == tag  # job q ran on environment q % N
    per_job = [2 + q % N for q in range(jobs)]
    assert length == np.mean(per_job)
    want_ret = np.mean([(1.0 + q % N) * n for q, n in zip(range(jobs), per_job)])
    cs = 1.0 if algo == "bc" else 2.0
    want_cost = np.mean([0.25 * (q % N + 1) * cs * n for q, n in zip(range(jobs), per_job)])
    if algo == "bc":  # bc.py:123 does not rescale
        assert ret == want_ret and cost == want_cost
    else:
        assert ret == want_ret / 4.0 and cost == want_cost / 2.0
    tr.env = (tr.env[0],)  # a tuple is a list of environments too
    assert tr.evaluate(2)[2] == 2
    for empty in ([], ()):
        tr.env = empty
        with pytest.raises(ValueError, match="empty"):
            tr.evaluate(3)
