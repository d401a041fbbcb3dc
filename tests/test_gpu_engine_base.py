"""The step engines' shared base (osrl_amd/engine/_step.py) on the device, for every engine: a capture leaves the
training state untouched -- also one that raises --, the replayed step is the eager step, and the scalar training state
comes from one list (core.scalar_state)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cases import BEARL_CASES, CASES, CDT_CASES, COPTIDICE_CASES, make_cdt_batch  # noqa: E402
from gpu_util import build_gpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["bc_small", "cpq_small", "bcql_pid", "bearl_lap", "coptidice_kl", "cdt_small", "cdt_det"]
# the scalar training state each engine's own snapshot saved before there was one list of it
SCALARS = {"bc": (), "cpq": ("log_alpha",), "bcql": ("pid_state",), "bearl": ("pid_state", "log_alpha"),
           "coptidice": ("scalar_leaves",), "cdt": ("log_temperature",)}


def _build(name):
    """(model, engine, step): ``step(use_graph)`` runs one train step on device-drawn inputs."""
    if name in CDT_CASES:
        from test_gpu_cdt import build_cdt_gpu
        c = CDT_CASES[name]
        m, tr, lg = build_cdt_gpu(c, stats_mode="none")
        eng = m.engine(c.B, tr.cfg)
        b = {k: torch.from_numpy(v).to(DEV) for k, v in make_cdt_batch(c).items()}
        return m, eng, lambda g: eng.step(b["states"], b["actions"], b["returns"], b["costs_return"], b["time_steps"],
                                          b["mask"], b["costs"], use_graph=g)
    from osrl_amd.common.replay import ReplayStore, synthetic_transitions
    c = {**CASES, **BEARL_CASES, **COPTIDICE_CASES}[name]
    m, tr, lg = build_gpu(c, stats_mode="none")
    eng = m.engine(c.B)
    eng.attach_replay(ReplayStore(synthetic_transitions(2048, c.od, c.ad, seed=7, max_action=c.max_action),
                                  torch.device(DEV), reward_scale=0.1, seed=3, state_init=c.algo == "coptidice"))
    if c.algo == "bc":
        eng.direct = False  # (the one-launch step is launched directly by default: here it goes through the graph)
    return m, eng, eng.step_replay


def _tensors(m, eng):
    """Every tensor of the training state, named -- listed here independently of the engine's own snapshot."""
    out = {}
    for n, g in m.groups.items():
        for b in ("p", "m", "v", "tgt"):
            if getattr(g, b) is not None:
                out[f"{n}.{b}"] = getattr(g, b)
    out.update({"st.state": eng.st.state, "st.stats": eng.st.stats, "st.ring": eng.st.ring})
    for k in SCALARS[type(m).__name__.lower()]:
        if isinstance(getattr(m, k, None), torch.Tensor):  # (a deterministic CDT has no temperature)
            out[k] = getattr(m, k)
    if hasattr(eng, "temp_mv"):
        out["temp_mv"] = eng.temp_mv
    return out


def _copy(m, eng):
    return {k: t.clone() for k, t in _tensors(m, eng).items()}, eng.st.host_step


def _bytes(t):
    return t.detach().contiguous().view(torch.uint8)


def _assert_same(m, eng, ref, what, atol=0.0):
    """Byte for byte; with ``atol`` the fp32 tensors within that absolute bound instead (the step state's bytes always)."""
    torch.cuda.synchronize()
    for k, t in _tensors(m, eng).items():
        if atol and t.dtype == torch.float32:
            d = (t - ref[0][k]).abs().max().item()
            print(f"{what}: {k} max |d| = {d:.3e}")
            assert d < atol, f"{what}: {k} differs by {d:.3e}"
        else:
            assert torch.equal(_bytes(t), _bytes(ref[0][k])), f"{what}: {k} changed"
    assert eng.st.host_step == ref[1], f"{what}: host_step {eng.st.host_step} != {ref[1]}"


def _stepped(name):
    m, eng, step = _build(name)
    for _ in range(2):  # two real (eager) steps: Adam moments, targets and the step count are non-zero
        step(False)
    torch.cuda.synchronize()
    assert eng.graph is None and eng.st.device_step() == 2
    return m, eng, step


@pytest.mark.parametrize("name", NAMES)
def test_capture_leaves_the_training_state_untouched_and_its_replay_is_the_eager_step(name):
    """capture() leaves every byte of the training state as it was, in all seven cases.  The replayed step then equals
    the same step issued eagerly from a copy of that state: byte for byte for the MLP engines; for the two CDT cases
    within 1e-6, because two runs of the SAME CDT step are not bit-equal -- its timestep-embedding scatter accumulates
    with fp32 atomics, whose order (and, through the clip norm, every update's last bits) varies from run to run.  1e-6
    is the bound tests/test_gpu_cdt.py already holds graph == eager and run == run to for that reason
    (test_cdt_graph_replay_matches_eager); the step state (counter, bias corrections) stays byte-equal there too."""
    m, eng, step = _stepped(name)
    before = _copy(m, eng)
    eng.capture()
    assert eng.graph is not None
    _assert_same(m, eng, before, "capture()")  # byte for byte: parameters, moments, targets, step state, scalars
    step(True)  # the replayed step 3 ...
    torch.cuda.synchronize()
    assert eng.st.device_step() == 3 and eng.st.host_step == 3
    replayed = _copy(m, eng)
    for k, t in _tensors(m, eng).items():  # ... against the same step issued eagerly from a copy of the state before it
        t.copy_(before[0][k])
    eng.st.host_step = before[1]
    m.repack()
    step(False)
    _assert_same(m, eng, replayed, "eager step 3 vs replayed step 3", atol=1e-6 if name in CDT_CASES else 0.0)


@pytest.mark.parametrize("name", NAMES)
def test_a_capture_that_raises_restores_the_training_state(name):
    m, eng, step = _stepped(name)
    before = _copy(m, eng)
    body = eng.body

    def failing(*a, **k):  # a host-side exception behind the warm-up pass's launches: before stream capture begins
        body(*a, **k)
        raise RuntimeError("host-side failure behind the warm-up launches")

    eng.body = failing
    try:
        with pytest.raises(RuntimeError, match="host-side failure behind the warm-up launches"):
            eng.capture()
    finally:
        del eng.body
    assert eng.graph is None
    assert not torch.cuda.is_current_stream_capturing()
    _assert_same(m, eng, before, "a capture that raised")
    step(True)  # and the engine goes on: this capture succeeds, the step is step 3
    torch.cuda.synchronize()
    assert eng.graph is not None and eng.st.device_step() == 3


@pytest.mark.parametrize("name", NAMES)
def test_scalar_state_is_one_list_for_snapshot_and_broadcast(name):
    from osrl_amd.engine.core import scalar_state
    from osrl_amd.engine.dist import DataParallel
    m, eng, _ = _build(name)
    got = {t.data_ptr() for t in scalar_state(m, eng)}
    want = {k: t.data_ptr() for k, t in _tensors(m, eng).items() if k in ("log_alpha", "pid_state", "log_temperature",
                                                                         "scalar_leaves", "temp_mv")}
    assert set(want.values()) <= got, f"scalar_state misses {[k for k, p in want.items() if p not in got]}"
    assert got <= {t.data_ptr() for t in eng._state_tensors()}  # ... and the snapshot covers all of it

    class Recorder(DataParallel):  # a world of one without a process group: which tensors would be broadcast
        def __init__(self):
            self.world, self.rank, self.seen = 1, 0, set()

        def broadcast_(self, t):
            self.seen.add(t.data_ptr())
            return t

    rec = Recorder()
    rec.broadcast_model(m, eng)
    assert got <= rec.seen
    for g in m.groups.values():
        assert {b.data_ptr() for b in (g.p, g.m, g.v, g.tgt) if b is not None} <= rec.seen
