"""plan.vae_dw_side (engine/plan.py, engine/cpq.py): the VAE group's dW launch on the side branch, in front of the VAE's
optimizer step, instead of on the main chain.

It is a placement: the launches and their inputs are the same, so every parameter, moment and target keeps its bits --
provided the graph's EDGES order it.  Two dependencies cross queues: the dW launch reads the activation and dZ buffers that
the main chain's VAE phase writes (the side branch's second half waits for an event behind that phase), and the NEXT step's
VAE phase rewrites them (the main chain waits, in front of the actor group's Adam, for the event behind the VAE's optimizer
step, which follows the dW launch on its stream).  As in test_unjoined_graphs_are_ordered_by_edges_not_by_timing the second
one is ordered by hundreds of microseconds of slack in an undisturbed run, so the test takes the slack away: a ~600 us spin
kernel in front of the side branch's second half, or at the head of the main chain, of every step of a no-join graph."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
TOTAL, SPG = 6, 3
_ref = {}


def _one_step_replays(monkeypatch, knob):
    """State and statistics after TOTAL replays of the one-step graph at C2's shape with the knob at ``knob``."""
    from test_gpu_pipeline import _bench, _state
    monkeypatch.setenv("OSRL_LAB", "1")
    monkeypatch.setenv("OSRL_VAE_DW_SIDE", knob)
    if knob not in _ref:
        m, e = _bench("c2")
        assert e.plan.vae_adam_side and e.plan.ood_rows and e.plan.vae_dw_side == (knob == "1")
        for _ in range(TOTAL):
            e.step_replay(True)
        torch.cuda.synchronize()
        _ref[knob] = (_state(m, e), [e.st.read_stats(s) for s in range(1, TOTAL + 1)])
        del m, e
        torch.cuda.empty_cache()
    return _ref[knob]


@pytest.mark.parametrize("at", ["second", "main"])
def test_side_dw_is_ordered_by_edges_not_by_timing(at, monkeypatch):
    from test_gpu_pipeline import _bench, _spin_cycles, _state
    ref, ref_stats = _one_step_replays(monkeypatch, "1")
    monkeypatch.setenv("OSRL_STRESS_SPIN_CYCLES", str(_spin_cycles(600.0)))
    monkeypatch.setenv("OSRL_STRESS_SPIN_AT", at)
    m, e = _bench("c2")
    assert e.plan.pipe_no_join and e.plan.vae_dw_side and e._stress_spin > 0
    e.steps_replay(TOTAL, steps_per_graph=SPG)
    torch.cuda.synchronize()
    got, stats = _state(m, e), [e.st.read_stats(s) for s in range(1, TOTAL + 1)]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    e.steps_replay(SPG, steps_per_graph=SPG)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / SPG
    assert us > 500.0, f"the spin kernel is not in the graph ({us:.0f} us per step)"
    assert set(got) == set(ref)
    for k in ref:
        assert torch.equal(ref[k], got[k]), f"{k} moves when the {at} chain is late (max |d| = {(ref[k] - got[k]).abs().max().item():.3e})"
    for s in range(TOTAL):
        for k, v in ref_stats[s].items():
            assert stats[s][k] == v, f"statistic {k} of step {s + 1} moves when the {at} chain is late: {stats[s][k]} vs {v}"


def test_placement_leaves_every_bit(monkeypatch):
    """Knob 0 and 1: the same parameters, moments, targets and statistics."""
    on, on_stats = _one_step_replays(monkeypatch, "1")
    off, off_stats = _one_step_replays(monkeypatch, "0")
    assert set(on) == set(off)
    for k in on:
        assert torch.equal(on[k], off[k]), f"{k} depends on where the VAE's dW launch sits (max |d| = {(on[k] - off[k]).abs().max().item():.3e})"
    assert on_stats == off_stats
