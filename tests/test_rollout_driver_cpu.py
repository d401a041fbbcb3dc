"""The run driver the rollouts and collectors share (engine/rollout.py ``_Driver``, engine/collect.py ``_Tables``), on a stub:
``body`` counts its calls and ``graph`` is an object whose ``replay`` counts.  No library is loaded, no device is used.  These
are the edges at which five separate run loops could drift apart: the step counts around one and two chunks, the two
chunk rules, the injected noise's lifetime when a body raises, and the trainers' ``(key, object)`` cache."""
import pytest

from osrl_amd.engine.collect import _Tables
from osrl_amd.engine.rollout import _CHUNK, _Driver, cached

STEPS = (1, 19, 20, 21, 41)


class _Graph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


class _Stub(_Tables, _Driver):
    use_graph = True

    def __init__(self, raise_at=None):
        self.graph, self.bodies, self.raise_at, self._eps, self.seen = _Graph(), 0, raise_at, None, []

    def body(self):
        self.bodies += 1
        self.seen.append(self._eps)
        if self.bodies == self.raise_at:
            raise RuntimeError("body failed")

    def _capture(self, chunk=_CHUNK):
        raise AssertionError("a driver that holds a graph must not capture again")


def test_chunk_is_twenty():
    assert _CHUNK == 20


@pytest.mark.parametrize("steps", STEPS)
def test_eager_runs_steps_bodies(steps):
    s = _Stub()
    s._drive(steps, _CHUNK, False)
    assert (s.bodies, s.graph.replays) == (steps, 0)
    s = _Stub()
    s._drive(steps, min(steps, _CHUNK), False)
    assert (s.bodies, s.graph.replays) == (steps, 0)


@pytest.mark.parametrize("steps", STEPS)
def test_graph_replays_ceil_steps_over_chunk(steps):
    for chunk in (_CHUNK, min(steps, _CHUNK)):  # (the second: ModelCollector's rule)
        s = _Stub()
        s._drive(steps, chunk, True)
        assert (s.bodies, s.graph.replays) == (0, -(-steps // chunk)), chunk
        assert s.graph.replays * chunk >= steps > (s.graph.replays - 1) * chunk


def test_drive_captures_once_when_there_is_no_graph():
    class Capturing(_Stub):
        def _capture(self, chunk=_CHUNK):
            self.captured.append(chunk)
            self.graph = _Graph()

    s = Capturing()
    s.graph, s.captured = None, []
    s._drive(41, 7, True)
    s._drive(41, 7, True)
    assert s.captured == [7] and s.graph.replays == 12 and s.bodies == 0


@pytest.mark.parametrize("steps", STEPS)
def test_recorded_drive(steps):
    s = _Stub()
    s._drive_recorded(steps, _CHUNK, None)  # no injected noise: the graph
    assert (s.bodies, s.graph.replays, s._eps) == (0, -(-steps // _CHUNK), None)
    noise = object()
    s = _Stub()
    s._drive_recorded(steps, _CHUNK, noise)  # injected noise: eager, and every body sees it
    assert (s.bodies, s.graph.replays, s._eps) == (steps, 0, None)
    assert all(x is noise for x in s.seen)
    s = _Stub()
    s.use_graph = False
    s._drive_recorded(steps, _CHUNK, None)
    assert (s.bodies, s.graph.replays, s._eps) == (steps, 0, None)


def test_raising_body_clears_the_injected_noise():
    s = _Stub(raise_at=3)
    with pytest.raises(RuntimeError, match="body failed"):
        s._drive_recorded(21, _CHUNK, object())
    assert s._eps is None and s.bodies == 3


def test_cache_helper():
    class Owner:
        pass

    o, made = Owner(), []

    def make():
        made.append(object())
        return made[-1]

    a = cached(o, "_rollout", (1, "cpq", 1.0, None), make)
    assert cached(o, "_rollout", (1, "cpq", 1.0, None), make) is a and len(made) == 1
    assert o._rollout == ((1, "cpq", 1.0, None), a)  # the pair the trainers' callers read
    b = cached(o, "_rollout", (1, "cpq", 2.0, None), make)
    assert b is not a and o._rollout[1] is b and len(made) == 2
    c = cached(o, "_collector", (1, "cpq", 2.0, None), make)  # another attribute is another cache
    assert c is not b and o._rollout[1] is b and o._collector[1] is c
