"""The optimizer tail of csrc/optim.hip -- osrl_adam_step, osrl_adam_step_packed, osrl_polyak, osrl_reduce_slabs,
osrl_reduce_slabs_counts, osrl_step_tick, osrl_step_tick_peer -- and the tick arithmetic restated in csrc/rng.hip
(osrl_step_begin_peer_w) against the fp64 restatement of tests/optim_oracle.py on the case table of
tests/optim_cases.py, called through ``osrl_amd._lib`` directly.  Gates: tests/optim_oracle.py (module docstring).  The
equivalence tests of the suite (the dW + Adam launch, the Polyak step carried by Adam, the descriptor twins, the one-launch
BC step) assert bit equality with these launches, so they bottom out here.

Every Adam case is one step from a planted state (p, m, v, tgt, slabs and the 24 state bytes are written by the test).
Every device buffer of a launch carries a 64-element guard tail; every word the oracle marks untouched (NaN), every
input buffer and every guard must keep its bits.
"""
import struct

import numpy as np
import pytest
import torch

import optim_cases as OC
import optim_oracle as OO

pytestmark = pytest.mark.gpu
GUARD = 64
STATE = np.dtype([("step", "<i8"), ("bc1", "<f4"), ("bc2_sqrt", "<f4"), ("lr_scale", "<f4"), ("arrive", "<u4")])
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _class_maxima():
    yield
    print("\nworst |got - fp64| / gate per class: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _state_bytes(s):
    return np.frombuffer(struct.pack("<qfffI", int(s["step"]), s["bc1"], s["bc2_sqrt"], s["lr_scale"], 0), np.uint8)


_BODY = {"p": (np.float32, np.nan), "q": (np.int32, -7), "b": (np.uint8, 0xA5), "s": (np.uint8, 0xA5)}


def launch(kernel, x, over=None, expect=0):
    """One launch of osrl_<kernel> on the inputs ``x``.  Returns (name -> buffer after, name -> buffer before), the guard
    tails checked and stripped; a refused call (``expect`` != 0) must leave every buffer as it was."""
    from osrl_amd import _lib as L
    from osrl_amd.engine.core import cur_stream
    dev = _dev()
    p = dict(x, **{k: (v(x) if callable(v) else v) for k, v in (over or {}).items()})
    args, bufs = [], {}
    for kind, name in OC.spec(kernel):
        v = p.get(name)
        if kind in _BODY:
            if v is None:
                args.append(None)
            elif isinstance(v, str):
                args.append(bufs[v[1:]][0].data_ptr())
            else:
                dtype, fill = _BODY[kind]
                body = _state_bytes(v) if kind == "s" else np.asarray(v, dtype).ravel()
                init = np.concatenate([body, np.full(GUARD, fill, dtype)])
                t = torch.from_numpy(init.copy()).to(dev)
                bufs[name] = (t, len(body), init)
                args.append(t.data_ptr())
        elif kind in ("H", "v"):
            assert v is None
            args.append(None)
        else:
            args.append(float(v) if kind == "f" else int(v))
    rc = getattr(L.load(), "osrl_" + kernel)(*args, cur_stream())
    torch.cuda.synchronize()
    assert rc == expect, (kernel, over, rc)
    got, before = {}, {}
    for name, (t, n, init) in bufs.items():
        a = t.cpu().numpy()
        assert _same(a[n:], init[n:]), f"{kernel}: {name} written past its end"
        if expect != 0:
            assert _same(a, init), f"{kernel}: refused call wrote {name}"
        got[name], before[name] = a[:n], init[:n]
    return got, before


def _words(got):
    """The launch's buffers with the state bytes of ``st`` decoded into st.step, st.bc1, ..."""
    out = dict(got)
    if "st" in got:
        s = got["st"].view(STATE)[0]
        out.update({"st." + k: np.array([s[k]]) for k in STATE.names})
    return out


def check(kernel, x, tag):
    r64, r32 = OO.reference(kernel, x)
    got, before = launch(kernel, x)
    ticked = "st.step" in r64.out
    for name, a in got.items():
        if name in r64.out:
            skip = np.isnan(r64.out[name])
            assert _same(a[skip], before[name][skip]), f"{tag}: {name} written where the launch must leave it alone"
        elif name not in r64.aux.get("free", ()) and not (name == "st" and ticked):
            assert _same(a, before[name]), f"{tag}: the launch wrote its input {name}"
    vals = _words(got)
    worst, where = OO.compare(vals, r64, r32)
    per = OO.by_class(vals, r64, r32)
    for k, v in per.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(f"{tag}: worst |got - fp64| / gate = {worst:.3g} at {where}  " + " ".join(f"{k}={v:.3g}" for k, v in per.items()))
    assert worst <= 1.0, (tag, where, worst)
    return got, before


def _cases(*kernels):
    return [c for c in OC.CASES if c.kernel in kernels]


def _mapped(got, copy, index, src):
    """The packed copy holds the very words the launch stored in the flat buffer."""
    on = index >= 0
    return _same(got[copy][index[on]], got[src][on])


@pytest.mark.parametrize("c", _cases("adam_step", "adam_step_packed"), ids=lambda c: c.id)
def test_adam_step_from_a_planted_state(c):
    x = OC.inputs(c)
    got, before = check(c.kernel, x, c.id)
    z = x["_plant"]["zero"]  # g = 0 with m = v = 0: nothing moves
    assert _same(got["m"][z], before["m"][z]) and _same(got["v"][z], before["v"][z])
    if x["weight_decay"] == 0:
        assert _same(got["p"][z], before["p"][z])
    if c.kernel == "adam_step_packed":
        assert _mapped(got, "pf", x["map_f"], "p")
        if x["map_b"] is not None:
            assert _mapped(got, "pb", x["map_b"], "p")
        if x["tf"] is not None and x["tgt"] is not None:
            assert _mapped(got, "tf", x["map_f"], "tgt")


@pytest.mark.parametrize("c", _cases("polyak"), ids=lambda c: c.id)
def test_polyak_step_alone(c):
    x = OC.inputs(c)
    got, _ = check(c.kernel, x, c.id)
    if x["map_f"] is not None:
        assert _mapped(got, "tf", x["map_f"], "tgt")


@pytest.mark.parametrize("cid", ["adam_step_packed-all", "adam_step_packed-S17-tau1", "adam_step_packed-n4-S9",
                                 "adam_step-step1-b0.5-wd0.5-warm-tau0", "adam_step-big"])
def test_polyak_alone_leaves_the_target_bits_of_the_adam_launch(cid):
    """osrl_polyak on the parameters an Adam launch left and the targets it started from: the targets (and their packed
    copy) that launch left."""
    c = OC.BY_ID[cid]
    x = OC.inputs(c)
    got, _ = launch(c.kernel, x)
    packed = c.kernel == "adam_step_packed"
    y = dict(p=got["p"], tgt=x["tgt"], n=x["n"], tau=x["tau"], map_f=x["map_f"] if packed else None,
             tf=x["tf"] if packed else None)
    alone, _ = launch("polyak", y)
    assert _same(alone["tgt"], got["tgt"])
    if packed:
        assert _same(alone["tf"], got["tf"])


@pytest.mark.parametrize("c", _cases("reduce_slabs"), ids=lambda c: c.id)
def test_reduce_slabs_is_the_fp32_sum_in_slab_order_bit_for_bit(c):
    x = OC.inputs(c)
    got, _ = check(c.kernel, x, c.id)
    want = OO.reference(c.kernel, x)[0].out["flat"][:x["n"]]
    assert _same(got["flat"][:x["n"]], want)


@pytest.mark.parametrize("c", _cases("reduce_slabs_counts"), ids=lambda c: c.id)
def test_reduce_slabs_counts_adds_each_chunks_own_count_and_no_more(c):
    x = OC.inputs(c)
    got, _ = check(c.kernel, x, c.id)
    assert _same(got["flat"], OO.reference(c.kernel, x)[0].out["flat"])
    if "zeros" in c.tag:  # zeros past each count: the plain sum of the largest count
        y = dict(flat=x["flat"], slabs=x["slabs"], n_splits=int(x["counts"].max()), slab_stride=x["slab_stride"], n=x["n"])
        plain, _ = launch("reduce_slabs", y)
        assert _same(plain["flat"], got["flat"])


@pytest.mark.parametrize("c", _cases("step_tick", "step_tick_peer", "step_begin_peer_w"), ids=lambda c: c.id)
def test_step_tick_words_and_ring(c):
    x = OC.inputs(c)
    got, _ = check(c.kernel, x, c.id)
    if "noise" in got:
        assert np.isfinite(got["noise"]).all()


@pytest.mark.parametrize("row", OC.TICK_ROWS, ids=lambda r: r[0])
def test_step_begin_leaves_the_bytes_of_the_tick(row):
    """osrl_step_begin_peer_w (no gather, a 4-float noise buffer) restates the tick arithmetic: the same 24 state bytes and
    the same ring bytes as osrl_step_tick_peer on the same inputs."""
    tag, kw = row
    tick, _ = launch("step_tick_peer", OC.tick_inputs(with_peer_arg=True, **kw))
    begin, _ = launch("step_begin_peer_w", OC.tick_inputs(begin=True, **kw))
    assert _same(tick["st"], begin["st"]), (tag, tick["st"].view(OO.F), begin["st"].view(OO.F))
    if "ring" in tick:
        assert _same(tick["ring"], begin["ring"]), tag


def _refusal_base(kernel):
    first = {"adam_step": "adam_step-S9", "adam_step_packed": "adam_step_packed-all", "polyak": "polyak-tau0.005-map",
             "reduce_slabs": "reduce_slabs-S9-out", "step_tick_peer": "step_tick_peer-own5-peer9", "step_begin_peer_w": "step_begin_peer_w-own5-peer9"}
    return OC.BY_ID[first[kernel]] if kernel in first else _cases(kernel)[0]


@pytest.mark.parametrize("kernel", sorted(OC.REFUSALS))
def test_argument_errors_are_refused_before_any_launch(kernel):
    x = OC.inputs(_refusal_base(kernel))
    for over in OC.REFUSALS[kernel]:
        launch(kernel, x, over=over, expect=-1)


def test_every_entry_point_is_in_the_table():
    assert {c.kernel for c in OC.CASES} == set(OC.SPECS) == set(OC.REFUSALS)
