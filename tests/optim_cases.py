"""One table of cases for the optimizer tail of csrc/optim.hip (and the tick arithmetic restated in csrc/rng.hip), shared
by tests/test_optim_oracle_cpu.py and tests/test_gpu_optim_kernels.py.

``SPECS[kernel]`` is the argument list of ``osrl_<kernel>`` in the order and with the parameter names of
include/osrl_amd.h: ``p:`` a device float buffer, ``q:`` a device int32 buffer, ``b:`` a device uint8 buffer, ``s:`` a
24-byte ``osrl_step_state_t`` written by the test, ``i:`` int32, ``l:`` int64, ``u:`` uint32, ``U:`` uint64, ``f:``
float, ``H:`` a host array and ``v:`` a device pointer that these cases always pass as NULL.  The stream is appended by
the caller.  A buffer whose value is the string ``"=name"`` is the SAME device buffer as ``name`` (the in-place slab sum,
``peer == st``).

Every Adam case is ONE step from a planted state, so it depends neither on the tick nor on an earlier step.  Shapes are
the smallest that reach each path of the kernels: ``n = 4 * 257`` is one full 256-thread workgroup and one lane of the
next; ``n_splits`` walks the up-front eight loads, the 8-deep loop of ``slab_sum_from`` alone, with tails of 1 and 7, and
several times; ``BIG_N`` (``n4 = 2048 * 256 + 257``) is the grid-stride second pass with a ragged end.  A quarter of
the elements of every Adam case are plants (``x['_plant']``: kind -> element indices), one per float4 on a rotating lane:

``p0``      p = 0 (the update is visible at full precision, not under ulp(p)); the gradient has the sign of m, so that
            the first moment does not cancel and the gate of these elements stays a few ulp of the update
``zero``    g = 0 with m = v = 0: p (without weight decay), m and v come back bit-identical
``zero_mv`` g = 0 with the state's moments, p = 0
``eps``     |g| ~ 1e-8 and v ~ 1e-16 with p = 0: sqrt(v) / bc2_sqrt is of the order of eps, which tells eps outside the
            root from inside it and sqrt(v) / bc2_sqrt from sqrt(v) / bc2
``big``     |g| = 1e15 (g^2 finite; overflow is no contract), ``tiny`` |g| = 1e-25 (g^2 underflows)
``cancel``  slabs (+x, -x, y, ...) with |x| ~ 1e8: any other summation order loses y
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, List

import numpy as np

F = np.float32
N1 = 4 * 257
BIG_N = 4 * (2048 * 256 + 257)
KINDS = ("p0", "zero", "zero_mv", "eps", "big", "tiny", "cancel")

_ADAM = "p:p p:m p:v p:tgt p:slabs i:n_splits l:slab_stride l:n f:lr f:beta1 f:beta2 f:eps f:weight_decay f:tau p:gscale s:st"
_TICK = "f:beta1 f:beta2 i:warmup p:stats_cur p:ring i:n_stats i:ring_len"
_BEGIN = (" p:noise l:noise_n U:noise_seed u:noise_stream i:n_fields H:src H:dst H:width H:scale l:n_rows i:batch "
          "U:gather_seed u:gather_stream v:cum")
SPECS: Dict[str, str] = {
    "adam_step": _ADAM,
    "adam_step_packed": _ADAM + " q:map_f q:map_b p:pf p:pb p:tf",
    "polyak": "p:p p:tgt l:n f:tau q:map_f p:tf",
    "reduce_slabs": "p:flat p:slabs i:n_splits l:slab_stride l:n",
    "reduce_slabs_counts": "p:flat p:slabs b:counts l:slab_stride l:n",
    "step_tick": "s:st " + _TICK,
    "step_tick_peer": "s:st s:peer " + _TICK,
    "step_begin_peer_w": "s:st s:peer " + _TICK + _BEGIN,
}


def spec(kernel) -> List[tuple]:
    return [tuple(a.split(":")) for a in SPECS[kernel].split()]


def _stride2(x):
    return x["n"] + 2


# argument errors the host code refuses with -1 before any launch; every buffer keeps its bits.  (A callable is resolved
# on the case's inputs.)
_SIZES = [dict(n=0), dict(n=2), dict(n=6), dict(slab_stride=_stride2)]
_ADAM_REF = _SIZES + [dict(n_splits=0), dict(p=None), dict(m=None), dict(v=None), dict(slabs=None), dict(st=None)]
REFUSALS: Dict[str, List[dict]] = {
    "adam_step": _ADAM_REF,
    "adam_step_packed": _ADAM_REF + [dict(map_f=None), dict(pf=None), dict(pb=None)],  # (the last: map_b without pb)
    "polyak": [dict(tf=None), dict(n=6), dict(n=0), dict(p=None), dict(tgt=None)],     # (the first: map_f without tf)
    "reduce_slabs": _SIZES + [dict(n_splits=0), dict(flat=None), dict(slabs=None)],
    "reduce_slabs_counts": _SIZES + [dict(counts=None), dict(flat=None), dict(slabs=None)],
    "step_tick": [dict(st=None)],
    "step_tick_peer": [dict(st=None), dict(peer="=st")],
    "step_begin_peer_w": [dict(st=None), dict(peer="=st")],
}


@dataclass
class Case:
    kernel: str
    tag: str
    build: Callable[[], dict]

    @property
    def id(self):
        return f"{self.kernel}-{self.tag}"


def inputs(c: Case) -> dict:
    return c.build()


def f32(v) -> float:
    """A hyper-parameter as the kernel receives it: its fp32 value, widened."""
    return float(F(v))


def state(step, betas=(0.9, 0.999), lr_scale=1.0) -> dict:
    """The state words a tick leaves at ``step`` (fp64 arithmetic, stored as fp32), with a planted warm-up factor."""
    b1, b2 = f32(betas[0]), f32(betas[1])
    with np.errstate(under="ignore"):
        p1, p2 = float(np.power(np.float64(b1), float(step))), float(np.power(np.float64(b2), float(step)))
    return dict(step=int(step), bc1=f32(1.0 - p1), bc2_sqrt=f32(math.sqrt(1.0 - p2)), lr_scale=f32(lr_scale))


def _signs(rs, k):
    return np.where(rs.uniform(size=k) < 0.5, -1.0, 1.0)


def slab_buffer(rs, n_splits, n, pad):
    """[n_splits, n + pad] of N(0, 1); the gap between slabs holds 777 (a stride / length confusion adds it)."""
    stride = n + pad
    buf = np.full((n_splits, stride), 777.0, F)
    buf[:, :n] = rs.standard_normal((n_splits, n))
    return buf


def plant_cancel(rs, view, idx):
    """(+x, -x, y, ...) with |x| in [1e7, 1e9] on the elements ``idx`` of the slab view [n_splits, .]."""
    S = view.shape[0]
    if S < 2 or len(idx) == 0:
        return
    xv = (_signs(rs, len(idx)) * 10.0 ** rs.uniform(7, 9, size=len(idx))).astype(F)
    view[0, idx], view[1, idx] = xv, -xv


def plant_index(n):
    j = np.arange(n // 4)
    return 4 * j + (j % 4), j % len(KINDS), j


def pack_maps(n):
    """map_f: -1 runs (one across a float4 boundary, one of 9, every 7th element), the rest in DESCENDING order with a gap
    every 16; map_b: ascending from 3 with a gap every 8 and every 5th element unmapped."""
    on = np.ones(n, bool)
    if n >= 8:
        on[2:6] = False
        on[n // 2:n // 2 + 9] = False
        on[::7] = False
    else:
        on[1] = False
    k = int(on.sum())
    n_f = n + n // 16 + 37
    mf = np.full(n, -1, np.int32)
    mf[on] = n_f - 1 - (np.arange(k) + np.arange(k) // 16)
    onb = (np.arange(n) % 5) != 1
    kb = int(onb.sum())
    n_b = n + n // 8 + 20
    mb = np.full(n, -1, np.int32)
    mb[onb] = 3 + np.arange(kb) + np.arange(kb) // 8
    assert mf.max() < n_f and mf[on].min() >= 0 and mb.max() < n_b and len(set(mf[on])) == k
    return mf, n_f, mb, n_b


def adam_inputs(seed, n=N1, S=3, pad=8, step=3, betas=(0.9, 0.999), wd=0.0, gscale=None, lr_scale=1.0, tgt=True,
                tau=0.005, lr=1e-3, packed=None):
    rs = np.random.RandomState(seed)
    slabs = slab_buffer(rs, S, n, pad)
    p = (_signs(rs, n) * (0.5 + np.abs(rs.standard_normal(n)))).astype(F)
    if step > 1:
        m = rs.standard_normal(n).astype(F)
        v = ((0.5 + np.abs(rs.standard_normal(n))) ** 2).astype(F)
    else:
        m, v = np.zeros(n, F), np.zeros(n, F)
    t0 = rs.standard_normal(n).astype(F)
    idx, kind, j = plant_index(n)
    u = lambda k: 1.0 + 0.5 * rs.uniform(size=k)  # noqa: E731
    plant = {}
    for k, name in enumerate(KINDS):
        i = idx[kind == k]
        alt = ((j[kind == k] // len(KINDS)) % 2) == 0
        plant[name] = i
        if len(i) == 0:
            continue
        s = _signs(rs, len(i))
        if name == "p0":
            p[i] = 0
            sg = np.where(m[i] < 0, -1.0, 1.0)
            slabs[:, i] = np.abs(slabs[:, i]) * sg
        elif name == "zero":
            slabs[:, i] = 0
            m[i], v[i] = 0, 0
        elif name == "zero_mv":
            slabs[:, i] = 0
            p[i] = 0
        elif name == "eps":
            p[i] = 0
            slabs[:, i] = 0
            slabs[0, i] = s * 1e-8 * u(len(i))
            if step > 1:
                m[i], v[i] = s * 1e-8 * u(len(i)), 1e-16 * u(len(i))
        elif name in ("big", "tiny"):
            slabs[:, i] = 0
            slabs[0, i] = s * (1e15 if name == "big" else 1e-25) * u(len(i))
            p[i[alt]] = 0
            m[i] = np.abs(m[i]) * s
        else:
            plant_cancel(rs, slabs, i)
    x = dict(p=p, m=m, v=v, tgt=t0 if tgt else None, slabs=slabs.ravel(), n_splits=S, slab_stride=n + pad, n=n,
             lr=f32(lr), beta1=f32(betas[0]), beta2=f32(betas[1]), eps=f32(1e-8), weight_decay=f32(wd), tau=f32(tau),
             gscale=None if gscale is None else np.array([gscale], F), st=state(step, betas, lr_scale), _plant=plant)
    if packed is not None:
        mf, n_f, mb, n_b = pack_maps(n)
        x.update(map_f=mf, map_b=mb if packed["map_b"] else None, pf=np.full(n_f, np.nan, F),
                 pb=np.full(n_b, np.nan, F) if packed["map_b"] else None, tf=np.full(n_f, np.nan, F) if packed["tf"] else None)
    return x


def polyak_inputs(seed, n, tau, with_map):
    rs = np.random.RandomState(seed)
    p, t0 = rs.standard_normal(n).astype(F), rs.standard_normal(n).astype(F)
    p[1::9], t0[2::11] = 0, 0
    x = dict(p=p, tgt=t0, n=n, tau=f32(tau), map_f=None, tf=None)
    if with_map:
        mf, n_f, _, _ = pack_maps(n)
        x.update(map_f=mf, tf=np.full(n_f, np.nan, F))
    return x


def reduce_inputs(seed, n, S, pad, in_place):
    rs = np.random.RandomState(seed)
    slabs = slab_buffer(rs, S, n, pad)
    plant_cancel(rs, slabs, np.arange(6, n, 7))
    x = dict(n_splits=S, slab_stride=n + pad, n=n)
    if in_place:
        x.update(flat=slabs.ravel(), slabs="=flat")
    else:
        x.update(flat=np.full(n, np.nan, F), slabs=slabs.ravel())
    return x


def counts_inputs(seed, n, counts, alloc, planted):
    """Slabs past a 1024-float chunk's own count hold zeros, or (``planted``) values of order 1000 that must not be added."""
    rs = np.random.RandomState(seed)
    slabs = slab_buffer(rs, alloc, n, 8)
    plant_cancel(rs, slabs, np.arange(6, n, 7))
    for c, k in enumerate(counts):
        lo, hi = c * 1024, min((c + 1) * 1024, n)
        slabs[k:, lo:hi] = (1000.0 + rs.standard_normal((alloc - k, hi - lo))) if planted else 0.0
    return dict(flat=np.full(n, np.nan, F), slabs=slabs.ravel(), counts=np.array(counts, np.uint8), slab_stride=n + 8,
                n=n, _alloc=alloc)


JUNK = dict(bc1=7.0, bc2_sqrt=-3.0, lr_scale=11.0)  # what the state holds before the tick (every word must be rewritten)


def tick_inputs(own, peer=None, betas=(0.9, 0.999), warmup=0, n_stats=3, ring_len=3, stats=True, ring=True, begin=False,
                with_peer_arg=False):
    rl = max(ring_len, 1)
    x = dict(st=dict(step=int(own), **JUNK), beta1=f32(betas[0]), beta2=f32(betas[1]), warmup=warmup,
             stats_cur=(np.arange(n_stats) + 0.5 + (own % 1000)).astype(F) if stats else None,
             ring=np.full(rl * n_stats, np.nan, F) if ring else None, n_stats=n_stats, ring_len=ring_len)
    if peer is not None or begin or with_peer_arg:
        x["peer"] = None if peer is None else dict(step=int(peer), bc1=0.25, bc2_sqrt=0.125, lr_scale=0.5)
    if begin:
        x.update(noise=np.full(4, np.nan, F), noise_n=4, noise_seed=1234, noise_stream=3, n_fields=0, src=None, dst=None,
                 width=None, scale=None, n_rows=0, batch=0, gather_seed=0, gather_stream=0, cum=None)
    return x


def _tick_rows():
    rows = []
    for t_old in (0, 1, 2, 999, 10 ** 4, 10 ** 6, 2 ** 31):
        for betas in ((0.9, 0.999), (0.5, 0.5), (0.9, 0.95), (0.0, 0.0)):
            rows.append((f"t{t_old}-b{betas[0]}_{betas[1]}", dict(own=t_old, betas=betas)))
    # t at which sqrtf(fp32(1 - b2^t)) is not fp32(sqrt(1 - b2^t)) (at t = 2, 3, 4 the same holds for a single-precision
    # power in bc1): a restatement of the tick in float leaves other bytes here, on the rest of the table it does not
    for betas, olds in (((0.9, 0.999), (9, 10, 28)), ((0.9, 0.95), (6, 10, 20))):
        for t_old in olds:
            rows.append((f"froot-t{t_old}-b{betas[0]}_{betas[1]}", dict(own=t_old, betas=betas)))
    for w, olds in ((1, (0, 5)), (3, (0, 1, 2, 3)), (500, (0, 499, 500))):
        for t_old in olds:
            rows.append((f"warm{w}-t{t_old}", dict(own=t_old, warmup=w)))
    for own, peer in ((5, 9), (9, 5), (7, 7)):
        rows.append((f"own{own}-peer{peer}", dict(own=own, peer=peer, warmup=20, betas=(0.9, 0.95))))
    for ns in (1, 63, 64, 65, 200):
        rows.append((f"ring-ns{ns}", dict(own=5, n_stats=ns)))
    for rl in (1, 3, 256, 0):
        for t_old in (0, max(rl, 1), max(rl, 1) + 1):
            rows.append((f"ring-len{rl}-t{t_old}", dict(own=t_old, n_stats=5, ring_len=rl)))
    rows.append(("no-stats", dict(own=2, stats=False)))
    rows.append(("no-ring", dict(own=2, ring=False)))
    return rows


TICK_ROWS = _tick_rows()


def _cases() -> List[Case]:
    out: List[Case] = []
    seed = [100]

    def add(kernel, tag, fn, **kw):
        seed[0] += 1
        s = seed[0]
        out.append(Case(kernel, tag, (lambda: fn(s, **kw)) if fn is not tick_inputs else (lambda: fn(**kw))))

    # ---- Adam: the slab count (step-3 state, Polyak target) ---------------------------------------------------------
    for S in (1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 32):
        add("adam_step", f"S{S}", adam_inputs, S=S, pad=0 if S in (9, 16) else 8)
    # ---- Adam: the size ------------------------------------------------------------------------------------------------
    for n in (4, 4 * 255, 4 * 256):
        add("adam_step", f"n{n}", adam_inputs, n=n, S=3)
    add("adam_step", "big", adam_inputs, n=BIG_N, S=2)
    # ---- Adam: the settings, crossed sparsely ------------------------------------------------------------------------
    add("adam_step", "step1-wd1e-4-gs1-notgt", adam_inputs, step=1, wd=1e-4, gscale=1.0, tgt=False)
    add("adam_step", "step3-wd0.5-gs0.25-warm-tau0.25", adam_inputs, wd=0.5, gscale=0.25, lr_scale=0.002, tau=0.25)
    add("adam_step", "step1e6-gs0-tau1", adam_inputs, step=10 ** 6, gscale=0.0, tau=1.0)
    add("adam_step", "step1-b0.5-wd0.5-warm-tau0", adam_inputs, step=1, betas=(0.5, 0.5), wd=0.5, lr_scale=0.002, tau=0.0)
    add("adam_step", "step1e6-b0.5-wd1e-4-gs0.25-S9", adam_inputs, step=10 ** 6, betas=(0.5, 0.5), wd=1e-4, gscale=0.25, S=9)
    add("adam_step", "step3-warm-notgt-S17", adam_inputs, lr_scale=0.002, tgt=False, S=17, pad=0)
    add("adam_step", "step1-gs1-S32", adam_inputs, step=1, gscale=1.0, S=32)
    add("adam_step", "step3-wd0.5", adam_inputs, wd=0.5)
    add("adam_step", "step1e6-wd0.5-gs0.25", adam_inputs, step=10 ** 6, wd=0.5, gscale=0.25)
    # ---- packed ----------------------------------------------------------------------------------------------------------
    add("adam_step_packed", "all", adam_inputs, packed=dict(map_b=True, tf=True))
    add("adam_step_packed", "nomapb-notf", adam_inputs, packed=dict(map_b=False, tf=False), wd=1e-4)
    add("adam_step_packed", "tf-without-tgt", adam_inputs, packed=dict(map_b=True, tf=True), tgt=False, step=1)
    add("adam_step_packed", "n4-S9", adam_inputs, n=4, S=9, packed=dict(map_b=True, tf=True), wd=1e-4, gscale=0.25)
    add("adam_step_packed", "S17-tau1", adam_inputs, S=17, pad=0, packed=dict(map_b=True, tf=True), tau=1.0)
    # ---- Polyak ----------------------------------------------------------------------------------------------------------
    for tau in (0.0, 0.005, 1.0):
        for wm in (False, True):
            add("polyak", f"tau{tau}-{'map' if wm else 'nomap'}", polyak_inputs, n=N1, tau=tau, with_map=wm)
    add("polyak", "n4-map", polyak_inputs, n=4, tau=0.005, with_map=True)
    add("polyak", "n4-nomap", polyak_inputs, n=4, tau=0.005, with_map=False)
    add("polyak", "big", polyak_inputs, n=BIG_N, tau=0.005, with_map=False)
    # ---- slab sums -------------------------------------------------------------------------------------------------------
    for S in (1, 2, 3, 8, 9, 10, 16, 17, 25, 33):
        for ip in (True, False):
            add("reduce_slabs", f"S{S}-{'inplace' if ip else 'out'}", reduce_inputs, n=N1, S=S, pad=0 if S in (3, 10) else 8,
                in_place=ip)
    add("reduce_slabs", "big-inplace", reduce_inputs, n=BIG_N, S=2, pad=8, in_place=True)
    add("reduce_slabs", "big-out", reduce_inputs, n=BIG_N, S=3, pad=0, in_place=False)
    for planted in (False, True):
        add("reduce_slabs_counts", f"n3076-{'planted' if planted else 'zeros'}", counts_inputs, n=3 * 1024 + 4,
            counts=[1, 9, 32, 2], alloc=32, planted=planted)
        add("reduce_slabs_counts", f"n1024-{'planted' if planted else 'zeros'}", counts_inputs, n=1024, counts=[1], alloc=4,
            planted=planted)
    # ---- the tick, and the same rows through the step prologue -------------------------------------------------------
    for tag, kw in TICK_ROWS:
        add("step_tick_peer" if kw.get("peer") is not None else "step_tick", tag, tick_inputs, **kw)
    for tag, kw in TICK_ROWS:
        add("step_begin_peer_w", tag, tick_inputs, begin=True, **kw)
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
