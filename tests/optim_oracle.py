"""Plain numpy restatements of the optimizer tail of csrc/optim.hip -- the slab sums, Adam / AdamW with the Polyak target
and the packed-copy refresh, the Polyak step alone, the step tick -- and of the tick arithmetic restated in csrc/rng.hip
(osrl_step_begin_peer_w).  TEST INFRASTRUCTURE ONLY: nothing here calls code under ``osrl_amd/``.

Every ``ref_<entry point>(x, dt)`` takes the input dict of an ``optim_cases.Case`` and a dtype: ``np.float64`` is the
reference, ``np.float32`` the "honest fp32" run of the same formula, used only to size the "trans" gates.  It returns a
``loss_oracle.Ref``; ``reference`` turns every gate into an explicit absolute gate per element (``Ref.gate``), so that
``loss_oracle.compare`` is the comparison.

Hyper-parameters enter as their fp32 values widened to fp64 (that is what the kernel receives; 1 - b1 and 1 - b2 are
then exact).  The state words ``bc1`` / ``bc2_sqrt`` / ``lr_scale`` enter as the case gives them (the cases give fp32
values, the torch comparison of tests/test_optim_oracle_cpu.py gives fp64 ones).

    g = (sum_s slab_s, in slab order, fp32) * gscale      lr_t = lr * lr_scale
    p <- p (1 - lr_t wd)  when wd != 0                    (torch.optim.AdamW)
    m <- b1 m + (1 - b1) g ;  v <- b2 v + (1 - b2) g^2
    p <- p - (lr_t / bc1) m / (sqrt(v) / bc2_sqrt + eps)  (torch.optim.Adam, adam.h)
    tgt <- tau p + (1 - tau) tgt                          (cpq.py:107-113 _soft_update)
    pf[map_f[i]] = p[i], pb[map_b[i]] = p[i], tf[map_f[i]] = tgt[i] where the map is >= 0; other words stay (NaN here)
    tick: t = max(own, peer) + 1; bc1 = fp32(1 - b1^t); bc2_sqrt = fp32(sqrt(1 - b2^t)); lr_scale = fp32(min(t / warmup, 1))
          or 1 when warmup <= 0; the own previous statistics go to ring slot (own - 1) % max(ring_len, 1) when own >= 1 and
          both pointers are given; arrive_ stays 0.

Gates (all derived here, none tuned on the GPU)
-----------------------------------------------
"exact"  slab sums: bit-equal to the fp32 accumulation one slab at a time in slab order (the header promises the order, a
         chain of IEEE adds has no contraction to choose from, the build uses no fast-math); ``step``, ``lr_scale``
         (one correctly rounded fp64 divide, one conversion), ``arrive_`` and the ring words.
"arith"  m, v, and the target of the Polyak step alone: 8 ulp of the largest intermediate.  Both runs start from the fp32
         in-order sum, so the slab sum's own rounding is not part of this comparison.  (Worst case by hand: the rounding
         of g * gscale, of (1 - b) g [and of its product with g], of the fused multiply-add: <= 2.5 ulp of the scale.)
"trans"  p, tgt, pf, pb, tf (through sqrtf and two divides): 8 x this oracle's own fp32-vs-fp64 error relative to the
         scale, floor 4 ulp, cap 5e-5 (loss_oracle.GRAD_CAP).  scale(p) = max(|p decay|, |dp|): on the p = 0 plants the
         gate is relative to the update alone.  scale(tgt) = max(tau scale(p), |(1 - tau) tgt|).
"ulp1"   bc1, bc2_sqrt: 1 fp32 ulp of the fp64 value (the device's double pow is not proven correctly rounded, and a
         double-rounding boundary can move the fp32 result by one).
Every state-word gate has an absolute floor of 2^-126: a result in the subnormal range is not gated on flush behaviour
nobody has measured on this chip.

Worst |got - fp64| / gate per class over the whole table on an MI355X (2026-10-21, tests/test_gpu_optim_kernels.py prints
them): exact 0, arith 0.128, trans 0.171, ulp1 0.498 (bc1 and bc2_sqrt are the correctly rounded fp32 values on every row;
"trans" is 0.125 = 1/8 on most cases: at the honest fp32 run's worst element the kernel has that run's error).
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict

import numpy as np

import loss_oracle as LO
from loss_oracle import Ref, compare  # noqa: F401  (the comparison the CPU and GPU tests share)

F = np.float32
TINY = 2.0 ** -126

_MUT: set = set()
MUTATIONS = ("drop_last", "drop_8", "swap_12", "no_gscale", "decay_after", "decay_lr", "no_lr_scale", "eps_in_root",
             "bc2_not_root", "no_bc1", "tau_swapped", "tf_from_p", "ring_slot_t", "no_peer", "bc1_prev")


@contextlib.contextmanager
def mutate(name):
    assert name in MUTATIONS
    _MUT.add(name)
    try:
        yield
    finally:
        _MUT.discard(name)


def _on(name) -> bool:
    return name in _MUT


def _mx(*arrs):
    m = np.abs(np.asarray(arrs[0], np.float64))
    for a in arrs[1:]:
        m = np.maximum(m, np.abs(np.asarray(a, np.float64)))
    return m


def _exact(r: Ref, name, val):
    r.put(name, val, "exact")
    r.gate[name] = np.zeros(np.shape(r.out[name]))


# ---- slab sums -------------------------------------------------------------------------------------------------------------
def slab_sum32(buf, n_splits, stride, n, lo=0, hi=None):
    """fp32 sum of elements [lo, hi) of the first n_splits slabs, one slab at a time in slab order."""
    hi = n if hi is None else hi
    order = list(range(n_splits))
    if _on("drop_last") and n_splits > 1:
        order = order[:-1]
    if _on("drop_8") and n_splits > 8:
        order.remove(8)
    if _on("swap_12") and len(order) > 2:
        order[1], order[2] = order[2], order[1]
    buf = np.asarray(buf, F)
    g = buf[order[0] * stride + lo:order[0] * stride + hi].copy()
    for s in order[1:]:
        g = g + buf[s * stride + lo:s * stride + hi]
    assert g.dtype == F
    return g


def ref_reduce_slabs(x, dt):
    r = Ref()
    n, S, stride = x["n"], x["n_splits"], x["slab_stride"]
    in_place = isinstance(x["slabs"], str)
    buf = x["flat"] if in_place else x["slabs"]
    out = np.full(len(x["flat"]), np.nan, F)
    out[:n] = slab_sum32(buf, S, stride, n)
    _exact(r, "flat", out)
    return r


def ref_reduce_slabs_counts(x, dt):
    r = Ref()
    n, stride = x["n"], x["slab_stride"]
    out = np.full(n, np.nan, F)
    for c, k in enumerate(x["counts"]):
        lo, hi = c * 1024, min((c + 1) * 1024, n)
        out[lo:hi] = slab_sum32(x["slabs"], int(k), stride, n, lo, hi)
    _exact(r, "flat", out)
    return r


# ---- Adam / AdamW, Polyak, packed copies -----------------------------------------------------------------------------------
def _polyak(tau, p, t0, dt):
    a, b = (dt(1.0) - tau, tau) if _on("tau_swapped") else (tau, dt(1.0) - tau)
    return a * p + b * t0, a, b


def _scatter(n_out, index, val, fill=np.nan, dtype=np.float64):
    out = np.full(n_out, fill, dtype)
    on = index >= 0
    out[index[on]] = val[on]
    return out


def _adam(x, dt, packed):
    r = Ref()
    n, S, stride = x["n"], x["n_splits"], x["slab_stride"]
    h = lambda k: dt(x[k])  # noqa: E731
    lr, b1, b2, eps, wd, tau = h("lr"), h("beta1"), h("beta2"), h("eps"), h("weight_decay"), h("tau")
    st = x["st"]
    bc1, bc2s, lrs = dt(st["bc1"]), dt(st["bc2_sqrt"]), dt(st["lr_scale"])
    g32 = slab_sum32(x["slabs"], S, stride, n)
    gs = dt(1.0) if (x.get("gscale") is None or _on("no_gscale")) else dt(x["gscale"][0])
    g = g32.astype(dt) * gs
    lr_t = lr * (dt(1.0) if _on("no_lr_scale") else lrs)
    decay = dt(1.0) - (lr if _on("decay_lr") else lr_t) * wd
    p0, m0, v0 = (np.asarray(x[k], dt) for k in ("p", "m", "v"))
    pd = p0 * decay if (x["weight_decay"] != 0 and not _on("decay_after")) else p0
    mg, vg = (dt(1.0) - b1) * g, ((dt(1.0) - b2) * g) * g
    m, v = b1 * m0 + mg, b2 * v0 + vg
    if _on("eps_in_root"):
        d = np.sqrt(v + eps) / bc2s
    elif _on("bc2_not_root"):
        d = np.sqrt(v) / (bc2s * bc2s) + eps
    else:
        d = np.sqrt(v) / bc2s + eps
    dp = (lr_t / (dt(1.0) if _on("no_bc1") else bc1)) * (m / d)
    p = pd - dp
    if _on("decay_after") and x["weight_decay"] != 0:
        p = p * decay
    s_p = _mx(pd, dp)
    r.put("m", m, "arith", _mx(b1 * m0, mg, m))
    r.put("v", v, "arith", _mx(b2 * v0, vg, v))
    r.put("p", p, "trans", s_p)
    t = s_t = None
    if x.get("tgt") is not None:
        t0 = np.asarray(x["tgt"], dt)
        t, a, b = _polyak(tau, p, t0, dt)
        s_t = np.maximum(float(a) * s_p, _mx(b * t0))
        r.put("tgt", t, "trans", s_t)
    if packed:
        mf = np.asarray(x["map_f"])
        r.put("pf", _scatter(len(x["pf"]), mf, p, dtype=dt), "trans", _scatter(len(x["pf"]), mf, s_p, 1.0))
        if x.get("map_b") is not None:
            mb = np.asarray(x["map_b"])
            r.put("pb", _scatter(len(x["pb"]), mb, p, dtype=dt), "trans", _scatter(len(x["pb"]), mb, s_p, 1.0))
        if x.get("tf") is not None:
            if t is None:
                r.put("tf", np.full(len(x["tf"]), np.nan, dt), "trans")
            else:
                src, sc = (p, s_p) if _on("tf_from_p") else (t, s_t)
                r.put("tf", _scatter(len(x["tf"]), mf, src, dtype=dt), "trans", _scatter(len(x["tf"]), mf, sc, 1.0))
    return r


def ref_adam_step(x, dt):
    return _adam(x, dt, False)


def ref_adam_step_packed(x, dt):
    return _adam(x, dt, True)


def ref_polyak(x, dt):
    r = Ref()
    p, t0 = np.asarray(x["p"], dt), np.asarray(x["tgt"], dt)
    t, a, b = _polyak(dt(x["tau"]), p, t0, dt)
    s_t = _mx(a * p, b * t0)
    r.put("tgt", t, "arith", s_t)
    if x.get("map_f") is not None:
        mf = np.asarray(x["map_f"])
        src = p if _on("tf_from_p") else t
        r.put("tf", _scatter(len(x["tf"]), mf, src, dtype=dt), "arith", _scatter(len(x["tf"]), mf, s_t, 1.0))
    return r


# ---- the tick ----------------------------------------------------------------------------------------------------------------
def tick_words(t, beta1, beta2, warmup):
    """(1 - b1^t, sqrt(1 - b2^t), min(t / warmup, 1)) in fp64, the betas as fp32 values."""
    b1, b2 = float(F(beta1)), float(F(beta2))
    with np.errstate(under="ignore"):
        p1, p2 = float(np.power(np.float64(b1), np.float64(t))), float(np.power(np.float64(b2), np.float64(t)))
    return 1.0 - p1, math.sqrt(1.0 - p2), (min(float(t) / float(warmup), 1.0) if warmup > 0 else 1.0)


def _tick(x, dt, begin=False):
    r = Ref()
    own = int(x["st"]["step"])
    peer = x.get("peer")
    t_old = own if (peer is None or _on("no_peer")) else max(own, int(peer["step"]))
    t = t_old + 1
    bc1, bc2s, lrs = tick_words(t, x["beta1"], x["beta2"], x["warmup"])
    if _on("bc1_prev"):
        bc1 = tick_words(t - 1, x["beta1"], x["beta2"], x["warmup"])[0]
    rnd = (lambda v: v) if dt is np.float64 else (lambda v: float(F(v)))
    _exact(r, "st.step", np.array([float(t)]))
    _exact(r, "st.lr_scale", np.array([float(F(lrs))]))
    _exact(r, "st.arrive", np.array([0.0]))
    for name, v in (("st.bc1", bc1), ("st.bc2_sqrt", bc2s)):
        r.put(name, np.array([rnd(v)]), "ulp1")
        r.gate[name] = np.array([float(np.spacing(F(abs(v))))])
    if x.get("ring") is not None:
        ns, rl = x["n_stats"], max(x["ring_len"], 1)
        ring = np.full(len(x["ring"]), np.nan, F)
        if x.get("stats_cur") is not None and own >= 1:
            slot = (own if _on("ring_slot_t") else own - 1) % rl
            ring[slot * ns:(slot + 1) * ns] = x["stats_cur"]
        _exact(r, "ring", ring)
    if begin:
        r.aux["free"] = ("noise",)  # written by the launch, no part of this comparison
    return r


def ref_step_tick(x, dt):
    return _tick(x, dt)


ref_step_tick_peer = ref_step_tick


def ref_step_begin_peer_w(x, dt):
    return _tick(x, dt, begin=True)


REFS = {k[4:]: v for k, v in list(globals().items()) if k.startswith("ref_")}


# ---- gates and comparison ------------------------------------------------------------------------------------------------------
def reference(kernel: str, x, mutation=None):
    """(fp64 Ref, honest-fp32 Ref) of one case's inputs; the fp64 Ref carries the absolute gate of every element."""
    fn = REFS[kernel]
    with np.errstate(all="ignore"):
        if mutation is None:
            r64, r32 = fn(x, np.float64), fn(x, np.float32)
        else:
            with mutate(mutation):
                r64, r32 = fn(x, np.float64), fn(x, np.float32)
        for name, (rel, sc) in LO.gate_parts(r64, r32).items():
            if name not in r64.gate:
                r64.gate[name] = np.maximum(rel * sc, TINY)
    return r64, r32


def by_class(got, r64: Ref, r32: Ref) -> Dict[str, float]:
    """Worst |got - fp64| / gate per gate class."""
    out: Dict[str, float] = {}
    for name in r64.out:
        sub = Ref()
        sub.out, sub.cls, sub.gate = {name: r64.out[name]}, {name: r64.cls[name]}, {name: r64.gate[name]}
        out[r64.cls[name]] = max(out.get(r64.cls[name], 0.0), compare(got, sub, r32)[0])
    return out
