"""The fp64 oracle of the optimizer tail (tests/optim_oracle.py) is itself checked here, without a GPU:

* Adam / AdamW equal ``torch.optim.Adam`` / ``torch.optim.AdamW`` in fp64 on three consecutive steps (the oracle is fed its
  own outputs, the warm-up factor comes from ``LambdaLR(min((s + 1) / warmup, 1))``), to 1e-12 relative;
* the Polyak step equals the reference project's soft update (cpq.py:107-113);
* the honest fp32 run of the oracle stays inside every gate on every case of tests/optim_cases.py, so the gates are known
  to be satisfiable before a GPU is touched;
* the gates are sharp: every listed mutation of the oracle pushes at least one case past its gate;
* the case table holds every entry point and slab counts on both sides of 8 and 16, and its argument lists are those of
  include/osrl_amd.h and of ``osrl_amd._lib``.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import optim_cases as OC
import optim_oracle as OO

D = torch.float64
SMALL = [c for c in OC.CASES if "big" not in c.tag]


@pytest.mark.parametrize("decoupled,wd,warmup,betas", [(False, 0.0, 0, (0.9, 0.999)), (True, 1e-4, 0, (0.9, 0.999)),
                                                       (True, 0.5, 2, (0.5, 0.5)), (True, 0.0, 5, (0.9, 0.95))])
def test_oracle_equals_torch_adam_fp64_over_three_steps(decoupled, wd, warmup, betas):
    rs = np.random.RandomState(7)
    n = 64
    lr, eps = OC.f32(1e-3), OC.f32(1e-8)
    b1, b2, wd = OC.f32(betas[0]), OC.f32(betas[1]), OC.f32(wd)
    p = torch.tensor(rs.standard_normal(n), dtype=D, requires_grad=True)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd,
                                                               foreach=False)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: min((s + 1) / warmup, 1.0)) if warmup > 0 else None
    x = dict(p=p.detach().numpy().copy(), m=np.zeros(n), v=np.zeros(n), tgt=None, n_splits=1, slab_stride=n, n=n, lr=lr,
             beta1=b1, beta2=b2, eps=eps, weight_decay=wd, tau=0.0, gscale=None)
    for t in (1, 2, 3):
        g = rs.standard_normal(n).astype(np.float32)  # (pre-summed slabs)
        bc1, bc2s, lrs = OO.tick_words(t, b1, b2, warmup)
        x.update(slabs=g, st=dict(step=t, bc1=bc1, bc2_sqrt=bc2s, lr_scale=lrs))
        r = OO.ref_adam_step(x, np.float64)
        p.grad = torch.tensor(g, dtype=D)
        opt.step()
        if sched is not None:
            sched.step()
        want = p.detach().numpy()
        np.testing.assert_allclose(r.out["p"], want, rtol=1e-12, atol=1e-12)
        state = opt.state[p]
        np.testing.assert_allclose(r.out["m"], state["exp_avg"].numpy(), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(r.out["v"], state["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-15)
        x.update(p=r.out["p"], m=r.out["m"], v=r.out["v"])


def test_oracle_polyak_equals_the_reference_soft_update():
    rs = np.random.RandomState(8)
    p, t0 = rs.standard_normal(100).astype(np.float32), rs.standard_normal(100).astype(np.float32)
    for tau in (0.0, 0.005, 0.25, 1.0):
        tau = OC.f32(tau)
        r = OO.ref_polyak(dict(p=p, tgt=t0, tau=tau, map_f=None), np.float64)
        want = tau * torch.tensor(p, dtype=D) + (1 - tau) * torch.tensor(t0, dtype=D)  # cpq.py:113
        np.testing.assert_allclose(r.out["tgt"], want.numpy(), rtol=1e-15, atol=0)


@pytest.mark.parametrize("c", OC.CASES, ids=lambda c: c.id)
def test_the_oracle_fp32_run_passes_its_own_gates(c):
    r64, r32 = OO.reference(c.kernel, OC.inputs(c))
    worst, where = OO.compare(r32.out, r64, r32)
    assert worst <= 1.0, (c.id, where, worst)


# mutation -> the kernels it applies to
_A = ["adam_step", "adam_step_packed"]
_T = ["step_tick", "step_tick_peer", "step_begin_peer_w"]
APPLIES = {
    "drop_last": _A + ["reduce_slabs", "reduce_slabs_counts"], "drop_8": _A + ["reduce_slabs", "reduce_slabs_counts"],
    "swap_12": ["reduce_slabs", "reduce_slabs_counts"] + _A,
    "no_gscale": ["adam_step"], "decay_after": ["adam_step"], "decay_lr": ["adam_step"], "no_lr_scale": ["adam_step"],
    "eps_in_root": _A, "bc2_not_root": _A, "no_bc1": _A, "tau_swapped": _A + ["polyak"],
    "tf_from_p": ["adam_step_packed", "polyak"], "ring_slot_t": _T, "no_peer": ["step_tick_peer", "step_begin_peer_w"],
    "bc1_prev": _T,
}


@pytest.mark.parametrize("mutation", OO.MUTATIONS)
def test_the_gates_catch_every_mutation(mutation):
    assert set(APPLIES) == set(OO.MUTATIONS)
    for kernel in APPLIES[mutation]:
        worst = 0.0
        for c in SMALL:
            if c.kernel != kernel:
                continue
            x = OC.inputs(c)
            r64, r32 = OO.reference(kernel, x)
            m64, _ = OO.reference(kernel, x, mutation)
            worst = max(worst, OO.compare(m64.out, r64, r32)[0])
        assert worst >= 4.0, (mutation, kernel, worst)


def test_swapping_two_cancelling_slabs_breaks_bit_equality():
    hit = 0
    for c in SMALL:
        if c.kernel != "reduce_slabs" or OC.inputs(c)["n_splits"] < 3:
            continue
        x = OC.inputs(c)
        a = OO.reference(c.kernel, x)[0].out["flat"]
        b = OO.reference(c.kernel, x, "swap_12")[0].out["flat"]
        assert not np.array_equal(a.view(np.uint32), b.view(np.uint32)), c.id
        hit += 1
    assert hit >= 8


def test_the_eps_plants_tell_the_placements_of_eps_and_bc2_apart_on_their_own():
    """The two mutations are caught ON the eps-dominated elements (not merely somewhere in the case)."""
    c = OC.BY_ID["adam_step-S7"]
    x = OC.inputs(c)
    r64, r32 = OO.reference(c.kernel, x)
    i = x["_plant"]["eps"]
    for mutation in ("eps_in_root", "bc2_not_root"):
        m64, _ = OO.reference(c.kernel, x, mutation)
        ratio = np.abs(m64.out["p"] - r64.out["p"])[i] / r64.gate["p"][i]
        assert ratio.min() >= 4.0, (mutation, ratio.min())


def test_the_table_holds_every_entry_point_and_both_sides_of_8_and_16():
    assert {c.kernel for c in OC.CASES} == set(OC.SPECS) == set(OO.REFS) == set(OC.REFUSALS)
    for kernel in ("adam_step", "reduce_slabs"):
        s = {OC.inputs(c)["n_splits"] for c in SMALL if c.kernel == kernel}
        assert {8, 9, 16, 17} <= s and (kernel != "adam_step" or {7, 15} <= s) and min(s) == 1 and max(s) >= 25, (kernel, s)
    big = [c for c in OC.CASES if "big" in c.tag]
    assert {c.kernel for c in big} == {"adam_step", "polyak", "reduce_slabs"}
    assert all(OC.inputs(c)["n"] // 4 == 2048 * 256 + 257 for c in big)
    for c in OC.CASES:
        x = OC.inputs(c)
        if "n" in x:
            assert x["n"] % 4 == 0
        if c.kernel.startswith("adam"):
            k = sum(len(v) for v in x["_plant"].values())
            assert k == x["n"] // 4
            assert np.isfinite(x["slabs"]).all() and (np.abs(x["slabs"][x["slabs"] != 0]) >= 2.0 ** -126).all()


def test_plants_are_what_they_claim():
    x = OC.inputs(OC.BY_ID["adam_step-S9"])
    r64, _ = OO.reference("adam_step", x)
    pl = x["_plant"]
    g = OO.slab_sum32(x["slabs"], x["n_splits"], x["slab_stride"], x["n"])
    assert (x["p"][pl["p0"]] == 0).all() and (g[pl["zero"]] == 0).all() and (g[pl["zero_mv"]] == 0).all()
    for k in ("p", "m", "v"):  # g = 0 with m = v = 0: nothing moves (no weight decay in this case)
        assert np.array_equal(r64.out[k][pl["zero"]], np.asarray(x[k], np.float64)[pl["zero"]])
    assert (np.abs(g[pl["big"]]) >= 1e15).all() and (np.abs(g[pl["tiny"]]) <= 2e-25).all()
    root = np.sqrt(r64.out["v"][pl["eps"]]) / x["st"]["bc2_sqrt"]
    assert ((root > 0.05 * x["eps"]) & (root < 50 * x["eps"])).all()
    # the cancelling pair is exact in slab order: the sum is that of the other slabs
    i = pl["cancel"]
    rest = OO.slab_sum32(x["slabs"][2 * x["slab_stride"]:], x["n_splits"] - 2, x["slab_stride"], x["n"])
    assert np.array_equal(g[i], rest[i]) and (np.abs(x["slabs"][:x["n"]][i]) >= 1e7).all()


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def _header_protos():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "osrl_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(osrl_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [" ".join(p.split()) for p in m.group(2).split(",")]
    return out


@pytest.mark.parametrize("kernel", sorted(OC.SPECS))
def test_argument_lists_match_the_header_and_the_ctypes_table(kernel):
    import ctypes as C
    from osrl_amd import _lib as L
    params = _header_protos()["osrl_" + kernel]
    sp = OC.spec(kernel)
    assert len(params) == len(sp) + 1 and params[-1].replace(" ", "") == "void*stream", params
    argtypes = L.PROTOTYPES["osrl_" + kernel]
    assert len(argtypes) == len(params)
    scalars = {"i": ("int32_t", C.c_int32), "l": ("int64_t", C.c_int64), "f": ("float", C.c_float),
               "u": ("uint32_t", C.c_uint32), "U": ("uint64_t", C.c_uint64)}
    pointers = {"p": "float*", "q": "int32_t*", "b": "uint8_t*", "s": "osrl_step_state_t*", "v": "uint64_t*"}
    for (kind, name), p, at in zip(sp, params, argtypes):
        star = p.rindex("*") if "*" in p else None
        ptype, pname = (p.rsplit(" ", 1) if star is None else (p[:star + 1], p[star + 1:].strip()))
        assert pname == name, (kernel, p, name)
        if kind in scalars:
            assert ptype == scalars[kind][0] and at is scalars[kind][1], (kernel, p, at)
        elif kind in pointers:
            assert ptype.replace("const ", "").replace(" ", "") == pointers[kind] and at is C.c_void_p, (kernel, p, at)
        else:
            assert kind == "H" and ptype.count("*") >= 1, (kernel, p)
    for over in OC.REFUSALS[kernel]:
        assert set(over) <= {n for _, n in sp}, over


def test_the_tick_table_has_rows_where_a_float_restatement_leaves_other_bytes():
    """The byte comparison of osrl_step_begin_peer_w with osrl_step_tick_peer can only see a restatement that rounds
    differently on some row: a single-precision root does on the ``froot`` rows, a single-precision power at t = 2, 3, 4."""
    root = power = 0
    for tag, kw in OC.TICK_ROWS:
        t = max(kw["own"], kw.get("peer") or 0) + 1
        b1, b2 = (np.float32(b) for b in kw.get("betas", (0.9, 0.999)))
        bc1, bc2s, _ = OO.tick_words(t, b1, b2, 0)
        with np.errstate(under="ignore"):
            bc2 = 1.0 - float(np.power(np.float64(b2), np.float64(t)))
            root += int(np.sqrt(np.float32(bc2)) != np.float32(bc2s))
            power += int(np.float32(1.0) - np.power(b1, np.float32(t)) != np.float32(bc1))
    assert root >= 5 and power >= 3, (root, power)


def test_tick_words_are_the_formula():
    assert OO.tick_words(1, 0.9, 0.999, 0) == (1.0 - float(np.float32(0.9)), math.sqrt(1.0 - float(np.float32(0.999))), 1.0)
    assert OO.tick_words(2 ** 31 + 1, 0.9, 0.999, 3) == (1.0, 1.0, 1.0)
    assert OO.tick_words(2, 0.0, 0.0, 500)[2] == 2.0 / 500.0
