"""The row, loss and tail entry points of csrc/cdt.hip and csrc/cdt_grad.hip, one launch per case of
tests/cdt_kernel_cases.py, against the fp64 restatements of tests/cdt_kernel_oracle.py (gates: that module's docstring):
osrl_cdt_loss (both modes, the one-workgroup and the ``ws`` + finish form on either side of 1024 tokens, ``counts`` /
``world``, planted ``l0 == l1`` and ``costs == 0.5``, an all-padded batch, T = 1), osrl_cdt_mask_counts,
osrl_cdt_timestep_scatter, osrl_clip_grad_scale, osrl_cdt_temperature_step, the LayerNorm pairs with their dropout forms
(every kernel family, rows with |mean| >> std, constant rows, an outlier, eps-dominated rows, NULL operands,
``n_parts`` > M), GELU (the negative tail, |x| up to 40, +-0, denormals, the second grid-stride pass), osrl_cdt_embed_ln
(every token layout; the generic and the LDS-staged kernel), osrl_cdt_embed_input_grad and the three attention families
(scaled logits, one valid key, fully padded samples, S == rep, B * H = 1, probability dropout with the exported mask).

As in tests/test_gpu_loss_kernels.py every output buffer is filled with NaN before the launch and carries a 64-element
guard tail: the launch must write every word the oracle defines, leave alone every word it marks untouched, and nothing
past the end; a refused call returns -1 and writes nothing.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import cdt_kernel_cases as KC
import cdt_kernel_oracle as KO

pytestmark = pytest.mark.gpu
GUARD = 64


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _same(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _state(x):
    from osrl_amd.engine.core import StepState
    st = StepState(_dev(), ["s"])
    for _ in range(x.get("step", 1)):
        st.tick()
    return st


def _buf(init, off):
    """A device buffer holding ``init`` whose first element sits ``off`` floats past a 16-byte aligned address."""
    t = torch.from_numpy(np.concatenate([np.zeros(off, np.float32), init])).to(_dev())
    return t, t.data_ptr() + 4 * off


def launch(entry, x, shapes, st, over=None, expect=0):
    """One launch of osrl_<entry> on the inputs ``x``; ``shapes``: name -> shape of every buffer the launch writes (NaN
    filled unless ``x`` holds a starting value).  Returns name -> (array, initial array); workspaces of ``x['_scratch']``
    come back under their names as well.  Guard tails are checked, and (``expect`` != 0) that a refused call wrote nothing."""
    from osrl_amd import _lib as L
    from osrl_amd.engine.core import cur_stream
    p = dict(x, **(over or {}))
    null = p.pop("NULL", None)
    scratch, offs, nan_words = x.get("_scratch", {}), x.get("_offset", {}), x.get("_must_be_nan", {})
    args, outs, keep = [], {}, []
    for kind, name in KC.spec(entry):
        if name == null:
            args.append(None)
        elif kind == "p":
            v = p.get(name)
            if name in shapes or name in scratch:
                n = int(np.prod(shapes[name])) if name in shapes else int(scratch[name])
                init = np.full(n + GUARD, np.nan, np.float32)
                if name in scratch:
                    init[:n] = 0.0
                if v is not None:
                    init[:n] = np.asarray(v, np.float32).ravel()
                for w in nan_words.get(name, ()):
                    init[w] = 0.0
                t, ptr = _buf(init, offs.get(name, 0))
                outs[name] = (t, offs.get(name, 0), n, init, shapes.get(name, (n,)))
                args.append(ptr)
            elif v is None:
                args.append(None)
            else:
                t, ptr = _buf(np.ascontiguousarray(v, np.float32).ravel(), offs.get(name, 0))
                keep.append(t)
                args.append(ptr)
        elif kind == "q":
            t = torch.from_numpy(np.ascontiguousarray(p[name], np.int64)).to(_dev())
            keep.append(t)
            args.append(t.data_ptr())
        elif kind == "st":
            args.append(st.ptr)
        elif kind == "dr":
            if p.get("p") is None:
                args.append(None)
            else:
                d = L.DropoutT(float(p["p"]), int(p.get("site", 1)), int(p.get("seed", 1)), st.ptr)
                keep.append(d)
                args.append(C.byref(d))
        else:
            args.append(float(p[name]) if kind == "f" else int(p[name]))
    rc = getattr(L.load(), "osrl_" + entry)(*args, cur_stream())
    torch.cuda.synchronize()
    assert rc == expect, (entry, over, rc)
    got = {}
    for name, (t, off, n, init, shape) in outs.items():
        a = t.cpu().numpy()[off:]
        assert np.isnan(a[n:]).all(), f"{entry}: {name} written past its end"
        if expect != 0:
            assert _same(a, init), f"{entry}: refused call wrote {name}"
        got[name] = (a[:n].reshape(shape), init[:n].reshape(shape))
    return got


def export_keep(x, st):
    """The keep multiplier of the case's dropout site: osrl_dropout on ones at the same (seed, site, step)."""
    from osrl_amd import _lib as L
    from osrl_amd.engine.core import cur_stream
    n = x["_keep_n"]
    ones, raw = torch.ones(n, device=_dev()), torch.empty(n, device=_dev())
    d = L.DropoutT(float(x["p"]), int(x["site"]), int(x["seed"]), st.ptr)
    L.check(L.load().osrl_dropout(ones.data_ptr(), raw.data_ptr(), n, C.byref(d), cur_stream()), "osrl_dropout")
    k = raw.cpu().numpy()
    assert set(np.unique(k)) <= {0.0, np.float32(1.0 / (1.0 - np.float32(x["p"])))} and 0.05 < (k == 0).mean() < 0.5
    if "S" in x:
        B, H, S = x["B"], x["H"], x["S"]
        return np.ascontiguousarray(k.reshape(B, H, S, -1)[..., :S])
    return k.reshape(x["M"], x["E"])


def _out_shapes(r64):
    alias = r64.aux.get("alias", {})
    return {alias.get(k, k): v.shape for k, v in r64.out.items()}


def _verdict(tag, got, r64, r32):
    """Untouched words stay untouched, words that must be NaN are, everything else is within its gate."""
    alias = r64.aux.get("alias", {})
    views = {k: alias.get(k, k) for k in r64.out}
    for buf in set(views.values()):
        a, init = got[buf]
        skip = np.all([np.isnan(r64.out[k]) for k, b in views.items() if b == buf], 0)
        for w in r64.aux.get("must_be_nan", {}).get(buf, ()):
            assert np.isnan(a.ravel()[w]) and not np.isnan(init.ravel()[w]), f"{tag}: {buf}[{w}] must be NaN"
            skip.ravel()[w] = False
        assert _same(a[skip], init[skip]), f"{tag}: {buf} written where the launch must leave it alone"
    worst, where = KO.compare({k: got[b][0] for k, b in views.items()}, r64, r32)
    print(f"{tag}: worst |got - fp64| / gate = {worst:.3g} at {where}")
    assert worst <= 1.0, (tag, where, worst)


def check(c):
    x = KC.inputs(c)
    st = _state(x)
    if "_keep_n" in x:
        x["keep"] = export_keep(x, st)
    r64, r32 = KO.reference(c.kernel, x)
    x["_must_be_nan"] = r64.aux.get("must_be_nan", {})
    if c.kernel == "attention":
        got = run_attention(x, st)
    else:
        got = launch(c.kernel, x, _out_shapes(r64), st)
    _verdict(c.id, got, r64, r32)
    return x, got, r64


def run_attention(x, st):
    B, S, E, H = x["B"], x["S"], x["E"], x["H"]
    if x["family"] != "tiled":
        got = launch("attention_fwd", x, {"o": (B, S, E)}, st)
        got.update(launch("attention_bwd", x, {"dqkv": (B, S, 3 * E)}, st))
        return got
    n = B * H * S
    fw = launch("attention_fwd_ws", dict(x, _scratch={"lse": n}), {"o": (B, S, E)}, st)
    bw = launch("attention_bwd_ws", dict(x, o=fw["o"][0], lse=fw["lse"][0], _scratch={"ws": n}), {"dqkv": (B, S, 3 * E)}, st)
    return {"o": fw["o"], "dqkv": bw["dqkv"]}


def _cases(*kernels):
    return [c for c in KC.CASES if c.kernel in kernels]


@pytest.mark.parametrize("c", [c for c in _cases("cdt_loss") if not c.dp], ids=lambda c: c.id)
def test_cdt_loss_kernel(c):
    x, got, r64 = check(c)
    if not (x["mask"] > 0).any():  # the documented departure: nll = ent = 0 where the reference's empty mean is NaN
        stat = got["stat"][0]
        assert np.isnan(stat[6]) and stat[0] == 0 and stat[1] == 0 and not got["dhead"][0].any()


@pytest.mark.parametrize("c", _cases("cdt_mask_counts", "cdt_timestep_scatter", "clip_grad_scale", "cdt_temperature_step"),
                         ids=lambda c: c.id)
def test_counts_scatter_clip_and_temperature_kernels(c):
    check(c)


@pytest.mark.parametrize("c", _cases("layernorm_fwd", "layernorm_fwd_drop"), ids=lambda c: c.id)
def test_layernorm_forward_kernels(c):
    check(c)


@pytest.mark.parametrize("c", _cases("layernorm_bwd", "layernorm_bwd_drop"), ids=lambda c: c.id)
def test_layernorm_backward_kernels(c):
    x, got, r64 = check(c)
    E, go, bo = x["E"], x["g_off"], x["b_off"]
    parts = got["partial_ws"][0].astype(np.float64).reshape(x["n_parts"], 2 * E).sum(0)  # the partial rows add up to the same
    gate = r64.gate["slab"]
    for lo, sl in ((go, slice(0, E)), (bo, slice(E, 2 * E))):
        ratio = np.abs(parts[sl] - r64.out["slab"][lo:lo + E]) / np.maximum(gate[lo:lo + E], 1e-45)
        assert ratio.max() <= 1.0, (c.id, "partial_ws", float(ratio.max()))


@pytest.mark.parametrize("c", _cases("gelu_fwd", "gelu_bwd"), ids=lambda c: c.id)
def test_gelu_kernels(c):
    check(c)


@pytest.mark.parametrize("c", _cases("cdt_embed_ln", "cdt_embed_input_grad"), ids=lambda c: c.id)
def test_embedding_kernels(c):
    check(c)


@pytest.mark.parametrize("c", _cases("attention"), ids=lambda c: c.id)
def test_attention_kernels(c):
    x, got, _ = check(c)
    for b in range(x["B"]):
        if not (x["mask"][b] > 0).any():  # a fully padded sample: zero rows, zero gradient
            assert not got["o"][0][b].any() and not got["dqkv"][0][b].any(), (c.id, b)


def test_every_table_kernel_is_launched():
    assert {c.kernel for c in KC.CASES} == set(KC.TABLE_KERNELS)


@pytest.mark.parametrize("c", [c for c in KC.CASES if c.dp], ids=lambda c: c.id)
def test_two_ranks_reproduce_the_full_batch(c):
    """A 6-sequence, 1026-token batch as two ranks of 3 sequences (``world`` counts equal-sized ranks) with the all-reduced
    osrl_cdt_mask_counts as ``counts``: every rank's per-token gradients are the full-batch reference's, the summed
    statistics add up to the full-batch reference's, the replicated words (ent_reg, train_lr) are its share on each."""
    x = KC.inputs(c)
    st = _state(x)
    r64, r32 = KO.reference("cdt_loss", x)
    counts = np.zeros(2, np.float32)
    for b0 in (0, 3):
        m = x["mask"][b0 * x["T"]:(b0 + 3) * x["T"]]
        counts = counts + launch("cdt_mask_counts", dict(mask=m, BT=m.size), {"out": (2,)}, st)["out"][0]
    merged = {}
    for b0 in (0, 3):
        y = KC.loss_split(x, b0, 3, 2, counts)
        shapes = {k: ((s[0] // 2,) + s[1:] if k in ("dhead", "dlogits", "dsp") else s) for k, s in _out_shapes(r64).items()}
        got = {k: a.astype(np.float64) for k, (a, _) in launch("cdt_loss", y, shapes, st).items()}
        for k, a in got.items():
            if k in ("dhead", "dlogits", "dsp"):
                merged[k] = a if k not in merged else np.concatenate([merged[k], a], 0)
            else:
                merged[k] = a if k not in merged else merged[k] + a  # shares of 1 / world add up as the sums do
    alias = r64.aux["alias"]
    worst, where = KO.compare({k: merged[alias.get(k, k)] for k in r64.out}, r64, r32)
    print(f"{c.id} as two ranks: worst |got - fp64| / gate = {worst:.3g} at {where}")
    assert worst <= 1.0, (c.id, where, worst)


def _refusal_base(entry):
    if entry.startswith("attention"):
        fam = "tiled" if entry.endswith("_ws") else "reg"
        return next(c for c in _cases("attention") if KC.inputs(c)["family"] == fam and KC.inputs(c)["S"] in (17, 129))
    if entry == "cdt_embed_ln":
        return next(c for c in _cases(entry) if c.tag.startswith("rew1-cost1-pre1"))
    if entry == "cdt_embed_input_grad":
        return next(c for c in _cases(entry) if c.tag.startswith("rew1-cost1-pre1") and "no_" not in c.tag)
    return _cases(entry)[0]


@pytest.mark.parametrize("entry", sorted(KC.REFUSALS))
def test_argument_errors_are_refused_before_any_launch(entry):
    c = _refusal_base(entry)
    x = KC.inputs(c)
    st = _state(x)
    r64 = KO.reference(c.kernel, x)[0]
    shapes = _out_shapes(r64)
    if c.kernel == "attention":
        B, S, E, H = x["B"], x["S"], x["E"], x["H"]
        shapes = {"o": (B, S, E)} if "fwd" in entry else {"dqkv": (B, S, 3 * E)}
        if entry == "attention_fwd_ws":
            x["_scratch"] = {"lse": B * H * S}
        if entry == "attention_bwd_ws":
            x.update(o=np.zeros((B, S, E), np.float32), lse=np.zeros(B * H * S, np.float32), _scratch={"ws": B * H * S})
    for over in KC.REFUSALS[entry]:
        launch(entry, x, shapes, st, over=dict(over), expect=-1)
