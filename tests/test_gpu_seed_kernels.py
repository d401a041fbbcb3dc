"""The seeded backward launch (``osrl_mlp_backward_dz_seed``: the launch computes dL/d(output) itself, ``seed_dy`` in
csrc/mlp.hip, and reduces the logged statistic through per-tile partials and a last-arriver sum) against the fp64
references of tests/seed_oracle.py on the case table of tests/seed_cases.py: every kind of the header's enum on every
kernel instantiation a seed can run in (16 / 32 / 64-row tiles, 4 and 8 waves, 1 / 2 / 4 / 7 column blocks, the wide
path's one-layer sub-net), ragged row counts, more partials than the last workgroup has lanes, and the planted edges
(argmin ties, ``min qc == thres`` and one ulp beside it, done rows, clamp edges, log-variances far outside their bounds,
ensembles of 1 / 3 / 4 members with one more member in the table than the seed is told about).

A tiny net is built and run forward on random inputs; the case's outputs are then planted as the saved outputs the seed
stage reads (the lower activations stay the real forward's), the seed is built with the functions the engines use
(``osrl_amd.engine.glue.seed_*``, ``SeedStat``), and one backward launch runs.  Every buffer the seed reads and every
buffer the launch writes lies inside a NaN-filled allocation with a 64-float guard on both sides.  Asserted per case:

* dZ of the output layer against fp64 (``loss_oracle.compare``: routing exact, "arith" 8 ulp of scale, "trans" by the
  oracle's fp32-against-fp64 rule), the output activation composed in fp64;
* the chain below (dZ of the lower layers, the dX slice) against fp64 propagation from the GPU's own dZ of the output
  layer and saved activations, with the tolerances of ``test_mlp_fwd_bwd``;
* the statistic(s) against the oracle (gate: ``seed_oracle.SEED_STAT_GATE``), the same bits from a second launch on the
  same ``SeedStat`` (the counter re-arms), and, where the case asks, dZ unchanged with the statistic switched off;
* the header's promise: on identity-output nets dZ of the output layer has the bits of the named loss kernel, launched
  on the same inputs;
* the guards are still NaN.

Worst |GPU - fp64| / gate per kind on an MI355X (this table, 136 cases): see DESIGN.md.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import loss_oracle as LO
import seed_cases as SC
import seed_oracle as SO
import test_gpu_loss_kernels as TL

pytestmark = pytest.mark.gpu
GUARD = 64
_INT_NAN = 0x7FC00000  # the guard word of the int32 counter


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Guarded:
    """``data`` inside a NaN-filled allocation with a GUARD-word guard on both sides."""

    def __init__(self, data, dev, pool, dtype=np.float32):
        data = np.ascontiguousarray(data, dtype)
        n = data.size
        fill = np.nan if dtype == np.float32 else _INT_NAN
        host = np.full(n + 2 * GUARD, fill, dtype)
        host[GUARD:GUARD + n] = data.ravel()
        self.buf = torch.from_numpy(host).to(dev)
        self.t = self.buf[GUARD:GUARD + n].view(data.shape)
        self.n, self.fill, self.is_float = n, fill, dtype == np.float32
        pool.append(self)

    def intact(self):
        a = self.buf.cpu().numpy()
        g = np.concatenate([a[:GUARD], a[GUARD + self.n:]])
        return bool(np.isnan(g).all()) if self.is_float else bool((g == self.fill).all())


def nan_out(shape, dev, pool):
    return Guarded(np.full(shape, np.nan, np.float32), dev, pool)


class Rig:
    """A net [dims] x E on ``rows`` rows after its forward, outputs planted, backward buffers guarded."""

    def __init__(self, dims, E, rows, tile_rows, act, out_scale, y, seed=0):
        from osrl_amd.engine.core import FlatGroup, LayerRef, MlpRun, NetDesc
        self.dev = dev = _dev()
        self.pool = []
        self.dims, self.E, self.rows = dims, E, rows
        self.acts = ["relu"] * (len(dims) - 2) + [act]
        rs = np.random.RandomState(77 + seed)
        grp = FlatGroup("t", dev)
        for e in range(E):
            for l in range(len(dims) - 1):
                grp.add(f"{e}.{l}.w", (dims[l + 1], dims[l]))
                grp.mark_weight(f"{e}.{l}.w")
                grp.add(f"{e}.{l}.b", (dims[l + 1],))
        grp.finalize()
        refs, self.W = [], []
        for e in range(E):
            rr, ww = [], []
            for l in range(len(dims) - 1):
                k = 1 / math.sqrt(dims[l])
                W, b = grp.view(f"{e}.{l}.w"), grp.view(f"{e}.{l}.b")
                W.copy_(torch.tensor(rs.uniform(-k, k, W.shape), dtype=torch.float32))
                b.copy_(torch.tensor(rs.uniform(-k, k, b.shape), dtype=torch.float32))
                rr.append(LayerRef(W, b, grp, f"{e}.{l}.w", f"{e}.{l}.b"))
                ww.append(W.cpu().numpy().astype(np.float64))
            refs.append(rr)
            self.W.append(ww)
        grp.repack()
        self.grp = grp
        desc = NetDesc(refs, self.acts, out_scale)
        if tile_rows:
            desc.c.tile_rows = tile_rows
        self.run = run = MlpRun(desc, rows, True, dev)
        run.forward(torch.tensor(rs.randn(rows, dims[0]), dtype=torch.float32, device=dev))
        torch.cuda.synchronize()
        # plant the outputs: run.y[e] is saved.h[e][L-1]; the launch reads them from a guarded copy
        self.y = Guarded(y, dev, self.pool)
        run.y.copy_(self.y.t)
        self.dx_cols = (1, dims[0] - 2)
        self.dx = nan_out((E, rows, self.dx_cols[1]), dev, self.pool)
        run.setup_backward(torch.zeros(E, 1, 1, device=dev), need_dz=True, dx_cols=self.dx_cols, dx_out=self.dx.t)
        nl = len(dims) - 1
        self.dz = [[nan_out((rows, dims[l + 1]), dev, self.pool) for l in range(nl)] for _ in range(E)]
        for e in range(E):
            run.grads_c.dy[e] = None  # a seeded launch ignores dy
            run.saved_c.h[e][nl - 1] = self.y.t[e].data_ptr()
            for l in range(nl):
                run.grads_c.dz[e][l] = self.dz[e][l].t.data_ptr()
                run.dz[e][l] = self.dz[e][l].t

    def put(self, a, dtype=np.float32):
        return None if a is None else Guarded(a, self.dev, self.pool, dtype).t

    def seed_stat(self):
        """The engines' ``SeedStat`` with its scratch moved into guarded allocations of the same size."""
        from osrl_amd.engine import glue as G
        ws = G.SeedStat(self.dev, self.E, self.rows)
        ws.partials = self.put(np.zeros(ws.partials.numel(), np.float32))
        ws.counter = self.put(np.zeros(1, np.int32), np.int32)
        return ws

    def launch(self, seed, expect=0):
        from osrl_amd import _lib as L
        from osrl_amd.engine.core import cur_stream
        r = self.run
        rc = L.load().osrl_mlp_backward_dz_seed(C.byref(r.bwd_net.c), self.rows, C.byref(r.saved_c), C.byref(r.grads_c),
                                                None, C.byref(seed), cur_stream())
        torch.cuda.synchronize()
        assert rc == expect, rc
        for g in self.pool:
            assert g.intact(), "a guard word was overwritten"

    def dz_np(self, l):
        return np.stack([self.dz[e][l].t.cpu().numpy() for e in range(self.E)])

    def reset_outputs(self):
        for row in self.dz:
            for g in row:
                g.t.fill_(float("nan"))
        self.dx.t.fill_(float("nan"))

    def check_chain(self, tag):
        """dz[l] (l < L-1) and the dX slice against fp64 propagation from the GPU's own dz[L-1] and saved activations."""
        nl = len(self.dims) - 1
        for e in range(self.E):
            g = self.dz[e][nl - 1].t.cpu().numpy().astype(np.float64)
            for l in range(nl - 1, 0, -1):
                g = g @ self.W[e][l]
                h = self.run.h[e][l - 1].cpu().numpy().astype(np.float64)
                ref = g * (h > 0)
                got = self.dz[e][l - 1].t.cpu().numpy()
                assert np.isfinite(got).all(), (tag, e, l - 1)
                err = np.abs(got - ref).max()
                assert err < 3e-5 * max(1.0, np.abs(ref).max()), (tag, "dz", e, l - 1, err)
                g = got.astype(np.float64)
            c0, nc = self.dx_cols
            ref = (g @ self.W[e][0])[:, c0:c0 + nc]
            got = self.dx.t[e].cpu().numpy()
            assert np.isfinite(got).all(), (tag, "dx", e)
            assert np.abs(got - ref).max() < 3e-5 * max(1.0, np.abs(ref).max()), (tag, "dx", e)


def build_seed(rig: Rig, kind, x, ws, stat, stat2=None):
    """The seed of one case, through the engines' builders where one exists; (seed, loss kernel, its inputs, its
    output's name and shape) -- the last four None where no loss kernel computes the same thing."""
    from osrl_amd import _lib as L
    from osrl_amd.engine import glue as G
    E, rows, NL = x["y"].shape
    p = rig.put
    yt = rig.y.t
    loss = None
    if kind == "MSE" and x.get("head") is not None:
        s = G.seed_vae(p(x["act"]), p(x["head"]), rows, NL, x["L"], x["beta"], x["rows_global"], ws, stat)
        if E == 1:
            loss = ("vae_loss", dict(x, u=x["y"][0]), "du", (rows, NL))
    elif kind == "MSE":
        ng = x.get("n_global", 0)
        s = G._seed(L.SEED_MSE, rows, 0, ws, stat)
        t = p(x["target"])
        s.x0 = t.data_ptr()
        s.scale = s.stat_scale = float(np.float32(1.0) / np.float32(ng if ng > 0 else rows * NL))
        s._keep += [t]
        if E == 1:
            loss = ("mse_loss", dict(u=x["y"][0].ravel(), target=x["target"].ravel(), n=rows * NL, n_global=ng), "du",
                    (rows, NL))
    elif kind == "CPQ_CRITIC":
        n_a, n_b = x["n_q_old"], x["n_qc_old"]
        s = G.seed_cpq_critic(p(x["q_old"]), n_a, p(x["qc_old"]), n_b, p(x["rew"]), p(x["done"]), rows, x["gamma"],
                              x["q_thres"], x["rows_global"], ws, stat)
        loss = ("cpq_critic_loss", dict(x, q_old=x["q_old"][:n_a], qc_old=x["qc_old"][:n_b], q=x["y"][..., 0], n_q=E), "dq",
                (E, rows))
    elif kind == "CPQ_COST":
        n = x["n_qc_old"]
        s = G.seed_cpq_cost(p(x["qc_old_next"]), n, p(x["cost"]), rows, x["gamma"], x["rows_global"], ws, stat)
        loss = ("cpq_cost_loss", dict(x, qc_old_next=x["qc_old_next"][:n], qc=x["y"][..., 0], n_qc=E), "dq", (E, rows))
    elif kind == "CPQ_ACTOR":
        s = G.seed_cpq_actor(yt, E, p(x["qc"]), x["n_qc"], rows, x["q_thres"], x["rows_global"], ws, stat)
        loss = ("cpq_actor_loss", dict(x, q=x["y"][..., 0], qc=x["qc"][:x["n_qc"]], n_q=E), "dq", (E, rows))
    elif kind == "GAUSS_HEAD":
        n = x["n_nets"]
        s = G.seed_gauss_head(p(x["eps"]), p(x["tanh_u"]), p(x["da_nets"]), n, rows, x["max_action"])
        loss = ("gauss_head_bwd", dict(x, head=x["y"][0], da_nets=x["da_nets"][:n]), "dhead", (rows, NL))
    elif kind == "BCQ_CRITIC":
        s = G.seed_bcq_critic(p(x["q_t"]), x["n1"], x["n2"], x["n_samples"], p(x["base"]), p(x.get("done")), rows,
                              x["gamma"], x["lmbda"], x["rows_global"], ws, stat)
        loss = ("bcq_critic_loss", dict(x, q_on=x["y"][..., 0], n_on=E), "dq", (E, rows))
    elif kind == "FQE":
        s = G.seed_fqe(p(x["q_t"]), x["n_r"], x["n_c"], p(x["rew"]), p(x["cost"]), p(x["done"]), rows, x["gamma"], ws,
                       stat, stat2)
    elif kind == "GAUSS_NLL":
        s = G._seed(L.SEED_GAUSS_NLL, rows, 0, ws, stat)
        t = p(x["target"])
        s.x0 = t.data_ptr()
        s.scale = s.stat_scale = float(np.float32(1.0) / np.float32(rows * ((NL + 1) // 2)))
        s.gamma, s.thres = float(x["lo"]), float(x["hi"])
        s._keep += [t]
    else:
        raise KeyError(kind)
    return s, loss


def _rig(c, x):
    dims, E, rows = SC.shape(c, x)
    return Rig(dims, E, rows, c.tile_rows, x["_act"], x["_out_scale"], x["y"])


WORST = {}  # kind -> ((worst / gate, where), (the statistics' worst / gate, case)): printed per case, copied into DESIGN.md


@pytest.mark.parametrize("c", SC.CASES, ids=lambda c: c.id)
def test_seeded_backward_launch_against_fp64(c):
    x = SC.inputs(c)
    r64, r32 = SO.reference(c.kind, x)
    rig = _rig(c, x)
    has_stat = "stat" in r64.out
    ws = rig.seed_stat() if has_stat else None
    stat = nan_out((1,), rig.dev, rig.pool) if has_stat else None
    stat2 = nan_out((1,), rig.dev, rig.pool) if "stat2" in r64.out else None
    seed, loss = build_seed(rig, c.kind, x, ws, stat.t if stat else None, stat2.t if stat2 else None)
    rig.launch(seed)
    nl = len(rig.dims) - 1
    got = dict(dz=rig.dz_np(nl - 1))
    if has_stat:
        got["stat"] = stat.t.cpu().numpy().copy()
        assert int(ws.counter.item()) == 0, "the arrival counter was not re-armed"
    if stat2:
        got["stat2"] = stat2.t.cpu().numpy().copy()
    worst, where = LO.compare(got, r64, r32)
    kid = "MSE_KL" if (c.kind == "MSE" and x.get("head") is not None) else c.kind
    sworst = max([float(abs(float(got[n][0]) - float(r64.out[n][0])) / r64.gate[n][0]) for n in ("stat", "stat2")
                  if n in r64.out] or [0.0])
    WORST[kid] = tuple(max(a, b) for a, b in zip(WORST.get(kid, ((0.0, ""), (0.0, ""))),
                                                 ((worst, f"{c.id} {where}"), (sworst, c.id))))
    print(f"{c.id} [{x['_tile']}]: worst |got - fp64| / gate = {worst:.3g} at {where}, statistic {sworst:.3g}; {kid} so far "
          f"{WORST[kid][0][0]:.3g} / statistic {WORST[kid][1][0]:.3g} at {WORST[kid][1][1]}")
    assert worst <= 1.0, (c.id, where, worst)
    rig.check_chain(c.id)
    # the header's promise: the bits of the named loss kernel (identity-output nets)
    if loss is not None and x["_act"] == "id":
        kernel, xl, name, shp = loss
        ref = TL.launch(kernel, xl, {name: shp})[name][0]
        mine = got["dz"][..., 0] if name == "dq" else got["dz"][0]
        assert torch.equal(torch.from_numpy(np.ascontiguousarray(mine)), torch.from_numpy(np.ascontiguousarray(ref))), \
            (c.id, kernel, np.argwhere(mine.view(np.int32) != ref.view(np.int32))[:4].tolist())
    if has_stat:  # a second launch on the same SeedStat: the counter re-armed, the same bits
        keep = {k: v.copy() for k, v in got.items()}
        rig.reset_outputs()
        stat.t.fill_(float("nan"))
        if stat2:
            stat2.t.fill_(float("nan"))
        rig.launch(seed)
        assert np.array_equal(stat.t.cpu().numpy().view(np.int32), keep["stat"].view(np.int32)), c.id
        if stat2:
            assert np.array_equal(stat2.t.cpu().numpy().view(np.int32), keep["stat2"].view(np.int32)), c.id
        assert np.array_equal(rig.dz_np(nl - 1).view(np.int32), keep["dz"].view(np.int32)), c.id
        if c.nostat:
            # stat == NULL with the scratch given, then no scratch at all: dZ is still written, the statistic left alone
            for scratch in (True, False):
                rig.reset_outputs()
                stat.t.fill_(float("nan"))
                s2, _ = build_seed(rig, c.kind, x, ws if scratch else None, None, None)
                rig.launch(s2)
                assert np.isnan(stat.t.cpu().numpy()).all(), (c.id, "stat written", scratch)
                assert np.array_equal(rig.dz_np(nl - 1).view(np.int32), keep["dz"].view(np.int32)), (c.id, scratch)
                assert int(ws.counter.item()) == 0
                rig.check_chain(c.id)
            if stat2:  # FQE with stat2 == NULL: stat as before, stat2 left alone
                stat2.t.fill_(float("nan"))
                s3, _ = build_seed(rig, c.kind, x, ws, stat.t, None)
                rig.launch(s3)
                assert np.array_equal(stat.t.cpu().numpy().view(np.int32), keep["stat"].view(np.int32)), c.id
                assert np.isnan(stat2.t.cpu().numpy()).all(), c.id


# ---- refusals: every condition of the host check returns -1 before any launch and writes nothing ---------------------------
def _refusals():
    from osrl_amd import _lib as L

    def setf(**kw):
        def f(s, rig):
            for k, v in kw.items():
                setattr(s, k, v)
        return f

    def no_saved(s, rig):
        rig.run.saved_c.h[rig.E - 1][len(rig.dims) - 2] = None

    def no_counter(s, rig):
        s.counter = None

    def no_partials(s, rig):
        s.partials = None

    def with_partials(s, rig):
        ws = rig.seed_stat()
        s.partials, s.counter = ws.partials.data_ptr(), ws.counter.data_ptr()
        s._keep.append(ws)

    def kl_zero(s, rig):
        s.kl_L = 0

    def kind_nll(lo, hi):
        def f(s, rig):
            s.kind, s.gamma, s.thres = L.SEED_GAUSS_NLL, lo, hi
        return f

    out = []
    # (case to start from, output width the net is built with or None = the case's, what to break)
    for k in ("CPQ_CRITIC", "CPQ_ACTOR", "FQE"):
        for f in ("n_a", "n_b"):
            for v in (0, 5):
                out.append((k, None, f"{f}={v}", setf(**{f: v})))
    for v in (0, 5):
        out.append(("CPQ_COST", None, f"n_a={v}", setf(n_a=v)))
    for k in ("CPQ_CRITIC", "CPQ_COST", "CPQ_ACTOR", "BCQ_CRITIC", "FQE"):
        out.append((k, 2, "NL=2", None))
    for NL in (6, 3):
        out.append(("GAUSS_NLL", NL, f"NL={NL}", None))
    out.append(("GAUSS_HEAD", 5, "NL=5", None))
    out.append(("GAUSS_NLL", None, "lo==hi", kind_nll(0.5, 0.5)))
    out.append(("GAUSS_NLL", None, "lo>hi", kind_nll(0.5, -10.0)))
    out.append(("FQE", None, "n_a+n_b!=nets", setf(n_a=1, n_b=1)))
    out.append(("CPQ_CRITIC", None, "partials without counter", no_counter))
    out.append(("CPQ_CRITIC", None, "counter without partials", no_partials))
    out.append(("GAUSS_HEAD", None, "partials for GAUSS_HEAD", with_partials))
    out.append(("MSE_KL", None, "kl_head with kl_L=0", kl_zero))
    out.append(("CPQ_CRITIC", None, "no saved output", no_saved))
    out.append(("BCQ_CRITIC", None, "n_samples=0", setf(n_samples=0)))
    out.append(("CPQ_CRITIC", None, "kind=9", setf(kind=9)))
    return out


_BASE = {"MSE_KL": "MSE-kl-ad3-L6-r15", "CPQ_CRITIC": "CPQ_CRITIC-n34-r15", "CPQ_COST": "CPQ_COST-n4-r15",
         "CPQ_ACTOR": "CPQ_ACTOR-n34-r15", "GAUSS_HEAD": "GAUSS_HEAD-ad3-n4-r15", "BCQ_CRITIC": "BCQ_CRITIC-n25-s10-nodone-r15",
         "FQE": "FQE-n21-r15", "GAUSS_NLL": "GAUSS_NLL-od3-r15"}


@pytest.mark.parametrize("ri", range(32))
def test_the_host_check_refuses_and_writes_nothing(ri):
    table = _refusals()
    assert len(table) == 32
    kid, NL, what, brk = table[ri]
    c = SC.BY_ID[_BASE[kid]]
    x = SC.inputs(c)
    dims, E, rows = SC.shape(c, x)
    if NL is not None:  # the same seed on a net whose output width the kind does not take
        dims = dims[:-1] + [NL]
    y = np.zeros((E, rows, dims[-1]), np.float32)
    rig = Rig(dims, E, rows, 0, "id", 1.0, y)
    has_stat = kid != "GAUSS_HEAD"
    ws = rig.seed_stat() if has_stat else None
    stat = nan_out((1,), rig.dev, rig.pool)
    stat2 = nan_out((1,), rig.dev, rig.pool)
    seed, _ = build_seed(rig, c.kind, x, ws, stat.t if has_stat else None, stat2.t if kid == "FQE" else None)
    if brk is not None:
        brk(seed, rig)
    rig.launch(seed, expect=-1)
    for e in range(E):
        for g in rig.dz[e]:
            assert np.isnan(g.t.cpu().numpy()).all(), (what, "dz written")
    assert np.isnan(rig.dx.t.cpu().numpy()).all() and np.isnan(stat.t.cpu().numpy()).all(), what
    assert np.isnan(stat2.t.cpu().numpy()).all(), what
    if ws is not None:
        assert not ws.partials.any() and int(ws.counter.item()) == 0, (what, "scratch written")
