"""GPU parity of the wide MLP path (include/osrl_amd.h: nets with a layer 449..1024 wide run one launch per layer):
kernel level against fp64 numpy (random seeded shapes mixing wide and narrow layers, every row map, src1, all three
activations, out_scale != 1, dX slices, NULL dZ / h pointers, every tail against its standalone glue call), and whole
train steps of the five MLP algorithms at reference-sized widths against the numpy oracle, eager / graph-replayed /
pipelined / data-parallel, with checkpoints, evaluate() and act()."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from cases import Case
from gpu_util import build_gpu, gpu_batch, gpu_step
from oracle_util import build_oracle, oracle_step

pytestmark = pytest.mark.gpu

GROUP_GATE, KINK_FLOOR = 2e-5, 1e-7  # == tests/test_gpu_train_step.py


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _act64(name, x):
    return {"relu": lambda v: np.maximum(v, 0), "tanh": np.tanh, "id": lambda v: v}[name](x)


def _dact64(name, y):
    return {"relu": lambda v: (v > 0).astype(np.float64), "tanh": lambda v: 1 - v * v,
            "id": lambda v: np.ones_like(v)}[name](y)


WIDE = [449, 464, 500, 512, 640, 750, 800, 1000, 1024]


def _wide_cases(n, seed=4096):
    """(E, dims, acts, out_scale, rows, (d0, map0, div0), dx) with at least one layer > 448 wide."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        L_ = int(rs.randint(1, 5))
        widths = [int(rs.choice(WIDE)) if rs.rand() < 0.6 else int(rs.choice([1, 2, 17, 64, 256, 448])) for _ in range(L_)]
        k0 = int(rs.choice([3, 33, 78, 130, 512, 1000]))
        dims = [k0] + widths
        if max(dims) <= 448:
            dims[1 + int(rs.randint(0, L_))] = int(rs.choice(WIDE))
        acts = [["relu", "tanh", "id"][int(rs.randint(0, 3))] for _ in range(L_)]
        E = int(rs.choice([1, 2, 3, 4, 8]))
        rows = int(rs.choice([1, 17, 256, 2048, 20480]))
        if E * rows * max(dims) > 40_000_000:  # keep the fp64 reference affordable
            rows = int(rs.choice([1, 17, 256]))
        d0 = int(rs.randint(1, k0 + 1))
        mode = int(rs.randint(0, 3))
        div0 = {0: 1, 1: int(rs.randint(1, rows + 1)), 2: int(rs.randint(1, 12))}[mode]
        dxc = None
        if rs.rand() < 0.6:
            c0 = int(rs.randint(0, k0))
            dxc = (c0, int(rs.randint(1, k0 - c0 + 1)))
        out.append((E, dims, acts, float(rs.choice([1.0, 0.5, 2.0])), rows, (d0, mode, div0), dxc))
    return out


MLP_CASES = [
    (1, [78, 1024, 1024, 1], ["relu", "relu", "id"], 1.0, 2048, (76, 0, 1), (76, 2)),     # CPQ critic [1024, 1024]
    (2, [78, 512, 512, 1], ["relu", "relu", "id"], 1.0, 20480, (76, 1, 2048), None),      # N*B rows, MOD map
    (1, [78, 750, 750, 8], ["relu", "relu", "id"], 1.0, 2048, (76, 0, 1), (76, 2)),       # VAE encoder 750
    (1, [80, 800, 800, 2], ["relu", "relu", "tanh"], 1.5, 2048, (76, 0, 1), (76, 4)),     # VAE decoder 800, tanh * scale
    (4, [41, 512, 512, 1], ["relu", "relu", "id"], 1.0, 333, (33, 2, 3), (33, 8)),        # DIV map, 4 nets
    (1, [20, 640, 48, 1024, 6], ["relu", "tanh", "relu", "tanh"], 2.0, 130, (16, 0, 1), (3, 11)),  # 4 layers mixed
    (8, [12, 1024, 1], ["relu", "id"], 1.0, 50, (8, 0, 1), (8, 4)),                       # 8 nets
    (1, [1024, 1024], ["id"], 1.0, 17, (1000, 0, 1), (0, 1024)),                          # one layer, 1024 in and out
] + _wide_cases(16)


def _build(E, dims, acts, oscale, rs, dev):
    from osrl_amd.engine.core import FlatGroup, LayerRef, NetDesc
    grp = FlatGroup("t", dev)
    for e in range(E):
        for l in range(len(dims) - 1):
            grp.add(f"{e}.{l}.w", (dims[l + 1], dims[l]))
            grp.mark_weight(f"{e}.{l}.w")
            grp.add(f"{e}.{l}.b", (dims[l + 1],))
    grp.finalize()
    nets, refs = [], []
    for e in range(E):
        layers, rr = [], []
        for l in range(len(dims) - 1):
            k = 1 / math.sqrt(dims[l])
            W, b = grp.view(f"{e}.{l}.w"), grp.view(f"{e}.{l}.b")
            W.copy_(torch.tensor(rs.uniform(-k, k, W.shape), dtype=torch.float32))
            b.copy_(torch.tensor(rs.uniform(-k, k, b.shape), dtype=torch.float32))
            layers.append((W, b))
            rr.append(LayerRef(W, b, grp, f"{e}.{l}.w", f"{e}.{l}.b"))
        nets.append(layers)
        refs.append(rr)
    grp.repack()
    return grp, nets, NetDesc(refs, acts, oscale)


@pytest.mark.parametrize("ci", range(len(MLP_CASES)))
def test_wide_mlp_fwd_bwd_against_fp64(ci):
    from osrl_amd import _lib as L
    from osrl_amd.engine.core import DwPlan, MlpRun, cur_stream
    E, dims, acts, oscale, rows, (d0, map0, div0), dxc = MLP_CASES[ci]
    dev = _dev()
    rs = np.random.RandomState(40 + ci)
    grp, nets, desc = _build(E, dims, acts, oscale, rs, dev)
    assert desc.wide
    d1 = dims[0] - d0
    n0 = {0: rows, 1: div0, 2: (rows + div0 - 1) // div0}[map0]
    src0 = torch.tensor(rs.randn(n0, d0), dtype=torch.float32, device=dev)
    src1 = torch.tensor(rs.randn(rows, d1), dtype=torch.float32, device=dev) if d1 else None
    run = MlpRun(desc, rows, True, dev)
    y = run.forward(src0, src1, map0=map0, div0=div0)
    # a forward-only use of the same net: the same launches, the same bits
    run_ns = MlpRun(desc, rows, False, dev)
    y_ns = run_ns.forward(src0, src1, map0=map0, div0=div0)
    torch.cuda.synchronize()
    assert torch.equal(y, y_ns)

    idx0 = {0: np.arange(rows), 1: np.arange(rows) % div0, 2: np.arange(rows) // div0}[map0]
    X = src0.cpu().numpy().astype(np.float64)[idx0]
    if d1:
        X = np.concatenate([X, src1.cpu().numpy().astype(np.float64)], 1)
    np.testing.assert_array_equal(run.x.cpu().numpy(), X, err_msg="saved input x")
    caches = []
    for e in range(E):
        h, c = X, [X]
        for l, a in enumerate(acts):
            W, b = (t.cpu().numpy().astype(np.float64) for t in nets[e][l])
            h = _act64(a, h @ W.T + b)
            if l == len(acts) - 1:
                h = h * oscale
            got = run.h[e][l].cpu().numpy()
            err = np.abs(got - h).max()
            assert err < 3e-5 * max(1.0, np.abs(h).max()), f"case {ci} fwd net {e} layer {l}: max err {err}"
            h = got.astype(np.float64)  # (continue from the GPU's activations: no ReLU mask flips near 0)
            c.append(h)
        caches.append(c)

    dy = torch.tensor(rs.randn(E, rows, dims[-1]), dtype=torch.float32, device=dev)
    run.setup_backward(dy, need_dz=True, dx_cols=dxc)
    run.backward_dz()
    plan = DwPlan(grp, run.dw_entries(), rows, dev)
    plan.launch()
    torch.cuda.synchronize()
    for e in range(E):
        c = caches[e]
        g = dy[e].cpu().numpy().astype(np.float64)
        L_ = len(acts)
        for l in range(L_ - 1, -1, -1):
            yl = c[l + 1] / (oscale if l == L_ - 1 else 1.0)
            dz = g * _dact64(acts[l], yl) * (oscale if l == L_ - 1 else 1.0)
            got = run.dz[e][l].cpu().numpy()
            assert np.abs(got - dz).max() < 5e-5 * max(1.0, np.abs(dz).max()), f"case {ci} dz net {e} layer {l}"
            W = nets[e][l][0].cpu().numpy().astype(np.float64)
            dW, db = dz.T @ c[l], dz.sum(0)
            gW = grp.grad_view(f"{e}.{l}.w").cpu().numpy()
            gb = grp.grad_view(f"{e}.{l}.b").cpu().numpy()
            assert np.abs(gW - dW).max() < 1e-4 * max(1.0, np.abs(dW).max()), f"case {ci} dW net {e} layer {l}"
            assert np.abs(gb - db).max() < 1e-4 * max(1.0, np.abs(db).max()), f"case {ci} db net {e} layer {l}"
            g = dz @ W
        if dxc is not None:
            c0, nc = dxc
            ref = g[:, c0:c0 + nc]
            assert np.abs(run.dx[e].cpu().numpy() - ref).max() < 5e-5 * max(1.0, np.abs(ref).max()), f"case {ci} dx {e}"
    # the dW tile kernels at these widths: 80 x 80 and 64 x 64 tiles give the same gradients
    ref_w = {k: grp.grad_view(k).cpu().numpy().astype(np.float64) for k in grp.layout}
    for T in (5, 4):
        plan_t = DwPlan(grp, run.dw_entries(), rows, dev, tile_blocks=T)
        plan_t.launch()
        torch.cuda.synchronize()
        for k, ref in ref_w.items():
            got = grp.grad_view(k).cpu().numpy()
            assert np.abs(got - ref).max() < 2e-5 * max(1.0, np.abs(ref).max()), f"case {ci} tiles {T}: {k}"

    # NULL dZ pointers: dz[e][0] skipped (no dX) -> the upper dZ are the same bits, dz[e][0] is not written
    if len(acts) >= 2:
        g2 = L.GradsT.from_buffer_copy(run.grads_c)
        keep = [[run.dz[e][l].clone() for l in range(len(acts))] for e in range(E)]
        for e in range(E):
            run.dz[e][0].fill_(7.0)
            g2.dz[e][0] = None
            for l in range(1, len(acts)):
                run.dz[e][l].zero_()
            g2.dx[e] = None
        L.check(L.load().osrl_mlp_backward_dz(C.byref(run.bwd_net.c), rows, C.byref(run.saved_c), C.byref(g2), cur_stream()),
                "osrl_mlp_backward_dz")
        torch.cuda.synchronize()
        for e in range(E):
            assert bool((run.dz[e][0] == 7.0).all()), "a NULL dz was written"
            for l in range(1, len(acts)):
                assert torch.equal(run.dz[e][l], keep[e][l]), (e, l)
        # a missing dZ that a lower step reads is refused (OSRL_E_UNSUPPORTED), nothing launched
        g3 = L.GradsT.from_buffer_copy(run.grads_c)
        g3.dz[0][len(acts) - 1] = None
        rc = L.load().osrl_mlp_backward_dz(C.byref(run.bwd_net.c), rows, C.byref(run.saved_c), C.byref(g3), cur_stream())
        assert rc == L.E_UNSUPPORTED
    # a missing intermediate activation in the forward is refused the same way
    if len(acts) >= 2:
        a2 = L.ActsT.from_buffer_copy(run.acts_c)
        a2.h[0][0] = None
        r = run._rows(src0, src1, map0, div0)
        rc = L.load().osrl_mlp_forward(C.byref(desc.c), C.byref(r), C.byref(a2), cur_stream())
        assert rc == L.E_UNSUPPORTED


def _lib():
    from osrl_amd import _lib as L
    return L, L.load()


@pytest.mark.parametrize("dims", [[78, 1024, 1024, 4], [33, 750, 750, 16], [5, 512, 8]])
def test_wide_forward_tails_equal_their_glue_calls(dims):
    """Every forward tail behind the wide path's layer launches == the plain forward + the named standalone call."""
    from osrl_amd.engine.core import MlpRun, cur_stream
    L, lib = _lib()
    dev = _dev()
    rs = np.random.RandomState(7)
    acts = ["relu"] * (len(dims) - 2) + ["id"]
    grp, nets, desc = _build(1, dims, acts, 1.0, rs, dev)
    rows, Lz = 300, dims[-1] // 2
    x = torch.tensor(rs.randn(rows, dims[0]), dtype=torch.float32, device=dev)
    eps = torch.tensor(rs.randn(rows, Lz), dtype=torch.float32, device=dev)
    eps2 = torch.tensor(rs.randn(rows, Lz), dtype=torch.float32, device=dev)
    eps_ood = torch.tensor(rs.randn(3, rows, Lz), dtype=torch.float32, device=dev)
    plain = MlpRun(desc, rows, False, dev)
    head = plain.forward(x)[0]
    f = dict(dtype=torch.float32, device=dev)
    st = cur_stream()
    # VAE_LATENT
    ref = torch.empty(rows, Lz, **f)
    L.check(lib.osrl_vae_latent(head.data_ptr(), eps.data_ptr(), rows, Lz, ref.data_ptr(), st), "osrl_vae_latent")
    out = torch.empty(rows, Lz, **f)
    t = L.TailT()
    t.kind, t.L, t.eps, t.out = L.TAIL_VAE_LATENT, Lz, eps.data_ptr(), out.data_ptr()
    run = MlpRun(desc, rows, False, dev)
    run.forward(x, tail=t)
    torch.cuda.synchronize()
    assert torch.equal(run.y, plain.y) and torch.equal(out, ref)
    # VAE_KL
    ref = torch.empty(rows, **f)
    L.check(lib.osrl_vae_kl_rows(head.data_ptr(), rows, Lz, ref.data_ptr(), st), "osrl_vae_kl_rows")
    out = torch.empty(rows, **f)
    t = L.TailT()
    t.kind, t.L, t.out = L.TAIL_VAE_KL, Lz, out.data_ptr()
    MlpRun(desc, rows, False, dev).forward(x, tail=t)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    # GAUSS: two draws (the second with its tanh) and the OOD draws
    r1, r2, rt, ro = (torch.empty(rows, Lz, **f), torch.empty(rows, Lz, **f), torch.empty(rows, Lz, **f),
                      torch.empty(3, rows, Lz, **f))
    L.check(lib.osrl_gauss_head(head.data_ptr(), eps.data_ptr(), rows, Lz, C.c_float(1.5), r1.data_ptr(), None, None, st), "g1")
    L.check(lib.osrl_gauss_head(head.data_ptr(), eps2.data_ptr(), rows, Lz, C.c_float(1.5), r2.data_ptr(), rt.data_ptr(),
                                None, st), "g2")
    L.check(lib.osrl_gauss_ood_sample(head.data_ptr(), eps_ood.data_ptr(), 3, rows, Lz, ro.data_ptr(), st), "ood")
    o1, o2, ot, oo = (torch.empty_like(r1), torch.empty_like(r2), torch.empty_like(rt), torch.empty_like(ro))
    t = L.TailT()
    t.kind, t.L, t.max_action = L.TAIL_GAUSS, Lz, 1.5
    t.eps, t.out, t.eps2, t.out2, t.tanh2 = eps.data_ptr(), o1.data_ptr(), eps2.data_ptr(), o2.data_ptr(), ot.data_ptr()
    t.eps_ood, t.out_ood, t.n_samples = eps_ood.data_ptr(), oo.data_ptr(), 3
    MlpRun(desc, rows, False, dev).forward(x, tail=t)
    torch.cuda.synchronize()
    for a, b in ((o1, r1), (o2, r2), (ot, rt), (oo, ro)):
        assert torch.equal(a, b)


def test_wide_backward_tail_equals_its_glue_call():
    """VAE_LATENT_BWD behind the wide path's dX launch == the plain backward + osrl_vae_latent_bwd."""
    from osrl_amd.engine.core import MlpRun, cur_stream
    L, lib = _lib()
    dev = _dev()
    rs = np.random.RandomState(8)
    od, ad, Lz, H, rows = 76, 2, 4, 800, 700
    grp, nets, desc = _build(1, [od + Lz, H, H, ad], ["relu", "relu", "tanh"], 1.0, rs, dev)
    obs = torch.tensor(rs.randn(rows, od), dtype=torch.float32, device=dev)
    z = torch.tensor(rs.randn(rows, Lz), dtype=torch.float32, device=dev)
    head = torch.tensor(rs.randn(rows, 2 * Lz), dtype=torch.float32, device=dev)
    eps = torch.tensor(rs.randn(rows, Lz), dtype=torch.float32, device=dev)
    dy = torch.tensor(rs.randn(1, rows, ad), dtype=torch.float32, device=dev)
    outs = []
    for fused in (False, True):
        run = MlpRun(desc, rows, True, dev)
        run.forward(obs, z)
        run.setup_backward(dy, dx_cols=(od, Lz))
        out = torch.empty(rows, 2 * Lz, dtype=torch.float32, device=dev)
        if fused:
            t = L.TailT()
            t.kind, t.L, t.eps, t.head, t.out, t.beta, t.rows_global = (L.TAIL_VAE_LATENT_BWD, Lz, eps.data_ptr(),
                                                                        head.data_ptr(), out.data_ptr(), 0.5, 0)
            run.backward_dz(tail=t)
        else:
            run.backward_dz()
            L.check(lib.osrl_vae_latent_bwd(head.data_ptr(), eps.data_ptr(), run.dx[0].data_ptr(), rows, Lz, C.c_float(0.5),
                                            0, out.data_ptr(), cur_stream()), "osrl_vae_latent_bwd")
        torch.cuda.synchronize()
        outs.append((run.dx.clone(), out))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_wide_regress_step_is_refused_and_forward2_is_two_launches():
    from osrl_amd.engine.core import MlpRun
    L, lib = _lib()
    dev = _dev()
    rs = np.random.RandomState(9)
    _, _, da = _build(2, [78, 512, 512, 1], ["relu", "relu", "id"], 1.0, rs, dev)
    _, _, db = _build(1, [76, 1000, 4], ["relu", "id"], 1.0, rs, dev)
    s = L.MlpStepT()
    s.net = da.c
    dummy = torch.zeros(4096, device=dev)  # (never read: the shape is refused before any launch)
    ftypes = dict(L.MlpStepT._fields_)
    for f in ("st", "target", "entries", "work", "p", "m", "v", "ws"):
        t = ftypes[f]
        setattr(s, f, dummy.data_ptr() if t is C.c_void_p else C.cast(dummy.data_ptr(), t))
    assert lib.osrl_mlp_regress_step(C.byref(s), None) == L.E_UNSUPPORTED
    x = torch.tensor(rs.randn(99, 76), dtype=torch.float32, device=dev)
    a = torch.tensor(rs.randn(99, 2), dtype=torch.float32, device=dev)
    r0, r1 = MlpRun(da, 99, False, dev), MlpRun(db, 99, False, dev)
    y0, y1 = r0.forward_with((x, a), r1, (x,))
    p0, p1 = MlpRun(da, 99, False, dev).forward(x, a), MlpRun(db, 99, False, dev).forward(x)
    torch.cuda.synchronize()
    assert torch.equal(y0, p0) and torch.equal(y1, p1)


# ---- whole train steps -----------------------------------------------------------------------------------------------
STEP_CASES = {
    "cpq_512_750": dict(algo="cpq", od=33, ad=4, B=256, hidden=[512, 512], vae_hidden=750, N=10, steps=1, seed=61),
    "cpq_1024_800_c2": dict(algo="cpq", od=76, ad=2, B=2048, hidden=[1024, 1024], vae_hidden=800, N=10, steps=1, seed=62),
    "bcql_512_750": dict(algo="bcql", od=33, ad=8, B=256, hidden=[512, 512], vae_hidden=750, N=10, steps=1, seed=63),
    "bearl_640_512": dict(algo="bearl", od=17, ad=6, B=128, hidden=[640, 640], vae_hidden=512, N=5, steps=1, seed=64,
                          hp=dict(mmd_sigma=20.0)),
    "coptidice_1024": dict(algo="coptidice", od=33, ad=8, B=256, hidden=[1024, 1024], steps=1, seed=65),
    "bc_1024x3": dict(algo="bc", od=17, ad=6, B=256, hidden=[1024, 1024, 1024], steps=1, seed=66),
}


def _case(name):
    return Case(name, episode_len=1000, **STEP_CASES[name])


def _opts(o):
    return {k: v for k, v in vars(o).items() if k.startswith("opt") and hasattr(v, "m") and isinstance(v.m, dict)}


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_wide_train_step_matches_the_oracle(name):
    """One train step at reference-sized widths == the numpy oracle (fp32 / fp64, the closer one): statistics <= 1e-5, the
    gradients (Adam first moments) at GROUP_GATE of each tensor's scale or the KINK_FLOOR, with the KinkBook bound for
    ReLU units within 2 ulp of their kink (tests/test_gpu_train_step.py::test_random_shape_tuples_match_the_oracle)."""
    from oracle.osrl_oracle import MLP, KinkBook
    c = _case(name)
    m, tr, lg = build_gpu(c)
    o32, o64 = build_oracle(c, np.float32), build_oracle(c, np.float64)
    b = gpu_batch(c)
    gpu_step(tr, c, b, 0)
    book = KinkBook(ulps=2.0)
    s32 = oracle_step(o32, c, 0)
    MLP.kink = book
    try:
        s64 = oracle_step(o64, c, 0)
    finally:
        MLP.kink = None
    for k in s64:
        got = lg.last(k)
        d = min(abs(got - s64[k]), abs(got - s32[k]))
        assert d <= 1e-5 * max(1.0, abs(s64[k])), f"{name} {k}: gpu {got} vs oracle {s64[k]} / {s32[k]}"
    groups = list(m.groups.values()) if hasattr(m, "groups") else []
    n_checked = 0
    for oname, opt in _opts(o64).items():
        opt32 = getattr(o32, oname)
        for k, mo in opt.m.items():
            grp = next(g for g in groups if k in g.layout)
            mg = grp._view(grp.m, k).cpu().numpy()
            scale = max(np.abs(mo).max(), 1e-12)
            el = np.minimum(np.abs(mg - mo), np.abs(mg - opt32.m[k]))
            strict = max(GROUP_GATE * scale, KINK_FLOOR)
            allow = (1.0 - 0.9) * np.asarray(book.allow.get(k, 0.0)) * 1.01
            over = el - (strict + allow)
            assert over.max() <= 0, f"{name} Adam first moment {k}: max diff {el.max():.3e} vs scale {scale:.3e}"
            n_checked += 1
    assert n_checked > 0
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    for k, v in o64.p.items():
        d = min(np.abs(sd[k] - v).max(), np.abs(sd[k] - o32.p[k]).max())
        assert d <= 2.5e-3 and np.median(np.abs(sd[k] - v)) <= 2e-6, f"{name} param {k}: {d:.3e}"


def test_wide_plans_take_only_forms_that_exist():
    """The chooser's rows for a wide CPQ shape: the forms built on the fused tile kernels are off, the engine runs."""
    c = _case("cpq_1024_800_c2")
    m, tr, lg = build_gpu(c)
    eng = m.engine(c.B)
    assert not eng.plan.vae_ns and not eng.plan.ood_rows and not eng.plan.ood_share and eng.vae_ns is None
    assert eng.pre_cost == 0 and eng.pre_enc == 0


def _state(m):
    out = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for name, g in m.groups.items():
        out["m/" + name], out["v/" + name] = g.m.clone(), g.v.clone()
    if isinstance(getattr(m, "log_alpha", None), torch.Tensor):
        out["log_alpha"] = m.log_alpha.clone()
    return out


WIDE_CPQ = Case("cpq_wide_graph", "cpq", od=33, ad=4, B=1024, hidden=[512, 512], vae_hidden=750, N=5, steps=1,
                episode_len=1000, seed=70)


def test_wide_graph_replay_equals_the_eager_step():
    b = gpu_batch(WIDE_CPQ)
    res = []
    for use_graph in (False, True):
        m, tr, lg = build_gpu(WIDE_CPQ, use_graph=use_graph)
        for s in range(3):
            gpu_step(tr, WIDE_CPQ, b, s, with_noise=False)
        torch.cuda.synchronize()
        if use_graph:
            assert m._engine.graph is not None
        res.append(_state(m))
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k


def test_wide_pipelined_graph_equals_one_step_replays():
    """engine.steps_replay with several steps per graph (B >= 1024) == the same steps as one-step graph replays, bit for
    bit (tests/test_gpu_pipeline.py at a wide shape)."""
    from osrl_amd.common.replay import ReplayStore, synthetic_transitions
    c = WIDE_CPQ
    res = []
    for spg in (0, 4):
        m, tr, lg = build_gpu(c, stats_mode="none", use_graph=True)
        eng = m.engine(c.B)
        store = ReplayStore(synthetic_transitions(4096, c.od, c.ad, seed=7, max_action=c.max_action), torch.device("cuda:0"),
                            reward_scale=0.1, cost_scale=1.0, seed=3)
        eng.attach_replay(store)
        if spg:
            eng.steps_replay(8, steps_per_graph=spg)
        else:
            for _ in range(8):
                eng.step_replay(True)
        torch.cuda.synchronize()
        assert eng.st.device_step() == 8
        res.append(_state(m))
        del m, tr, eng
        torch.cuda.empty_cache()
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k


def test_wide_data_parallel_world1_equals_single(nccl_world1):
    from osrl_amd.engine.dist import DataParallel
    c = Case("cpq_wide_dp", "cpq", od=33, ad=4, B=256, hidden=[512, 512], vae_hidden=750, N=5, steps=1, episode_len=1000,
             seed=71)
    assert nccl_world1.is_initialized()
    b = gpu_batch(c)
    res = []
    for use_dp in (False, True):
        m, tr, lg = build_gpu(c)
        if use_dp:
            dp = DataParallel()
            m.engine(c.B, rows_global=c.B * dp.world, dist=dp)
            dp.broadcast_model(m)
        for s in range(2):
            gpu_step(tr, c, b, s)
        torch.cuda.synchronize()
        res.append({k: v.clone() for k, v in m.state_dict().items()})
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k


@pytest.mark.parametrize("name", ["cpq_512_750", "bc_1024x3", "coptidice_1024"])
def test_wide_checkpoint_resume_is_bit_identical(name, tmp_path):
    from osrl_amd.common.checkpoint import load_checkpoint, save_checkpoint
    from cases import make_params
    c = _case(name)
    b = gpu_batch(c)
    m_a, tr_a, _ = build_gpu(c)
    for s in range(3):
        gpu_step(tr_a, c, b, s, with_noise=False)
    m_b, tr_b, _ = build_gpu(c)
    gpu_step(tr_b, c, b, 0, with_noise=False)
    path = str(tmp_path / "model.pt")
    save_checkpoint(m_b, path)
    m_c, tr_c, _ = build_gpu(c)
    load_checkpoint(m_c, path)
    for s in range(1, 3):
        gpu_step(tr_c, c, b, s, with_noise=False)
    torch.cuda.synchronize()
    sa, sc = _state(m_a), _state(m_c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    # the reference's state_dict layout at these widths: the same keys and shapes as the reference-shaped parameters
    ref = make_params(c)
    sd = m_c.state_dict()
    assert set(sd) == set(ref)
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k


def test_wide_evaluate_and_act_match_a_numpy_policy():
    """Batched actor forward (the evaluate() path) and the B = 1 / B = 4 act() GEMV kernel at width 1024 == fp64 numpy."""
    c = Case("bc_act", "bc", od=17, ad=6, B=64, hidden=[1024, 1024, 1024], steps=1, episode_len=1000, seed=72)
    m, tr, lg = build_gpu(c)
    sd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    obs = np.random.RandomState(3).randn(64, c.od)

    def np_policy(x):
        h = x
        n = len(c.hidden) + 1
        for l in range(n):
            h = h @ sd[f"actor.pi.{2 * l}.weight"].T + sd[f"actor.pi.{2 * l}.bias"]
            h = np.maximum(h, 0) if l < n - 1 else np.tanh(h) * c.max_action
        return h

    ref = np_policy(obs)
    with torch.no_grad():
        got = m.actor(torch.tensor(obs, dtype=torch.float32, device="cuda:0")).cpu().numpy()
    assert np.abs(got - ref).max() < 3e-5
    got1 = np.stack([np.asarray(m.act(obs[i].astype(np.float32))).reshape(-1) for i in range(4)])
    gotn = m.fast_policy().act(obs[:4].astype(np.float32))[0]
    assert np.abs(got1 - ref[:4]).max() < 3e-5 and np.abs(gotn - ref[:4]).max() < 3e-5
