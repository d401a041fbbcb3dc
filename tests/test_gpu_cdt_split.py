"""The CDT train step with matmul="bf16x3" (projections and their input gradients on osrl_linear_split): the project's
parity bound against the goldens and the oracle, graph capture, freshness of the bf16 planes behind every path that
changes the weights, checkpoints across the two modes, and the untouched default."""
import dataclasses

import numpy as np
import pytest
import torch

from cases import CDT_CASES, CDTCase, make_cdt_batch
from oracle_util import load_golden
from test_gpu_cdt import C5_SLICE, DEV, build_cdt_gpu, t

pytestmark = pytest.mark.gpu

# cases with a layer the split kernel takes (N % 128 == 0 and K % 32 == 0 need embedding_dim % 128 == 0)
RUNS_SPLIT = {"cdt_mid", "cdt_c5_slice"}
# a C5-shaped model whose step is deterministic to the bit: no timestep embedding (its gradient scatter adds with fp32
# atomics, the one order-dependent sum of the step -- tests/test_gpu_cdt.py compares graph and eager to 1e-6 for that reason)
DET = CDTCase("cdt_split_det", od=11, ad=3, B=16, T=10, E=128, heads=8, layers=2, episode_len=200, steps=4, warmup=500,
              dropout=0.1, seed=21, time_emb=False, head_layers=2)


def batch(c):
    return {k: t(v) for k, v in make_cdt_batch(c).items()}


def step(tr, b, n=1):
    for _ in range(n):
        tr.train_one_step(b["states"], b["actions"], b["returns"], b["costs_return"], b["time_steps"], b["mask"],
                          b["episode_cost"], b["costs"])


def check_plan(name, m, c, tr):
    """The plan the engine reports, GEMM by GEMM: osrl_linear_split exactly where the kernel takes the shape (K % 32 == 0
    and N % 128 == 0), osrl_linear everywhere else.  The E = 128 / 256 cases run every block projection on the split
    kernel; the E = 16 cases have no such layer and are asserted to FALL BACK as a whole (they then check that the mode
    leaves the f32 path intact); cdt_v_prefix_det (E = 32) runs mlp.0 and the dX of mlp.2 on it."""
    e, g = m.engine(c.B, tr.cfg), m.groups["cdt"]
    assert e.plan.matmul == "bf16x3"
    n = dict(osrl_linear_split=[0, 0], osrl_linear=[0, 0])
    for key, dx, rows, resid in e._gemms():
        N, K = g.layout[key][1]
        if dx:
            K, N = N, K
        want = "osrl_linear_split" if (K % 32 == 0 and N % 128 == 0) else "osrl_linear"
        assert e.linear_kernel(key, dx) == want, (key, dx, K, N)
        assert (key in (g.pt_off if dx else g.pw_off)) == (want == "osrl_linear_split")
        n[want][int(dx)] += 1
    assert (e.plan.split_fwd, e.plan.split_dx) == tuple(n["osrl_linear_split"]), e.plan
    assert (e.plan.f32_fwd, e.plan.f32_dx) == tuple(n["osrl_linear"]), e.plan
    assert e.plan.split_fwd + e.plan.f32_fwd == 4 * c.layers + len(e.head_hidden) + 3
    if name in RUNS_SPLIT:
        assert e.plan.split_fwd >= 4 * c.layers and e.plan.split_dx >= 4 * c.layers, e.plan
        assert g.planes_w is not None and g.planes_t is not None
    elif c.E == 16:  # FALLBACK: nothing fits the kernel's tiles -- the whole step runs osrl_linear under the plan, no planes
        assert e.plan.split_fwd == 0 and e.plan.split_dx == 0, e.plan
        assert g.planes_w is None
    else:
        assert name == "cdt_v_prefix_det" and (e.plan.split_fwd, e.plan.split_dx) == (c.layers, c.layers), e.plan
    return e


@pytest.mark.parametrize("name", [n for n, c in CDT_CASES.items() if c.dropout == 0])
def test_cdt_split_train_step_matches_golden_and_oracle(name):
    """tests/test_gpu_cdt.py::test_cdt_train_step_matches_golden_and_oracle with matmul="bf16x3": the same statistics
    (1e-5 at step 0, 1e-4 after) and parameter (2e-5) comparisons against the goldens and the oracle."""
    from test_oracle_cdt_golden import build_cdt_oracle
    c = CDT_CASES[name]
    g = load_golden(name)
    keys = [str(k) for k in g["stat_keys"]]
    m, tr, lg = build_cdt_gpu(c, matmul="bf16x3")
    o = build_cdt_oracle(c)
    b, bn = batch(c), make_cdt_batch(c)
    for s in range(c.steps):
        step(tr, b)
        if s == 0:
            check_plan(name, m, c, tr)
        ost = o.train_one_step(bn["states"], bn["actions"], bn["returns"], bn["costs_return"], bn["time_steps"],
                               bn["mask"], bn["episode_cost"], bn["costs"])
        ref = dict(zip(keys, g["stats"][s]))
        tol = 1e-5 if s == 0 else 1e-4
        for k in keys:
            got = lg.last("train/" + k)
            for nm, r in (("golden", ref[k]), ("oracle", ost[k])):
                assert abs(got - r) <= tol * max(1.0, abs(r)), f"{name} step {s} {k}: gpu {got} vs {nm} {r}"
        if f"s{s + 1}/log_temperature" in g:
            assert abs(m.log_temperature.item() - float(g[f"s{s + 1}/log_temperature"])) < 1e-6
        sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
        for k, v in sd.items():
            if f"p{s + 1}/{k}" in g:
                d = np.abs(v - g[f"p{s + 1}/{k}"]).max()
                assert d <= 2e-5, f"{name} step {s + 1} param {k}: max diff {d:.3e}"
            elif f"p{s + 1}/smp/{k}" in g:
                d = np.abs(v.reshape(-1)[::97] - g[f"p{s + 1}/smp/{k}"]).max()
                assert d <= 2e-5, f"{name} step {s + 1} param sample {k}: {d:.3e}"
    ap, cp, sp = m(b["states"], b["actions"], b["returns"], b["costs_return"], b["time_steps"],
                   ~b["mask"].to(torch.bool), b["episode_cost"])
    a = (ap.mean if c.stochastic else ap).cpu().numpy()
    assert np.abs(a - g["act"]).max() <= 1e-4


@pytest.mark.parametrize("case,use_graph", [("cdt_drop", False), ("cdt_drop", True), ("cdt_c5_slice", False),
                                            ("cdt_v_prefix", False), ("cdt_v_prefix", True)])
def test_cdt_split_dropout_train_step_matches_oracle(case, use_graph):
    """The dropout and prefix variants (tests/test_gpu_cdt.py::test_cdt_dropout_train_step_matches_oracle) with
    matmul="bf16x3"; the C5-shaped slice (E = 256, 5120 token rows) runs every block projection on the split kernel."""
    from test_oracle_cdt_golden import build_cdt_oracle
    c = C5_SLICE if case == "cdt_c5_slice" else CDT_CASES[case]
    m, tr, lg = build_cdt_gpu(c, use_graph=use_graph, seed=1234, matmul="bf16x3")
    o = build_cdt_oracle(c)
    bn = make_cdt_batch(c)
    b = {k: t(v) for k, v in bn.items()}
    for s in range(c.steps):
        step(tr, b)
        if s == 0:
            e = check_plan(case, m, c, tr)
            assert (e.graph is not None) == use_graph
        masks = {k: v.cpu().numpy() for k, v in m.engine(c.B).dropout_masks().items()}
        ost = o.train_one_step(bn["states"], bn["actions"], bn["returns"], bn["costs_return"], bn["time_steps"],
                               bn["mask"], bn["episode_cost"], bn["costs"], drop=masks)
        for k, r in ost.items():
            got = lg.last("train/" + k)
            assert abs(got - r) <= 1e-4 * max(1.0, abs(r)), f"step {s} {k}: gpu {got} vs oracle {r}"
        assert abs(m.log_temperature.item() - o.log_temperature) < 1e-6
        for k, v in m.state_dict().items():
            if v.dtype != torch.bool:
                d = np.abs(v.cpu().numpy() - o.p[k]).max()
                assert d <= 2e-5, f"step {s + 1} param {k}: max diff {d:.3e}"


def _state(m):
    g = m.groups["cdt"]
    return g.p.clone(), g.m.clone(), g.v.clone()


def test_cdt_split_graph_replay_is_bit_equal_to_eager():
    """Four steps: the replayed graph leaves the same bits as eager launches -- parameters and both Adam moments.  A
    graph whose planes were not refreshed behind the captured AdamW step would run every step on the planes of capture
    time and part from the eager run at step 2."""
    c, b = DET, batch(DET)
    res = []
    for use_graph in (False, True):
        m, tr, _ = build_cdt_gpu(c, stats_mode="none", use_graph=use_graph, seed=5, matmul="bf16x3")
        step(tr, b, 4)
        torch.cuda.synchronize()
        e = m._engine
        assert (e.graph is not None) == use_graph and e.plan.split_fwd >= 4 * c.layers + 1
        res.append(_state(m))
        # the planes are those of the CURRENT parameters
        g = m.groups["cdt"]
        have = (g.planes_w.clone(), g.planes_t.clone())
        g.refresh_planes()
        torch.cuda.synchronize()
        assert torch.equal(have[0], g.planes_w) and torch.equal(have[1], g.planes_t)
    for x, y, nm in zip(res[0], res[1], "pmv"):
        assert torch.equal(x, y), nm
    # and the mode is not a no-op: the f32 step gives other bits
    m, tr, _ = build_cdt_gpu(c, stats_mode="none", use_graph=False, seed=5)
    step(tr, b, 4)
    assert not torch.equal(_state(m)[0], res[0][0])
    assert (_state(m)[0] - res[0][0]).abs().max() < 2e-5


@pytest.mark.parametrize("use_graph", [False, True])
def test_cdt_split_planes_follow_load_state_dict(use_graph):
    """Train k steps, load other weights, step once == a fresh model built with those weights stepping once (the Adam
    moments and the step count are made equal: the only thing under test is which weights the GEMMs read)."""
    c, b = DET, batch(DET)
    other = dataclasses.replace(c, seed=22)
    m_a, tr_a, _ = build_cdt_gpu(c, stats_mode="none", use_graph=use_graph, seed=5, matmul="bf16x3")
    step(tr_a, b, 3)
    m_b, tr_b, _ = build_cdt_gpu(other, stats_mode="none", use_graph=use_graph, seed=5, matmul="bf16x3")
    m_b.engine(c.B, tr_b.cfg)
    sd = {k: v.clone() for k, v in m_b.state_dict().items()}
    m_a.load_state_dict(sd)
    ga, gb = m_a.groups["cdt"], m_b.groups["cdt"]
    assert torch.equal(ga.planes_w, gb.planes_w) and torch.equal(ga.planes_t, gb.planes_t)
    # same optimizer state and step count on both sides
    gb.m.copy_(ga.m), gb.v.copy_(ga.v)
    ea, eb = m_a._engine, m_b._engine
    eb.st.state.copy_(ea.st.state), eb.st.ring.copy_(ea.st.ring)
    eb.st.host_step = ea.st.host_step
    eb.temp_mv.copy_(ea.temp_mv), m_b.log_temperature.copy_(m_a.log_temperature)
    step(tr_a, b)
    step(tr_b, b)
    torch.cuda.synchronize()
    for x, y, nm in zip(_state(m_a), _state(m_b), "pmv"):
        assert torch.equal(x, y), nm
    # repack() after an in-place edit of a parameter refreshes the planes too
    with torch.no_grad():
        ga.view("cdt.blocks.0.mlp.0.weight").mul_(1.5)
    before = ga.planes_w.clone()
    m_a.repack()
    torch.cuda.synchronize()
    assert not torch.equal(before, ga.planes_w)


def test_cdt_split_checkpoint_resume_is_bit_identical_and_crosses_modes(tmp_path):
    from osrl_amd.common.checkpoint import load_checkpoint, save_checkpoint
    c, b = DET, batch(DET)
    kw = dict(stats_mode="none", seed=5)
    m_a, tr_a, _ = build_cdt_gpu(c, matmul="bf16x3", **kw)
    step(tr_a, b, 5)
    m_b, tr_b, _ = build_cdt_gpu(c, matmul="bf16x3", **kw)
    step(tr_b, b, 3)
    path = str(tmp_path / "split.pt")
    save_checkpoint(m_b, path)
    m_c, tr_c, _ = build_cdt_gpu(dataclasses.replace(c, seed=23), matmul="bf16x3", **kw)
    step(tr_c, b, 1)  # (its planes exist and hold OTHER weights when the checkpoint arrives)
    load_checkpoint(m_c, path)
    step(tr_c, b, 2)
    torch.cuda.synchronize()
    for x, y, nm in zip(_state(m_a), _state(m_c), "pmv"):
        assert torch.equal(x, y), nm
    assert torch.equal(m_a.log_temperature, m_c.log_temperature)
    # the checkpoint holds no planes: the same keys as one written by the default mode
    m_f, tr_f, _ = build_cdt_gpu(c, **kw)
    step(tr_f, b, 3)
    path_f = str(tmp_path / "f32.pt")
    save_checkpoint(m_f, path_f)
    ck_s, ck_f = torch.load(path, weights_only=False), torch.load(path_f, weights_only=False)
    assert set(ck_s) == set(ck_f) and set(ck_s["model_state"]) == set(ck_f["model_state"])
    # written under "f32", resumed under "bf16x3" -- and the other way round: both continue next to the f32 run
    step(tr_f, b, 2)
    want = _state(m_f)[0]
    for src, mode in ((path_f, "bf16x3"), (path, "f32")):
        m_x, tr_x, _ = build_cdt_gpu(dataclasses.replace(c, seed=24), **(dict(kw, matmul=mode)))
        load_checkpoint(m_x, src)
        step(tr_x, b, 2)
        torch.cuda.synchronize()
        assert m_x._engine.plan.matmul == mode
        got = _state(m_x)[0]
        assert torch.isfinite(got).all() and (got - want).abs().max() < 2e-5, mode
        if mode == "bf16x3":  # the planes it stepped on were those of the checkpoint's weights, not of seed 24
            g = m_x.groups["cdt"]
            have = g.planes_w.clone()
            g.refresh_planes()
            assert torch.equal(have, g.planes_w)


def test_default_mode_is_f32_and_allocates_no_planes():
    c = CDT_CASES["cdt_mid"]
    m, tr, _ = build_cdt_gpu(c)
    step(tr, batch(c))
    e, g = m._engine, m.groups["cdt"]
    assert tr.cfg["matmul"] == "f32" and e.plan.matmul == "f32"
    assert e.plan.split_fwd == 0 and e.plan.split_dx == 0
    assert g.planes_w is None and g.planes_t is None and not g.pw_off and not g.pt_off
    assert all(e.linear_kernel(k) == "osrl_linear" for k in g.weights)
    # the engine dict of model.engine(batch, cfg) takes the same key; inference engines stay f32 under either
    m2, tr2, _ = build_cdt_gpu(c)
    e2 = m2.engine(c.B, dict(tr2.cfg, matmul="bf16x3"))
    assert e2.plan.matmul == "bf16x3" and e2.plan.split_fwd > 0
    b = batch(c)
    m2(b["states"], b["actions"], b["returns"], b["costs_return"], b["time_steps"], ~b["mask"].to(torch.bool),
       b["episode_cost"])
    assert m2._infer.plan.matmul == "f32" and m2._infer.plan.split_fwd == 0
    with pytest.raises(ValueError):
        m2.engine(c.B, dict(tr2.cfg, matmul="nope"))
