"""``CDT(..., differentiable=True)``: the CDT forward as an autograd node whose forward and backward run on the HIP
kernels of the fused train step (ops.cdt_apply, engine/cdt.py forward / backward) and whose input gradients come from
csrc/cdt_grad.hip.  Parameter and input gradients of a user loss against fp64 central differences of the pinned oracle
and torch autograd on CPU, the reference training loss against the fused step's own gradient, dropout, windows, modes,
stale graphs, and a user optimizer loop followed by the fused trainer, the act path and checkpoints."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from cases import CDT_CASES, CDTCase, make_cdt_batch, make_cdt_params
from test_gpu_cdt import build_cdt_gpu
from test_oracle_cdt_golden import build_cdt_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FEAT_DETACHED = ("cost_emb.weight", "cost_emb.bias", "timestep_emb.weight")  # also feed costs_emb.detach()


def t(x):
    return torch.as_tensor(x, device=DEV)


def _model(c, **kw):
    m, tr, lg = build_cdt_gpu(c, **kw)
    m.differentiable = True
    return m, tr, lg


def _inputs(bn, grad=()):
    b = {k: t(v) for k, v in bn.items()}
    for k in grad:
        b[k] = b[k].clone().requires_grad_(True)
    return b


def _call(m, b, Tin=None):
    sl = slice(None, Tin)
    return m(b["states"][:, sl], b["actions"][:, sl], b["returns"][:, sl], b["costs_return"][:, sl],
             b["time_steps"][:, sl], ~b["mask"][:, sl].to(torch.bool), b["episode_cost"])


def _weights(c, B, T, seed):
    rs = np.random.RandomState(seed)
    w = dict(lp=rs.randn(B, T, 2), sp=rs.randn(B, T, c.od))
    if c.stochastic:
        w.update(mu=rs.randn(B, T, c.ad), ls=rs.randn(B, T, c.ad))
    else:
        w.update(act=rs.randn(B, T, c.ad))
    return w


def _gpu_functional(c, out, w):
    ap, lp, sp = out
    f = lambda k, x: (t(w[k][:, :x.shape[1]]).float() * x).sum()  # noqa: E731
    heads = f("mu", ap.loc) + f("ls", ap.scale.log()) if c.stochastic else f("act", ap)
    return heads + f("lp", lp) + f("sp", sp)


def _oracle_functional(c, res, w):
    keys = ("mu", "ls") if c.stochastic else ("act",)
    tot = sum(float((w[k] * res[k]).sum()) for k in keys)
    return tot + float((w["lp"] * res["cost_logp"]).sum()) + float((w["sp"] * res["state_pred"]).sum())


def _fd_check(c, o, L, got, names, rs, h=1e-4, n_dir=4, gate=1e-5, label=""):
    """Central differences of the fp64 functional ``L()`` of the oracle along ``n_dir`` random directions per tensor of
    ``o.p`` named in ``names``; ``got`` = the GPU gradients.  Relative error of a directional derivative: against the
    larger of its own size and the size a random direction gives it (||g|| ||v|| / sqrt(n))."""
    worst = 0.0
    for k in names:
        g = np.asarray(got[k], np.float64)
        base = o.p[k].copy()
        for _ in range(n_dir):
            v = rs.randn(*base.shape)
            v /= np.linalg.norm(v)
            o.p[k] = base + h * v
            lp = L()
            o.p[k] = base - h * v
            lm = L()
            o.p[k] = base
            fd = (lp - lm) / (2 * h)
            gv = float((g * v).sum())
            scale = max(abs(fd), np.linalg.norm(g) / math.sqrt(g.size), 1e-12)
            rel = abs(gv - fd) / scale
            worst = max(worst, rel)
            assert rel <= gate, f"{label} {k}: <grad, v> {gv:.8e} vs central difference {fd:.8e} (rel {rel:.2e})"
    return worst


@pytest.mark.parametrize("name", list(CDT_CASES))
def test_parameter_gradients_match_fp64_central_differences(name):
    """A user loss (a random linear functional of mu / log_std or the action, the cost log-probabilities and the state
    predictions) + loss.backward() fills .grad of every parameter; each tensor's gradient matches fp64 central
    differences of the oracle's forward along 4 random directions.  (Without the feature this raises: the outputs
    carry no grad_fn.)"""
    c = CDT_CASES[name]
    m, _, _ = _model(c)
    m.eval()
    bn = make_cdt_batch(c)
    b = _inputs(bn)
    w = _weights(c, c.B, c.T, 1)
    loss = _gpu_functional(c, _call(m, b), w)
    loss.backward()
    got = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    assert all(p.grad is not None for p in m.parameters())
    o = build_cdt_oracle(c, np.float64)
    f8 = {k: np.asarray(v, np.float64) if v.dtype.kind == "f" else v for k, v in bn.items()}

    def L():
        res, _ = o.forward(f8["states"], f8["actions"], f8["returns"], f8["costs_return"], f8["time_steps"], f8["mask"],
                           episode_cost=f8["episode_cost"])
        return _oracle_functional(c, res, w)

    assert abs(float(loss.detach()) - L()) <= 1e-4 * max(1.0, abs(L()))
    feat = c.use_cost and (c.add_cost_feat or c.mul_cost_feat or c.cat_cost_feat)
    # with cost features the oracle has no detach: those tensors are pinned by the fused-step comparison below
    names = [k for k in got if not (feat and k in FEAT_DETACHED)]
    worst = _fd_check(c, o, L, got, names, np.random.RandomState(2), label=name)
    print(f"{name}: {len(names)} tensors, worst relative error {worst:.2e}")


def test_base_variant_matches_torch_cpu_autograd_fp64():
    from oracle.torch_cpu_baselines import TorchCDT
    c = CDT_CASES["cdt_small"]
    m, _, _ = _model(c)
    m.eval()
    bn = make_cdt_batch(c)
    w = _weights(c, c.B, c.T, 3)
    _gpu_functional(c, _call(m, _inputs(bn)), w).backward()
    tc = TorchCDT(make_cdt_params(c), seq_len=c.T, num_heads=c.heads, num_layers=c.layers,
                  cost_transform=c.cost_transform, stochastic=c.stochastic)
    tc.p = {k: v.detach().double().requires_grad_(True) for k, v in tc.p.items()}
    d = {k: torch.as_tensor(v).double() if v.dtype.kind == "f" else torch.as_tensor(v) for k, v in bn.items()}
    res = tc.forward(d["states"], d["actions"], d["returns"], d["costs_return"], d["time_steps"], d["mask"])
    tot = sum((torch.as_tensor(w[k]) * res[kk]).sum() for k, kk in (("mu", "mu"), ("ls", "ls"), ("lp", "cost_logp"),
                                                                     ("sp", "state_pred")))
    tot.backward()
    for k, p in m.named_parameters():
        ref = tc.p[k].grad.numpy()
        scale = max(np.abs(ref).max(), 1e-12)
        d_ = np.abs(p.grad.cpu().numpy() - ref).max()
        assert d_ <= 1e-5 * scale, f"{k}: {d_:.3e} vs max-abs {scale:.3e}"


def _reference_loss(m, c, out, b, temp):
    """CDTTrainer.train_one_step's loss (cdt.py:355-395) written in torch over the differentiable outputs."""
    ap, lp, sp = out
    mask = b["mask"]
    if m.stochastic:
        sel = mask > 0
        ll = ap.log_prob(b["actions"])[sel].mean()
        ent = ap.entropy()[sel].mean()
        act = -(ll + temp * ent)
    else:
        act = ((ap - b["actions"]) ** 2 * mask.unsqueeze(-1)).mean()
    cl = (torch.nn.functional.nll_loss(lp.reshape(-1, 2), b["costs"].flatten().long(), reduction="none")
          * mask.flatten()).mean()
    sl = ((sp[:, :-1] - b["states"][:, 1:]) ** 2 * mask[:, :-1].unsqueeze(-1)).mean()
    return act + c.cost_w * cl + c.state_w * sl


C5_SHAPE = CDTCase("cdt_c5_autograd", od=11, ad=3, B=1024, T=20, E=256, heads=8, layers=3, episode_len=1000, steps=1,
                   warmup=500, seed=6)


@pytest.mark.parametrize("name", list(CDT_CASES) + ["c5"])
def test_reference_loss_gradient_equals_the_fused_step(name):
    """The reference's training loss over the differentiable outputs, loss.backward(): every .grad equals the pre-clip
    gradient of one fused CDTTrainer step on the same batch and weights (dropout 0), read from its slabs."""
    from osrl_amd import _lib as L
    from osrl_amd.engine.core import cur_stream
    c = C5_SHAPE if name == "c5" else dataclasses.replace(CDT_CASES[name], dropout=0.0)
    m, tr, lg = _model(c)
    bn = make_cdt_batch(c)
    b = _inputs(bn)
    temp = m.temperature().detach() if m.stochastic else None
    _reference_loss(m, c, _call(m, b), b, temp).backward()
    got = {k: p.grad.clone() for k, p in m.named_parameters()}
    seen = []

    def probe(slabs, n_splits, counts):
        s = slabs.clone()
        L.check(L.load().osrl_reduce_slabs_counts(s.data_ptr(), s.data_ptr(), counts.data_ptr(), s.shape[1], s.shape[1],
                                                  cur_stream()), "rc")
        seen.append(s[0].clone())

    eng = m.engine(c.B, tr.cfg)
    eng._slab_probe = probe
    tr.train_one_step(b["states"], b["actions"], b["returns"], b["costs_return"], b["time_steps"], b["mask"],
                      b["episode_cost"], b["costs"])
    eng._slab_probe = None
    assert len(seen) == 1
    g = m.groups["cdt"]
    for k, gr in got.items():
        off, shape = g.layout["cdt." + k]
        ref = seen[0][off:off + gr.numel()].view(shape)
        scale = max(float(ref.abs().max()), 1e-12)
        d = float((gr - ref).abs().max())
        assert d <= 1e-6 * scale, f"{name} {k}: {d:.3e} vs max-abs {scale:.3e}"


def test_dropout_uses_fresh_masks_and_the_backward_uses_the_same():
    """train() mode, all three dropouts at 0.1: two calls draw different masks; the gradients of a call match fp64
    central differences of the oracle run with that call's masks (CDTEngine.dropout_masks())."""
    c = CDT_CASES["cdt_drop"]
    m, _, _ = _model(c)
    m.train()
    bn = make_cdt_batch(c)
    b = _inputs(bn)
    w = _weights(c, c.B, c.T, 5)
    out0 = _call(m, b)
    masks0 = {k: v.cpu().numpy() for k, v in m.grad_engine(c.B).dropout_masks().items()}
    m.zero_grad(set_to_none=True)
    _gpu_functional(c, _call(m, b), w).backward()
    eng = m.grad_engine(c.B)
    masks = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.dropout_masks().items()}
    assert any((masks[k] != masks0[k]).any() for k in masks), "two calls must draw different dropout masks"
    assert set(masks) == {"emb"} | {f"{k}{l}" for l in range(c.layers) for k in ("attn", "res1_", "res2_")}
    del out0
    got = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    o = build_cdt_oracle(c, np.float64)
    f8 = {k: np.asarray(v, np.float64) if v.dtype.kind == "f" else v for k, v in bn.items()}

    def L():
        res, _ = o.forward(f8["states"], f8["actions"], f8["returns"], f8["costs_return"], f8["time_steps"], f8["mask"],
                           drop=masks, episode_cost=f8["episode_cost"])
        return _oracle_functional(c, res, w)

    _fd_check(c, o, L, got, list(got), np.random.RandomState(6), label="dropout")


@pytest.mark.parametrize("name", ["cdt_small", "cdt_det", "cdt_v_prefix_det", "cdt_v_min"])
def test_input_gradients_match_central_differences(name):
    """states / actions / returns_to_go / costs_to_go / episode_cost gradients (the new osrl_cdt_embed_input_grad)
    against fp64 central differences of the oracle; costs_to_go gets none under cost_transform (the reference detaches
    it, cdt.py:187-188), time_steps and the mask never."""
    c = CDT_CASES[name]
    m, _, _ = _model(c)
    m.eval()
    bn = make_cdt_batch(c)
    names = ["states", "actions", "returns", "costs_return", "episode_cost"]
    b = _inputs(bn, grad=names)
    w = _weights(c, c.B, c.T, 7)
    _gpu_functional(c, _call(m, b), w).backward()
    o = build_cdt_oracle(c, np.float64)
    f8 = {k: np.asarray(v, np.float64) if v.dtype.kind == "f" else v for k, v in bn.items()}
    feat = c.use_cost and (c.add_cost_feat or c.mul_cost_feat or c.cat_cost_feat)
    expect = {"states": True, "actions": True, "returns": c.use_rew,
              "costs_return": c.use_cost and not c.cost_transform and not feat, "episode_cost": c.cost_prefix}
    if c.use_cost and c.cost_transform:
        assert b["costs_return"].grad is None
    rs = np.random.RandomState(8)
    for k in names:
        g = b[k].grad
        if not expect[k]:
            if k != "costs_return" or not feat:
                assert g is None, k
            continue
        g = g.cpu().numpy().astype(np.float64)
        assert g.shape == bn[k].shape
        base = f8[k].copy()
        for _ in range(4):
            v = rs.randn(*base.shape)
            v /= np.linalg.norm(v)
            vals = []
            for sgn in (1, -1):
                f8[k] = base + sgn * 1e-4 * v
                res, _ = o.forward(f8["states"], f8["actions"], f8["returns"], f8["costs_return"], f8["time_steps"],
                                   f8["mask"], episode_cost=f8["episode_cost"])
                vals.append(_oracle_functional(c, res, w))
            f8[k] = base
            fd = (vals[0] - vals[1]) / 2e-4
            gv = float((g * v).sum())
            scale = max(abs(fd), np.linalg.norm(g) / math.sqrt(g.size), 1e-12)
            assert abs(gv - fd) <= 1e-5 * scale, f"{name} d{k}: {gv:.8e} vs {fd:.8e}"
    assert b["time_steps"].grad is None and b["mask"].grad is None


def test_short_windows_padding_and_batch_size_changes():
    """A window of Tin < seq_len (left-aligned and padded): the same parameter gradients as the full window whose loss
    ignores the positions past Tin (causal attention); the halves of a batch add up to the whole batch (a change of B
    rebuilds the grad engine)."""
    c = CDT_CASES["cdt_drop"]
    m, _, _ = _model(c)
    m.eval()
    bn = make_cdt_batch(c)
    b = _inputs(bn)
    Tin = 3
    w = _weights(c, c.B, c.T, 9)
    for k in w:
        w[k][:, Tin:] = 0
    out = _call(m, b, Tin)
    assert out[1].shape == (c.B, Tin, 2) and out[2].shape == (c.B, Tin, c.od)
    _gpu_functional(c, out, w).backward()
    short = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    _gpu_functional(c, _call(m, b), w).backward()
    for k, p in m.named_parameters():
        scale = max(float(p.grad.abs().max()), 1e-12)
        assert float((short[k] - p.grad).abs().max()) <= 1e-6 * scale, k
    full = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    h = c.B // 2
    for sl in (slice(0, h), slice(h, c.B)):
        bb = {k: v[sl] for k, v in b.items()}
        ww = {k: v[sl] for k, v in w.items()}
        _gpu_functional(c, _call(m, bb), ww).backward()  # .grad accumulates over the two calls
    assert m.grad_engine(c.B - h).B == c.B - h
    for k, p in m.named_parameters():
        scale = max(float(full[k].abs().max()), 1e-12)
        assert float((full[k] - p.grad).abs().max()) <= 1e-5 * scale, k


def test_modes_flag_and_stale_graphs():
    c = CDT_CASES["cdt_v_prefix"]  # dropout 0.1 configured: eval mode must not apply it
    m, _, _ = _model(c)
    m.eval()
    b = _inputs(make_cdt_batch(c))
    on = _call(m, b)
    assert on[1].grad_fn is not None and on[0].loc.grad_fn is not None
    m.differentiable = False
    off = _call(m, b)
    assert off[1].grad_fn is None and off[2].grad_fn is None
    for x, y in ((on[0].loc, off[0].loc), (on[0].scale, off[0].scale), (on[1], off[1]), (on[2], off[2])):
        assert torch.equal(x.detach(), y), "eval-mode outputs with the flag on and off must be bit-equal"
    m.differentiable = True
    with torch.no_grad():
        ng = _call(m, b)
    assert ng[1].grad_fn is None and torch.equal(ng[2], off[2])
    # stale graph: a second forward on the same engine overwrote the first graph's activations
    first = _call(m, b)
    second = _call(m, b)
    with pytest.raises(RuntimeError, match="overwritten"):
        first[2].sum().backward()
    second[2].sum().backward()
    # double backward
    out = _call(m, b)
    (g,) = torch.autograd.grad(out[2].sum(), [m.state_pred_head.weight], create_graph=False)
    assert g.shape == m.state_pred_head.weight.shape
    out = _call(m, b)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(out[2].sum(), [m.state_pred_head.weight], create_graph=True)
    # parameters with requires_grad=False get none
    m.zero_grad(set_to_none=True)
    m.cost_pred_head.weight.requires_grad_(False)
    _call(m, b)[1].sum().backward()
    assert m.cost_pred_head.weight.grad is None and m.cost_pred_head.bias.grad is not None
    m.cost_pred_head.weight.requires_grad_(True)


def test_user_adamw_loop_then_trainer_act_path_and_checkpoint(tmp_path):
    """Five steps of torch.optim.AdamW on model.parameters() with the reference loss track the same loop on TorchCDT
    (float64 CPU autograd) within the project's multi-step gate; the fused trainer, the act path and checkpoints then
    see the updated weights."""
    from oracle.torch_cpu_baselines import TorchCDT
    from osrl_amd.common.checkpoint import load_checkpoint, save_checkpoint
    c = CDT_CASES["cdt_small"]
    m, tr, lg = _model(c)
    bn = make_cdt_batch(c)
    b = _inputs(bn)
    opt = torch.optim.AdamW(m.parameters(), lr=c.lr, weight_decay=c.wd)
    tc = TorchCDT(make_cdt_params(c), seq_len=c.T, num_heads=c.heads, num_layers=c.layers,
                  cost_transform=c.cost_transform, stochastic=c.stochastic)
    tc.p = {k: v.detach().double().requires_grad_(True) for k, v in tc.p.items()}
    topt = torch.optim.AdamW(list(tc.p.values()), lr=c.lr, weight_decay=c.wd)
    d = {k: torch.as_tensor(v).double() if v.dtype.kind == "f" else torch.as_tensor(v) for k, v in bn.items()}
    temp = float(m.temperature())
    for _ in range(5):
        opt.zero_grad()
        _reference_loss(m, c, _call(m, b), b, temp).backward()
        opt.step()
        topt.zero_grad()
        res = tc.forward(d["states"], d["actions"], d["returns"], d["costs_return"], d["time_steps"], d["mask"])
        ap = torch.distributions.Normal(res["mu"], res["ls"].exp())
        _reference_loss(m, c, (ap, res["cost_logp"], res["state_pred"]), d, temp).backward()
        topt.step()
    for k, p in m.named_parameters():
        diff = float((p.detach().cpu().double() - tc.p[k].detach()).abs().max())
        assert diff <= 2e-5, f"{k}: {diff:.3e} after 5 user AdamW steps"
    # the fused step starts from the user-updated weights: its gradient == the differentiable path's at those weights
    m.zero_grad(set_to_none=True)
    _reference_loss(m, c, _call(m, b), b, temp).backward()
    seen = []
    eng = m.engine(c.B, tr.cfg)
    eng._slab_probe = lambda slabs, n, counts: seen.append(slabs[:n].sum(0).clone())
    tr.train_one_step(b["states"], b["actions"], b["returns"], b["costs_return"], b["time_steps"], b["mask"],
                      b["episode_cost"], b["costs"])
    eng._slab_probe = None
    g = m.groups["cdt"]
    for k, p in m.named_parameters():
        off, shape = g.layout["cdt." + k]
        ref = seen[0][off:off + p.numel()].view(shape)
        assert float((p.grad - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1e-12), k
    # more user steps after the fused step, then the act path and a checkpoint round trip
    opt.zero_grad()
    _reference_loss(m, c, _call(m, b), b, temp).backward()
    opt.step()
    m.eval()
    obs = bn["states"][0, 0]
    pol = m.fast_policy()
    a_fast = np.asarray(pol.reset(obs, 3.0, 5.0))
    with torch.no_grad():
        ap, _, _ = m(t(obs)[None, None], torch.zeros(1, 1, c.ad, device=DEV), t([[3.0]]).float(), t([[5.0]]).float(),
                     torch.zeros(1, 1, dtype=torch.long, device=DEV), None, None)
    want = ap.mean.clamp(-1, 1)[0, -1].cpu().numpy()
    assert np.abs(a_fast - want).max() <= 1e-5, (a_fast, want)
    path = str(tmp_path / "cdt.pt")
    save_checkpoint(m, path)
    m2, _, _ = _model(c)
    load_checkpoint(m2, path)
    for (k, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(p.detach(), p2.detach()), k
