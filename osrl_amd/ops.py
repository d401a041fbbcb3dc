"""Tensor-level ops over libosrl_amd.so for code outside the captured step plan
(``model.act``, module ``forward`` methods, user losses).

``mlp_apply`` is a ``torch.autograd.Function`` whose forward AND backward are the fused HIP
kernels of csrc/mlp.hip (forward, backward-dz with dX, split-K dW).  ``cdt_apply`` is the same for
the CDT transformer (engine/cdt.py forward / backward, csrc/cdt_grad.hip for the input gradients).  Nothing here falls back to
aten arithmetic; without the library (or without a HIP device) every call raises.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib as L
from .engine import glue as G
from .engine.core import DwPlan, FlatGroup, MlpRun, NetDesc, cur_stream, randn_fill


def _chk(x: torch.Tensor) -> torch.Tensor:
    if not x.is_cuda:
        raise RuntimeError("osrl_amd ops need HIP device tensors (no CPU fallback)")
    return x.contiguous().float()


def randn(shape, device, seed: int = 0, stream_id: int = 7) -> torch.Tensor:
    """Standard-normal noise from the on-device Philox generator (csrc/rng.hip)."""
    out = torch.empty(shape, dtype=torch.float32, device=device)
    _RandnCounter.n += 1
    randn_fill(out, seed + 0x9E3779B97F4A7C15 * _RandnCounter.n % (1 << 63), stream_id, None)
    return out


class _RandnCounter:
    n = 0


class _FusedMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, desc: NetDesc, x0: torch.Tensor, x1: Optional[torch.Tensor], *params):
        rows = x0.shape[0]
        need_grad = any(ctx.needs_input_grad)  # (grad mode is off inside Function.forward)
        for g in desc.groups():  # weights may have been edited since the last pack: refresh (cheap)
            g.repack()
        run = MlpRun(desc, rows, need_grad, x0.device)
        run.forward(x0, x1)
        ctx.run, ctx.desc, ctx.has_x1 = run, desc, x1 is not None
        ctx.d0 = x0.shape[1]
        return run.y

    @staticmethod
    def backward(ctx, dy):
        run, desc = ctx.run, ctx.desc
        dy = dy.contiguous()
        din = desc.dims[0]
        run.setup_backward(dy, need_dz=True, dx_cols=(0, din))
        run.backward_dz()
        # weight gradients through a temporary flat slab with this net's own layout
        grp = FlatGroup("tmp", dy.device)
        entries = []
        for e in range(desc.E):
            for l in range(desc.nl):
                wk, bk = f"{e}.{l}.w", f"{e}.{l}.b"
                grp.add(wk, desc.nets[e][l].W.shape)
                grp.add(bk, desc.nets[e][l].b.shape)
                a = run.x if l == 0 else run.h[e][l - 1]
                entries.append((run.dz[e][l], a, wk, bk))
        grp.finalize()
        plan = DwPlan(grp, entries, run.rows, dy.device)
        plan.launch()
        grads = []
        for e in range(desc.E):
            for l in range(desc.nl):
                r = desc.nets[e][l]
                gw, gb = grp.grad_view(f"{e}.{l}.w"), grp.grad_view(f"{e}.{l}.b")
                # packed heads: split the stacked gradient back onto the individual nn.Parameters
                ws = r.wparams if r.wparams is not None else [r.W]
                bs = r.bparams if r.bparams is not None else [r.b]
                o = 0
                for w in ws:
                    grads.append(gw[o:o + w.shape[0]].contiguous())
                    o += w.shape[0]
                o = 0
                for bb in bs:
                    grads.append(gb[o:o + bb.shape[0]].contiguous())
                    o += bb.shape[0]
        dx = run.dx.sum(0)
        d0 = ctx.d0
        return (None, dx[:, :d0].contiguous(), dx[:, d0:].contiguous() if ctx.has_x1 else None, *grads)


class _CDTApply(torch.autograd.Function):
    """The CDT forward (cdt.py:166-265, without the aten tail: log_softmax, exp of log_std) on a grad engine of the
    model (``CDT.grad_engine``), and its backward on the same engine's HIP kernels."""

    @staticmethod
    def forward(ctx, model, eng, time_steps, padding_mask, states, actions, returns, costs_to_go, episode_cost,
                *params):
        Tin = model.load_window(eng, states, actions, returns, costs_to_go, time_steps, padding_mask, episode_cost)
        model.repack()  # parameters may have been edited (a user optimizer) since the last pack
        if eng.p_emb > 0 or eng.p_attn > 0 or eng.p_res > 0:
            eng.st.tick()  # fresh dropout masks per call, like nn.Dropout; the backward regenerates the same ones
        eng.forward(train=True)  # (train=True also keeps what the backward reads: attention row statistics, keep bits)
        eng.fwd_count = getattr(eng, "fwd_count", 0) + 1
        ctx.eng, ctx.fwd_count, ctx.Tin, ctx.model = eng, eng.fwd_count, Tin, model
        ctx.in_shapes = [(x.shape, x.dtype) if torch.is_tensor(x) else None
                         for x in (states, actions, returns, costs_to_go, episode_cost)]
        ctx.save_for_backward(*params)  # autograd's version check: parameters edited in place before backward() raise
        B, T = eng.B, eng.T
        return tuple(buf.view(B, T, buf.shape[1])[:, :Tin].clone() for buf in (eng.head, eng.logits, eng.sp))

    @staticmethod
    def backward(ctx, dhead, dlogits, dsp):
        if torch.is_grad_enabled():
            raise RuntimeError("CDT differentiable forward: double backward (create_graph=True) is not supported")
        eng, Tin, m = ctx.eng, ctx.Tin, ctx.model
        if getattr(eng, "fwd_count", 0) != ctx.fwd_count:
            raise RuntimeError("CDT differentiable forward: this graph's activations were overwritten by a later "
                               "forward on the same engine (same batch size and mode); call backward() before the next "
                               "forward, or recompute the forward")
        ctx.saved_tensors  # noqa: B018  (raises if a parameter was modified in place since the forward)
        B, T = eng.B, eng.T
        for buf, gr in ((eng.dhead, dhead), (eng.dlogits, dlogits), (eng.dsp, dsp)):  # seeds in row b*T + t
            v = buf.view(B, T, buf.shape[1])
            if Tin < T:
                v[:, Tin:].zero_()
            v[:, :Tin].copy_(gr)
        eng.backward()
        eng.reduce_grads()
        need = ctx.needs_input_grad
        g = eng.g
        flat = g.slabs[0].clone()  # (the slabs are this engine's scratch: the next backward overwrites them)
        grads = []
        for i, (name, _) in enumerate(m.named_parameters()):
            if not need[9 + i]:
                grads.append(None)
                continue
            off, shape = g.layout["cdt." + name]
            n = 1
            for d in shape:
                n *= d
            grads.append(flat[off:off + n].view(shape))
        # inputs (cdt.py:178-213): the reference detaches costs_to_go under cost_transform (cdt.py:187-188); returns,
        # costs and the episode cost only feed a token where the model has one
        want = [need[4], need[5], need[6] and m.use_rew, need[7] and m.use_cost and not m.cost_transform_on,
                need[8] and m.cost_prefix]
        dins = [None] * 5
        if any(want):
            f = dict(dtype=torch.float32, device=eng.dev)
            od, ad = m.state_dim, m.action_dim
            outs = [torch.empty(B, T, od, **f) if want[0] else None, torch.empty(B, T, ad, **f) if want[1] else None,
                    torch.empty(B, T, **f) if want[2] else None, torch.empty(B, T, **f) if want[3] else None,
                    torch.empty(B, **f) if want[4] else None]
            v = eng._v
            L.check(L.load().osrl_cdt_embed_input_grad(
                eng.dseq.data_ptr(), v("cdt.state_emb.weight"), v("cdt.action_emb.weight"),
                v("cdt.return_emb.weight") if m.use_rew else None, v("cdt.cost_emb.weight") if m.use_cost else None,
                v("cdt.prefix_emb.weight") if m.cost_prefix else None, B, T, od, ad, eng.E, int(m.use_rew),
                int(m.use_cost), int(m.cost_prefix), *[None if o is None else o.data_ptr() for o in outs],
                cur_stream()), "osrl_cdt_embed_input_grad")
            for k, o in enumerate(outs):
                if o is not None:
                    shape, dtype = ctx.in_shapes[k]
                    dins[k] = (o if k == 4 else o[:, :Tin]).reshape(shape).to(dtype)
        return (None, None, None, None, *dins, *grads)


def cdt_apply(model, eng, states, actions, returns_to_go, costs_to_go, time_steps, padding_mask=None,
              episode_cost=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Differentiable CDT forward (``CDT(..., differentiable=True)``): (head [B, Tin, 2*ad (mu | log_std) or ad],
    cost logits [B, Tin, 2], state predictions [B, Tin, od]) attached to the autograd graph.  Forward, backward and the
    input gradients run on the HIP kernels of the fused train step (engine/cdt.py ``forward`` / ``backward``) plus one
    launch for the input gradients (osrl_cdt_embed_input_grad); only the seeds' copies and the slab read-out are aten.

    * Gradients: one per parameter (``None`` where ``requires_grad`` is off), accumulated into ``.grad`` by autograd;
      ``states`` / ``actions`` / ``returns_to_go`` / ``costs_to_go`` / ``episode_cost`` as the reference's nn.Linear
      embeddings give them -- ``costs_to_go`` only without ``cost_transform`` (the reference detaches it, cdt.py:187),
      and through the token embedding only (the cost features use the detached embedding, cdt.py:243-250).
      ``time_steps`` and the padding mask get none; window positions past Tin (the padding of a short window) neither.
    * Activations live in the engine, not per call: a forward on the same engine (same batch size and mode) overwrites
      them, and the backward of an earlier graph then raises RuntimeError instead of returning wrong gradients.
    * Dropout (train() mode, p > 0): fresh masks per call; the backward regenerates exactly those masks.
    * Not supported: double backward (``create_graph=True`` raises), data parallelism, hipGraph capture of this path,
      gradients of ``log_temperature`` (not an input of the forward).  ``CDTTrainer`` stays the fused training path."""
    params = [p for _, p in model.named_parameters()]
    return _CDTApply.apply(model, eng, time_steps, padding_mask, states, actions, returns_to_go, costs_to_go,
                           episode_cost, *params)


def mlp_apply(desc: NetDesc, x0: torch.Tensor, x1: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[E, rows, out] = fused MLP ensemble on cat(x0, x1).  Differentiable w.r.t. inputs and weights
    when the NetDesc was built from live ``nn.Parameter`` storage (pass the params for autograd)."""
    x0 = _chk(x0)
    x1 = None if x1 is None else _chk(x1)
    params = [t for net in desc.nets for r in net
              for t in ((r.wparams if r.wparams is not None else [r.W]) + (r.bparams if r.bparams is not None else [r.b]))]
    return _FusedMLP.apply(desc, x0, x1, *params)


def gauss_head(head: torch.Tensor, eps: Optional[torch.Tensor], deterministic: bool, with_logprob: bool
               ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """SquashedGaussianMLPActor tail (net.py:176-205): returns (tanh(u), logp)."""
    head = _chk(head)
    rows, ad = head.shape[0], head.shape[1] // 2
    if not deterministic and eps is None:
        eps = randn((rows, ad), head.device)
    a = torch.empty(rows, ad, dtype=torch.float32, device=head.device)
    logp = torch.empty(rows, dtype=torch.float32, device=head.device) if with_logprob else None
    G.gauss_head(head, None if deterministic else _chk(eps), rows, ad, 1.0, a=a, logp=logp)
    return a, logp


def bcq_perturb(dec: torch.Tensor, t: torch.Tensor, phi: float, max_action: float) -> torch.Tensor:
    dec, t = _chk(dec), _chk(t)
    a = torch.empty_like(dec)
    G.bcq_perturb(dec, t, dec.shape[0], dec.shape[1], phi, max_action, a)
    return a


@torch.no_grad()
def cpq_act(model, obs: torch.Tensor, deterministic: bool):
    """CPQ._actor_forward (cpq.py:115-123) for inference: (max_action*tanh(u), logp)."""
    a, logp = model.actor(obs, deterministic, True)
    return a * model.max_action, logp
