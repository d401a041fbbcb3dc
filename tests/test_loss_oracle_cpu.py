"""The fp64 oracle of the loss / glue kernels (tests/loss_oracle.py) is itself checked here, without a GPU:

* its hand-derived gradients and statistics equal ``torch.float64`` autograd of the formulas written the way the
  reference writes them (``torch.min`` over stacked members, ``torch.min(a, b)``, ``clamp``, ``softmax(dim=0)``) on the
  whole case table, ties and clamp edges included -- torch's tie rules are the specification;
* no unplanted row of any case lies within 1e-4 of a switch point, so the GPU comparison excludes nothing;
* the gates of ``loss_oracle.compare`` are sharp: each listed mutation of the oracle fails them by >= 4 x on at least one
  case of every kernel it applies to;
* the argument lists of tests/loss_cases.py are those of include/osrl_amd.h and of ``osrl_amd._lib``.
"""
import os
import re

import numpy as np
import pytest
import torch

import loss_cases as LC
import loss_oracle as LO

D = torch.float64


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=D, requires_grad=grad)


def _min0(q):
    return torch.min(q, dim=0).values


def _inv(x, rows):
    g = x.get("rows_global", 0)
    return 1.0 / (g if g > 0 else rows)


def _head_u(x, head, lo=-20.0, hi=2.0):
    ad = head.shape[1] // 2
    return head[:, :ad] + torch.exp(torch.clamp(head[:, ad:], lo, hi)) * _t(x["eps"])


def _grad(loss, *leaves):
    return [g.numpy() for g in torch.autograd.grad(loss, leaves, allow_unused=False)]


# ---- torch restatements: kernel -> (x -> (x as given to the oracle, {output name: value})) ----------------------------
def t_gauss_head_bwd(x):
    head = _t(x["head"], True)
    u = _head_u(x, head)
    loss = (x["max_action"] * torch.tanh(u) * _t(x["da_nets"]).sum(0)).sum()
    return dict(x, tanh_u=torch.tanh(u).detach().numpy()), dict(dhead=_grad(loss, head)[0])


def t_bear_head_bwd(x):
    head = _t(x["head"], True)
    u = _head_u(x, head)
    first = torch.arange(0, head.shape[0], x["n_samples"])
    loss = float(x["coef"][0]) * (_t(x["du_mmd"]) * u).sum() + (torch.tanh(u[first]) * _t(x["da_nets"]).sum(0)).sum()
    return dict(x, tanh_u=torch.tanh(u).detach().numpy()), dict(dhead=_grad(loss, head)[0])


def _kl(head, Lz):
    std = torch.exp(torch.clamp(head[:, Lz:], -4.0, 15.0))
    return -0.5 * (1 + torch.log(std.pow(2)) - head[:, :Lz].pow(2) - std.pow(2))


def t_vae_loss(x):
    u, head = _t(x["u"], True), _t(x["head"])
    inv = _inv(x, u.shape[0])
    loss = ((u - _t(x["act"])) ** 2).sum() * inv / x["ad"] + x["beta"] * _kl(head, x["L"]).sum() * inv / x["L"]
    return x, dict(du=_grad(loss, u)[0], stat=np.array([loss.item()]))


t_vae_loss_ws = t_vae_loss


def t_vae_latent_bwd(x):
    head = _t(x["head"], True)
    z = _head_u(x, head, -4.0, 15.0)
    loss = (z * _t(x["dz"])).sum() + x["beta"] * _kl(head, x["L"]).sum() * _inv(x, head.shape[0]) / x["L"]
    return x, dict(dhead=_grad(loss, head)[0])


def t_cpq_critic_loss(x):
    q = _t(x["q"], True)
    backup = _t(x["rew"]) + x["gamma"] * (1 - _t(x["done"])) * (_min0(_t(x["qc_old"])) <= x["q_thres"]) * _min0(_t(x["q_old"]))
    loss = ((q - backup[None]) ** 2).sum() * _inv(x, q.shape[1])
    return x, dict(dq=_grad(loss, q)[0], stat=np.array([loss.item()]))


def t_cpq_cost_loss(x):
    qc = _t(x["qc"], True)
    backup = _t(x["cost"]) + x["gamma"] * _min0(_t(x["qc_old_next"]))
    inv = _inv(x, qc.shape[1])
    loss = ((qc - backup[None]) ** 2).sum() * inv
    out = dict(dq=_grad(loss, qc)[0])
    if x.get("qc_sampled") is not None:
        kl, quant = _t(x["kl"]), float(x["quantile"][0])
        ood = ((kl >= quant) * _min0(_t(x["qc_sampled"]))).mean(0).sum() * inv
        out["ood_mean_out"] = np.array([ood.item()])
    elif x.get("ood_mean") is not None:
        ood = _t(x["ood_mean"])[0]
    else:
        out["stat"] = np.array([loss.item(), np.nan])
        return x, out
    la = _t(x["log_alpha"])[0]
    total = loss - x.get("stat_share", 1.0) * la.exp() * (ood - x["qc_thres"])
    la_new = torch.clamp(la + x["alpha_lr"] * la.exp() * (x["qc_thres"] - ood), -5.0, 5.0)
    out.update(stat=np.array([total.item(), x.get("stat_share", 1.0) * la_new.exp().item()]),
               log_alpha=np.array([la_new.item()]))
    return x, out


t_cpq_cost_loss_ood = t_cpq_cost_loss


def t_cpq_actor_loss(x):
    q = _t(x["q"], True)
    loss = (-(_min0(_t(x["qc"])) <= x["q_thres"]).double() * _min0(q)).sum() * _inv(x, q.shape[1])
    return x, dict(dq=_grad(loss, q)[0], stat=np.array([loss.item()]))


def t_mse_loss(x):
    u = _t(x["u"], True)
    loss = ((u - _t(x["target"])) ** 2).sum() / (x["n_global"] if x["n_global"] > 0 else x["n"])
    return x, dict(du=_grad(loss, u)[0], stat=np.array([loss.item()]))


def t_bcq_perturb_bwd(x):
    t = _t(x["t"], True)
    ma = x["max_action"]
    a = torch.clamp(_t(x["dec"]) + x["phi"] * ma * t, -ma, ma)
    return x, dict(dt=_grad((a * _t(x["da_nets"]).sum(0)).sum(), t)[0])


def t_bcq_critic_loss(x):
    q_on, q_t, n1 = _t(x["q_on"], True), _t(x["q_t"]), x["n1"]
    q1, q2 = _min0(q_t[:n1]), _min0(q_t[n1:])
    v = x["lmbda"] * torch.min(q1, q2) + (1 - x["lmbda"]) * torch.max(q1, q2)
    nd = 1 - _t(x["done"]) if x.get("done") is not None else 1.0
    backup = _t(x["base"]) + x["gamma"] * nd * v.max(1).values
    loss = ((q_on - backup[None]) ** 2).sum() * _inv(x, q_on.shape[1])
    return x, dict(dq=_grad(loss, q_on)[0], stat=np.array([loss.item()]))


t_bcq_critic_loss_ws = t_bcq_critic_loss


def _twin(q, n1):
    return torch.min(_min0(q[:n1]), _min0(q[n1:]))


def _controller(x, qc_pi):
    """The multiplier (a constant of the loss: computed under no_grad in the reference) and the controller's new state
    words, from the train-step oracle's LagrangianPIDController -- nothing here comes from tests/loss_oracle.py."""
    from oracle.osrl_oracle import PID
    c = PID(x["KP"], x["KI"], x["KD"], x["qc_thres"])
    c.error_old, c.error_integral = float(x["pid"][0]), float(x["pid"][1])
    mult = c.control(qc_pi.detach().numpy())
    return mult, np.array([c.error_old, c.error_integral])


def t_bcq_actor_loss(x):
    q, qc = _t(x["q"], True), _t(x["qc"], True)
    q_pi, qc_pi = _twin(q, x["nq1"]), _twin(qc, x["nc1"])
    mult, pid = _controller(x, qc_pi)
    penalty = ((qc_pi - x["qc_thres"]) * mult).mean()
    loss = (-q_pi).mean() + penalty
    dq, dqc = _grad(loss, q, qc)
    return x, dict(dq=dq, dqc=dqc, pid=pid, stat=np.array([loss.item(), penalty.item(), mult]))


def t_bear_actor_loss(x):
    q, qc = _t(x["q"], True), _t(x["qc"], True)
    inv = _inv(x, q.shape[1])
    mult, pid = _controller(x, _twin(qc, x["nc1"]))
    mmd, la = _t(x["mmd"]), _t(x["log_alpha"])[0]
    if x["step"] - 1 >= x["start_update_policy_step"]:
        loss = (-_twin(q, x["nq1"]) + la.exp() * (mmd - x["target_mmd_thresh"])).sum() * inv
    else:
        loss = (la.exp() * (mmd - x["target_mmd_thresh"])).sum() * inv + 0.0 * q.sum()
    penalty = ((_twin(qc, x["nc1"]) - x["qc_thres"]) * mult).sum() * inv
    loss = loss + penalty
    dq, dqc = _grad(loss, q, qc)
    la_new = torch.clamp(la + x["alpha_lr"] * la.exp() * (mmd - x["target_mmd_thresh"]).mean(), -5.0, 5.0)
    stat = np.full(5, np.nan)
    stat[:] = loss.item(), mmd.mean().item(), penalty.item(), mult, la_new.exp().item()
    return x, dict(dq=dq, dqc=dqc, stat=stat, pid=pid, log_alpha=np.array([la_new.item()]), coef=np.array([la.exp().item() * inv]))


def _f_torch(f_type):
    """get_f_div_fn of the reference, in torch: f and f'^-1."""
    if f_type == 0:
        return (lambda w: 0.5 * (w - 1) ** 2), (lambda z: z + 1)
    if f_type == 1:
        return (lambda w: torch.where(w < 1, w * (torch.log(w + 1e-10) - 1) + 1, 0.5 * (w - 1) ** 2),
                lambda z: torch.where(z < 0, torch.exp(torch.clamp(z, max=0.0)), z + 1))
    return (lambda w: w * torch.log(w + 1e-10)), (lambda z: torch.exp(z - 1))


def t_dice_nu_step(x):
    """e and w are the kernel's inputs: their VALUES are kept, their dependence on nu (and of w on e) is attached."""
    nu2 = _t(x["nu2"], True)
    f, g = _f_torch(x["f_type"])
    nu_s, nu_n = _min0(nu2[:, 0]), _min0(nu2[:, 1])
    dep = x["gamma"] * (1 - _t(x["done"])) * nu_n - nu_s
    e = _t(x["e"]) + dep - dep.detach()
    wd = torch.relu(g(e / x["alpha"]))
    w = _t(x["w"]) + wd - wd.detach()
    inv = _inv(x, e.shape[0])
    loss = ((1 - x["gamma"]) * nu_s * _t(x["is_init"]) / x["init_state_propotion"]).sum() * inv \
        + (w * e - x["alpha"] * f(w)).sum() * inv
    stat = np.full(7, np.nan)
    stat[0], stat[1], stat[2] = f(_t(x["w"])).sum().item() * inv, (_t(x["e"]) ** 2).sum().item() * inv, loss.item()
    return x, dict(dnu=_grad(loss, nu2)[0], stat=stat)


def t_dice_chi_step(x):
    if x.get("chi2") is None:
        return x, {}
    chi2 = _t(x["chi2"], True)
    w, gam, B = _t(x["w"]), x["gamma"], x["rows"]
    cs, cn = _min0(chi2[:, 0]), _min0(chi2[:, 1])
    ell = (1 - gam) * cs * _t(x["is_init"]) / x["init_state_propotion"] \
        + w * (_t(x["cost"]) + gam * (1 - _t(x["done"])) * cn - cs)
    tau = float(x["work"][1])
    weights = torch.softmax(ell / tau, dim=0) * B
    log_weights = torch.log_softmax(ell / tau, dim=0) + np.log(B)
    loss = (weights * ell).mean()
    dkl = (weights * log_weights - weights + 1).mean().item()
    return x, dict(dchi=_grad(loss, chi2)[0], stat=np.array([loss.item(), tau * (x["cost_ub_epsilon"] - dkl), dkl]))


def t_dice_actor_loss(x):
    head, ad = _t(x["head"], True), x["ad"]
    dist = torch.distributions.Normal(head[:, :ad], torch.exp(torch.clamp(head[:, ad:], -20.0, 2.0)))
    loss = -(_t(x["w"]) * dist.log_prob(_t(x["act"])).sum(-1)).sum() * _inv(x, head.shape[0])
    return x, dict(dhead=_grad(loss, head)[0], stat=np.array([loss.item()]))


TORCH = {k[2:]: v for k, v in list(globals().items()) if k.startswith("t_")}
GRAD_CASES = [c for c in LC.CASES if c.kernel in TORCH]


@pytest.mark.parametrize("c", GRAD_CASES, ids=lambda c: c.id)
def test_oracle_equals_torch_fp64_autograd(c):
    x, want = TORCH[c.kernel](LC.inputs(c))
    ref = LO.reference(c.kernel, x)[0]
    for name, v in want.items():
        r = ref.out[name]
        ok = ~np.isnan(v)
        assert np.array_equal(np.isnan(r) | ~ok, ~ok) or name == "stat", name
        scale = max(1.0, float(np.abs(r[ok]).max())) if ok.any() else 1.0
        np.testing.assert_allclose(r[ok], v[ok], rtol=1e-12, atol=1e-12 * scale, err_msg=f"{c.id} {name}")


def test_every_gradient_kernel_has_a_torch_restatement():
    with_grad = {"gauss_head_bwd", "bear_head_bwd", "vae_loss", "vae_loss_ws", "vae_latent_bwd", "cpq_critic_loss",
                 "cpq_cost_loss", "cpq_cost_loss_ood", "cpq_actor_loss", "mse_loss", "bcq_perturb_bwd", "bcq_critic_loss",
                 "bcq_critic_loss_ws", "bcq_actor_loss", "bear_actor_loss", "dice_nu_step", "dice_chi_step",
                 "dice_actor_loss"}
    assert with_grad <= set(TORCH)
    assert set(LC.SPECS) == set(LO.REFS) == {c.kernel for c in LC.CASES}


@pytest.mark.parametrize("c", LC.CASES, ids=lambda c: c.id)
def test_no_unplanted_row_sits_near_a_kink(c):
    """Every indicator's operands are either exactly at the switch point (planted) or further than 1e-4 of their scale
    from it, so fp32 rounding cannot flip an indicator and the GPU comparison excludes no row."""
    ref = LO.reference(c.kernel, LC.inputs(c))[0]
    for name, d in ref.kink.items():
        d = np.asarray(d)
        near = (d != 0) & (d <= 1e-4)
        assert not near.any(), (c.id, name, c.seed, np.argwhere(near)[:4].tolist(), d[near][:4])


def test_the_oracle_fp32_run_passes_its_own_gates():
    for c in LC.CASES:
        r64, r32 = LO.reference(c.kernel, LC.inputs(c))
        worst, where = LO.compare(r32.out, r64, r32)
        assert worst <= 1.0, (c.id, where, worst)


# mutation -> the kernels it applies to
APPLIES = {
    "drop_last": ["vae_loss", "vae_loss_ws", "cpq_critic_loss", "cpq_ood_mean", "cpq_cost_loss", "cpq_cost_loss_ood",
                  "cpq_actor_loss", "mse_loss", "bcq_critic_loss", "bcq_critic_loss_ws", "bcq_actor_sums", "bcq_actor_loss",
                  "bear_actor_sums", "bear_actor_loss", "dice_nu_step", "dice_chi_step", "dice_actor_loss"],
    "tie_second": ["cpq_actor_loss", "bcq_actor_loss", "bear_actor_loss", "dice_nu_step", "dice_chi_step"],
    "split_one_side": ["bcq_actor_loss", "bear_actor_loss"],
    "lt_strict": ["cpq_critic_loss", "cpq_actor_loss", "cpq_ood_mean", "cpq_cost_loss_ood"],
    "no_grad_at_2": ["gauss_head_bwd", "bear_head_bwd", "dice_actor_loss", "vae_latent_bwd"],  # (its upper edge is 15)
    "rows_for_global": [],  # filled below: every kernel with a data-parallel case
    "no_share": ["cpq_cost_loss", "cpq_alpha_step", "bcq_actor_loss", "bear_actor_loss", "dice_nu_step", "dice_chi_step"],
    "skip_m4": ["cpq_critic_loss", "cpq_ood_mean", "cpq_cost_loss", "cpq_cost_loss_ood", "cpq_actor_loss",
                "gauss_head_bwd", "bcq_perturb_bwd", "bear_head_bwd", "bcq_critic_loss"],
    "no_bias_corr": ["dice_nu_step", "dice_chi_step"],
    "no_done": ["cpq_critic_loss", "bcq_critic_loss", "bcq_critic_loss_ws", "dice_optimal_w", "dice_chi_step",
                "dice_nu_step"],
}
APPLIES["drop_1024"] = APPLIES["drop_last"]
APPLIES["rows_for_global"] = sorted({c.kernel for c in LC.CASES if c.dp})


def _dp_inputs(c):
    """The first half of a data-parallel case, as one rank sees it."""
    x = LC.inputs(c)
    return LC.split(x, 0, LC.DP_SPLIT[0], LC.DP_ROWS)


@pytest.mark.parametrize("mutation", LO.MUTATIONS)
def test_the_gates_catch_every_mutation_by_4x(mutation):
    assert set(APPLIES) == set(LO.MUTATIONS)
    for kernel in APPLIES[mutation]:
        worst = 0.0
        for c in LC.CASES:
            if c.kernel != kernel:
                continue
            dp = mutation in ("rows_for_global", "no_share")
            if dp and not (c.dp or kernel == "cpq_alpha_step"):
                continue
            x = _dp_inputs(c) if (dp and c.dp) else LC.inputs(c)
            r64, r32 = LO.reference(kernel, x)
            m64, _ = LO.reference(kernel, x, mutation)
            worst = max(worst, LO.compare(m64.out, r64, r32)[0])
        assert worst >= 4.0, (mutation, kernel, worst)


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def _header_protos():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "osrl_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(osrl_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [" ".join(p.split()) for p in m.group(2).split(",")]
    return out


@pytest.mark.parametrize("kernel", sorted(LC.SPECS))
def test_argument_lists_match_the_header_and_the_ctypes_table(kernel):
    import ctypes as C
    from osrl_amd import _lib as L
    protos = _header_protos()
    params = protos["osrl_" + kernel]
    sp = LC.spec(kernel)
    assert len(params) == len(sp) + 1 and params[-1].replace(" ", "") == "void*stream", params
    argtypes = L.PROTOTYPES["osrl_" + kernel]
    assert len(argtypes) == len(params)
    kinds = {"i": ("int32_t", C.c_int32), "l": ("int64_t", C.c_int64), "f": ("float", C.c_float)}
    for (kind, name), p, at in zip(sp, params, argtypes):
        ptype, pname = p.rsplit(" ", 1) if "*" not in p else (p[: p.rindex("*") + 1], p[p.rindex("*") + 1:].strip())
        assert pname == name, (kernel, p, name)
        if kind in kinds:
            assert ptype == kinds[kind][0] and at is kinds[kind][1], (kernel, p, at)
        elif kind == "st":
            assert "osrl_step_state_t" in ptype and at is C.c_void_p, (kernel, p)
        else:
            assert ptype.replace("const ", "") in ("float*", "float *") and at in (C.c_void_p, L._fp), (kernel, p, at)
    assert kernel in LC.REFUSALS or kernel == "cpq_alpha_step"
    for over in LC.REFUSALS.get(kernel, []):
        assert set(over) <= {n for _, n in sp}, over
