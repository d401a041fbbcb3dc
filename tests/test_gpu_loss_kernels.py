"""Every loss / glue entry point of csrc/glue.hip, csrc/bear.hip and csrc/dice.hip against the fp64 restatement of its
formula (tests/loss_oracle.py) on the case table of tests/loss_cases.py: both instantiations of the CPQ kernels (<= 4 and
5 members), the second and third pass of the 1024-thread loops, planted ties / threshold equalities / clamp edges /
saturated tanh and softplus, the PID and log_alpha clamps, scalar Adam at step 3 with nonzero moments, the
data-parallel arguments on a 512 + 513 split, and the host-side refusals.  Gates: tests/loss_oracle.py (module
docstring); the equivalence tests of the suite (grid kernels, descriptor twins, fused tails) compare a launch with
one of these launches, so they bottom out here; the seeded backward launches meet fp64 in tests/test_gpu_seed_kernels.py.

Every output buffer is filled with NaN before the launch and carries a 64-element guard tail: the launch must write every
word the oracle defines, leave alone every word it marks untouched, and nothing past the end.
"""
import numpy as np
import pytest
import torch

import loss_cases as LC
import loss_oracle as LO

pytestmark = pytest.mark.gpu
GUARD = 64
SUMMED = ("stat", "out", "work", "ood_mean_out")  # batch statistics: a rank's launch leaves its share


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _same(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def launch(kernel, x, shapes, over=None, expect=0):
    """One launch of osrl_<kernel> on the inputs ``x``; ``shapes``: name -> shape of every buffer the launch writes.
    Returns name -> array, after checking the guard tails and (``expect`` != 0) that a refused call wrote nothing."""
    from osrl_amd import _lib as L
    from osrl_amd.engine.core import StepState, cur_stream
    dev = _dev()
    p = dict(x, **(over or {}))
    args, outs, keep = [], {}, []
    for kind, name in LC.spec(kernel):
        if kind == "p":
            v = p.get(name)
            if name in shapes:
                n = int(np.prod(shapes[name]))
                init = np.full(n + GUARD, np.nan, np.float32)
                if v is not None:
                    init[:n] = np.asarray(v, np.float32).ravel()
                buf = torch.from_numpy(init.copy()).to(dev)
                outs[name] = (buf, n, init)
                args.append(buf.data_ptr())
            elif v is None:
                args.append(None)
            else:
                t = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev)
                keep.append(t)
                args.append(t.data_ptr())
        elif kind == "st":
            st = StepState(dev, ["s"])
            for _ in range(p["step"]):
                st.tick()
            keep.append(st)
            args.append(st.ptr)
        else:
            args.append(float(p[name]) if kind == "f" else int(p[name]))
    rc = getattr(L.load(), "osrl_" + kernel)(*args, cur_stream())
    torch.cuda.synchronize()
    assert rc == expect, (kernel, over, rc)
    got = {}
    for name, (buf, n, init) in outs.items():
        a = buf.cpu().numpy()
        assert np.isnan(a[n:]).all(), f"{kernel}: {name} written past its end"
        if expect != 0:
            assert _same(a, init), f"{kernel}: refused call wrote {name}"
        got[name] = (a[:n].reshape(shapes[name]), init[:n].reshape(shapes[name]))
    return got


def check(kernel, x, tag):
    r64, r32 = LO.reference(kernel, x)
    got = launch(kernel, x, {k: v.shape for k, v in r64.out.items()})
    for name, v in r64.out.items():
        a, init = got[name]
        skip = np.isnan(v)
        assert _same(a[skip], init[skip]), f"{tag}: {name} written where the launch must leave it alone"
    worst, where = LO.compare({k: a for k, (a, _) in got.items()}, r64, r32)
    print(f"{tag}: worst |got - fp64| / gate = {worst:.3g} at {where}")
    assert worst <= 1.0, (tag, where, worst)
    return {k: a for k, (a, _) in got.items()}


def _cases(*kernels):
    return [c for c in LC.CASES if c.kernel in kernels]


def _run(c):
    check(c.kernel, LC.inputs(c), c.id)


@pytest.mark.parametrize("c", _cases("gauss_head", "gauss_head_bwd", "gauss_ood_sample"), ids=lambda c: c.id)
def test_gauss_head_kernels(c):
    _run(c)


@pytest.mark.parametrize("c", _cases("vae_latent", "vae_loss", "vae_loss_ws", "vae_latent_bwd", "vae_kl_rows"),
                         ids=lambda c: c.id)
def test_vae_tail_kernels(c):
    _run(c)


@pytest.mark.parametrize("c", _cases("cpq_critic_loss", "cpq_ood_mean", "cpq_actor_loss"), ids=lambda c: c.id)
def test_cpq_critic_actor_and_ood_mean_kernels(c):
    _run(c)


@pytest.mark.parametrize("c", _cases("cpq_cost_loss", "cpq_cost_loss_ood", "cpq_alpha_step"), ids=lambda c: c.id)
def test_cpq_cost_loss_modes_and_dual_step(c):
    _run(c)


@pytest.mark.parametrize("c", _cases("mse_loss", "clamp", "bcq_perturb", "bcq_perturb_bwd", "dice_perturb"),
                         ids=lambda c: c.id)
def test_mse_clamp_and_perturbation_kernels(c):
    _run(c)


@pytest.mark.parametrize("c", _cases("bcq_critic_loss", "bcq_critic_loss_ws", "bcq_actor_sums", "bcq_actor_loss"),
                         ids=lambda c: c.id)
def test_bcq_loss_kernels(c):
    _run(c)


@pytest.mark.parametrize("c", _cases("bear_actor_sums", "bear_actor_loss", "bear_head_bwd"), ids=lambda c: c.id)
def test_bear_loss_kernels(c):
    _run(c)


@pytest.mark.parametrize("c", _cases("dice_optimal_w", "dice_nu_step", "dice_chi_step", "dice_actor_loss"),
                         ids=lambda c: c.id)
def test_dice_loss_kernels(c):
    _run(c)


def test_every_entry_point_and_both_cpq_forms_are_in_the_table():
    assert {c.kernel for c in LC.CASES} == set(LC.SPECS)
    for kernel, keys in (("cpq_critic_loss", ("n_q_old", "n_qc_old", "n_q")), ("cpq_ood_mean", ("n_qc_old",)),
                         ("cpq_cost_loss", ("n_qc_old", "n_qc")), ("cpq_cost_loss_ood", ("n_qc_old", "n_qc", "n_qc_sampled")),
                         ("cpq_actor_loss", ("n_q", "n_qc"))):
        sizes = [tuple(LC.inputs(c)[k] for k in keys) for c in _cases(kernel)]
        assert any(max(s) <= 4 for s in sizes) and any(min(s) == 5 for s in sizes), kernel
        assert len(keys) == 1 or any(max(s) == 5 and min(s) < 5 for s in sizes), kernel  # one ensemble alone picks the form


MEANS = {"bcq_actor_loss": ("bcq_actor_sums", 2), "bear_actor_loss": ("bear_actor_sums", 3)}


@pytest.mark.parametrize("c", [c for c in LC.CASES if c.dp], ids=lambda c: c.id)
def test_two_ranks_reproduce_the_full_batch(c):
    """A 1025-row batch as 512 + 513 rows with rows_global = 1025 and stat_share = 0.5 (and the pre-pass means where the
    kernel takes them): every rank's per-row gradients are the full-batch reference's rows, the statistics add up to the
    full-batch reference's, every rank's state words are the full-batch reference's."""
    x = LC.inputs(c)
    r64, r32 = LO.reference(c.kernel, x)
    parts = [(0, LC.DP_SPLIT[0]), (LC.DP_SPLIT[0], LC.DP_SPLIT[1])]
    halves = [LC.split(x, r0, n, LC.DP_ROWS) for r0, n in parts]
    if c.kernel in MEANS:
        sums, k = MEANS[c.kernel]
        need = {name for _, name in LC.spec(sums)}
        means = np.zeros(k, np.float32)
        for y in halves:
            ys = {a: b for a, b in y.items() if a in need or a.startswith("_")}
            means = means + launch(sums, ys, {"out": (k,)})["out"][0]
        for y in halves:
            y["global_means"] = means
    merged, state = {}, []
    for y in halves:
        shapes = {}
        for name, v in r64.out.items():
            ax = x["_rows"].get(name)
            shapes[name] = v.shape if ax is None else v.shape[:ax] + (y.get("rows", y.get("n")),) + v.shape[ax + 1:]
        got = {k: a for k, (a, _) in launch(c.kernel, y, shapes).items()}
        st = {}
        for name, a in got.items():
            if name in x["_rows"]:
                merged[name] = a if name not in merged else np.concatenate([merged[name], a], x["_rows"][name])
            elif name in SUMMED:
                merged[name] = a.astype(np.float64) if name not in merged else merged[name] + a
            else:
                st[name] = a
        state.append(st)
    for k, st in enumerate(state):
        worst, where = LO.compare(dict(merged, **st), r64, r32)
        print(f"{c.id} rank {k}: worst |got - fp64| / gate = {worst:.3g} at {where}")
        assert worst <= 1.0, (c.id, k, where, worst)


def _refusal_base(kernel):
    if kernel == "dice_chi_step":
        return LC.BY_ID["dice_chi_step-B63-n1-step3"]
    return _cases(kernel)[0]


@pytest.mark.parametrize("kernel", sorted(LC.REFUSALS))
def test_argument_errors_are_refused_before_any_launch(kernel):
    x = LC.inputs(_refusal_base(kernel))
    shapes = {k: v.shape for k, v in LO.reference(kernel, x)[0].out.items()}
    for over in LC.REFUSALS[kernel]:
        over = {k: (np.zeros(over["rows_global"], np.float32) if isinstance(v, str) else v) for k, v in over.items()}
        launch(kernel, x, shapes, over=over, expect=-1)
