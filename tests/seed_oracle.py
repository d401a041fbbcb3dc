"""fp64 references of the loss seeds of the backward launch (``osrl_mlp_seed_t``, include/osrl_amd.h), shared by
tests/test_seed_oracle_cpu.py and tests/test_gpu_seed_kernels.py.  TEST INFRASTRUCTURE ONLY: nothing here calls code
under ``osrl_amd/``.

Every kind is mapped onto the restatement tests/loss_oracle.py already holds for the loss kernel it replaces; only what
has no loss kernel is new (``ref_seed_fqe``, ``ref_seed_gauss_nll``: plain numpy from the formulas in the header).  A
reference takes the input dict of a ``seed_cases.SCase`` -- the loss oracle's names plus ``y`` [nets, rows, NL], the
planted outputs of the launch's nets -- and returns a ``loss_oracle.Ref`` with

* ``dz``     [nets, rows, NL]  dL/d(pre-activation of the output layer) = dL/dy * out_scale * act'(y / out_scale),
* ``stat``   [1] and, for FQE, ``stat2`` [1],
* ``aux["elem"]`` [nets, rows, NL] / ``aux["elem_kl"]`` [rows, L]: the per-element terms of the statistic's sums in the
  run's own precision, laid out as the launch meets them (``emulate_stat``).

Tables of ensemble members may hold one member more than the seed is told about (``n < shape[0]``): the launch must not
look at it; the ``member_n`` mutation does.

Tolerances are ``loss_oracle.compare``'s.  Composition with a tanh output keeps the class of dL/dy: 1 - t^2 with
t = y * (1 / out_scale) adds <= 6 half-ulps of 1 (two roundings in t, doubled by the square, one each for the square and
the difference) and two products, <= 10 half-ulps of ``scale`` in all with the <= 3 of dL/dy itself: inside "arith"'s 8
ulp = 16 half-ulps.
"""
from __future__ import annotations

import numpy as np

import loss_oracle as LO
from loss_oracle import Ref, _a, _mx, _on, _row_sum

KINDS = dict(MSE=1, CPQ_CRITIC=2, CPQ_COST=3, CPQ_ACTOR=4, GAUSS_HEAD=5, BCQ_CRITIC=6, FQE=7, GAUSS_NLL=8)  # the header's enum
# mutations of the oracle (tests/test_seed_oracle_cpu.py: "the gates are sharp"), through loss_oracle.mutate()
MUTATIONS = ("lt_strict", "tie_second", "no_done", "pad_row_again", "fqe_swap", "no_grad_at_2", "nll_one_sigmoid",
             "member_n")


def _cut(q, n):
    """The n members the seed is told about (one more under ``member_n``, where the table holds one)."""
    q = np.asarray(q)
    return q[: n + 1] if (_on("member_n") and q.shape[0] > n) else q[:n]


def _pad_again(x, dt, stat, terms, inv):
    """``pad_row_again``: the rows a ragged last tile pads with re-read the last row and count it once more each."""
    if _on("pad_row_again"):
        bm = x.get("_BM", 16)
        return stat + dt((-terms.shape[0]) % bm) * terms[-1] * inv
    return stat


def _members(r: Ref, x, dt, name="dq"):
    """[n, rows] member gradients of a loss-kernel reference -> ``dy`` [n, rows, 1]; per-element terms from d = dq / 2 inv."""
    inv = LO._inv(x, dt, r.out[name].shape[1])
    dq = r.out.pop(name)
    r.put("dy", dq[..., None], r.cls.pop(name), r.scale.pop(name)[..., None], route=name in r.route)
    r.route.discard(name)
    d = dq / (dt(2.0) * inv)
    r.aux["elem"] = (d * d)[..., None]
    r.out["stat"] = np.array([_pad_again(x, dt, r.out["stat"][0], r.terms["stat"], inv)])
    return r


def ref_seed_cpq_critic(x, dt):
    xx = dict(x, q_old=_cut(x["q_old"], x["n_q_old"]), qc_old=_cut(x["qc_old"], x["n_qc_old"]), q=x["y"][..., 0])
    return _members(LO.ref_cpq_critic_loss(xx, dt), x, dt)


def ref_seed_cpq_cost(x, dt):
    xx = dict(x, qc_old_next=_cut(x["qc_old_next"], x["n_qc_old"]), qc=x["y"][..., 0], ood_mean=None, qc_sampled=None)
    r = LO.ref_cpq_cost_loss(xx, dt)
    r.out["stat"] = r.out["stat"][:1]  # (the dual step stays with osrl_cpq_alpha_step)
    return _members(r, x, dt)


def ref_seed_cpq_actor(x, dt):
    xx = dict(x, q=x["y"][..., 0], qc=_cut(x["qc"], x["n_qc"]))
    r = LO.ref_cpq_actor_loss(xx, dt)
    inv = LO._inv(x, dt, xx["q"].shape[1])
    dq = r.out.pop("dq")
    r.put("dy", dq[..., None], r.cls.pop("dq"), r.scale.pop("dq")[..., None], route=True)
    r.route.discard("dq")
    el = np.zeros(dq.shape + (1,), dt)
    el[0, :, 0] = r.terms["stat"]  # (net 0's tiles carry the statistic)
    r.aux["elem"] = el
    r.out["stat"] = np.array([_pad_again(x, dt, r.out["stat"][0], r.terms["stat"], inv)])
    return r


def ref_seed_bcq_critic(x, dt):
    return _members(LO.ref_bcq_critic_loss(dict(x, q_on=x["y"][..., 0]), dt), x, dt)


def ref_seed_gauss_head(x, dt):
    xx = dict(x, head=x["y"][0], da_nets=_cut(x["da_nets"], x["n_nets"]))
    r = LO.ref_gauss_head_bwd(xx, dt)
    r.put("dy", r.out.pop("dhead")[None], r.cls.pop("dhead"), r.scale.pop("dhead")[None])
    return r


def ref_seed_mse(x, dt):
    """OSRL_SEED_MSE: with ``head`` the VAE loss (ref_vae_loss, u = net 0's output; a further net of the launch adds its
    reconstruction term, the KL term is counted once), without it ref_mse_loss on the flattened outputs."""
    y = _a(x, "y", dt)
    E, rows, NL = y.shape
    r = Ref()
    dys, scs, terms, elem = [], [], None, []
    if x.get("head") is not None:
        inv = LO._inv(x, dt, rows)
        for e in range(E):
            o = LO.ref_vae_loss(dict(x, u=x["y"][e], beta=x["beta"] if e == 0 else 0.0), dt)
            dys.append(o.out["du"])
            scs.append(o.scale["du"])
            terms = o.terms["stat"] if e == 0 else terms + o.terms["stat"]
            d = y[e] - _a(x, "act", dt)
            elem.append(d * d)
            if e == 0:
                r.kink.update(o.kink)
        r.aux["elem_kl"] = LO._kl_elem(_a(x, "head", dt)[:, :x["L"]], _a(x, "head", dt)[:, x["L"]:], dt)
        cls = "tstat"
    else:
        xg = dict(n_global=x.get("n_global", 0))
        inv = dt(1.0) / dt(xg["n_global"] if xg["n_global"] > 0 else rows * NL)
        for e in range(E):
            o = LO.ref_mse_loss(dict(xg, u=x["y"][e].reshape(-1), target=np.asarray(x["target"]).reshape(-1)), dt)
            dys.append(o.out["du"].reshape(rows, NL))
            scs.append(o.scale["du"].reshape(rows, NL))
            t = o.terms["stat"].reshape(rows, NL).sum(1, dtype=dt)
            terms = t if e == 0 else terms + t
            elem.append(o.terms["stat"].reshape(rows, NL))
        cls = "astat"
    r.put("dy", np.stack(dys), "arith", np.stack(scs))
    r.put("stat", np.array([_pad_again(x, dt, _row_sum(terms) * inv, terms, inv)]), cls)
    r.terms["stat"] = terms
    r.aux["elem"] = np.stack(elem)
    return r


def ref_seed_fqe(x, dt):
    """Net e < n_r regresses on rew + gamma (1 - done) q_t[e], net e >= n_r on cost + gamma (1 - done) q_t[e]; dy_e =
    2 (y_e - backup_e) / rows; stat = sum over the reward nets of the batch-mean squared error, stat2 over the cost nets."""
    r = Ref()
    y, q_t = _a(x, "y", dt)[..., 0], _a(x, "q_t", dt)
    rew, cost, done = _a(x, "rew", dt), _a(x, "cost", dt), _a(x, "done", dt)
    n_r = x["n_r"]
    rows = rew.shape[0]
    inv = dt(1.0) / dt(rows)
    nd = dt(1.0) if _on("no_done") else dt(1.0) - done
    base = np.stack([rew] * n_r + [cost] * (y.shape[0] - n_r))
    boot = dt(x["gamma"]) * nd[None] * q_t
    backup = base + boot
    d = y - backup
    r.put("dy", (dt(2.0) * d * inv)[..., None], "arith", (_mx(y, backup, base, boot) * 2 * float(inv))[..., None])
    tr, tc = (d[:n_r] * d[:n_r]).sum(0, dtype=dt), (d[n_r:] * d[n_r:]).sum(0, dtype=dt)
    sr, sc = _pad_again(x, dt, _row_sum(tr) * inv, tr, inv), _pad_again(x, dt, _row_sum(tc) * inv, tc, inv)
    if _on("fqe_swap"):
        sr, sc = sc, sr
    r.put("stat", np.array([sr]), "astat")
    r.put("stat2", np.array([sc]), "astat")
    r.terms["stat"], r.terms["stat2"] = tr, tc
    r.aux["elem"] = (d * d)[..., None]
    return r


def _softplus(z):
    return np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))


def _sigmoid(z, dt):
    with np.errstate(over="ignore"):
        return dt(1.0) / (dt(1.0) + np.exp(-z))


def ref_seed_gauss_nll(x, dt):
    """Every net's output row is (od + 1 means | raw cost | od + 1 raw log-variances); lv = lo + softplus(hi -
    softplus(hi - raw) - lo); loss = mean over (rows, od + 2) of (y - t)^2 exp(-lv) + lv on the mean columns and of
    (y - t)^2 on the cost column, summed over the nets."""
    r = Ref()
    y, t = _a(x, "y", dt), _a(x, "target", dt)
    E, rows, NL = y.shape
    no = (NL + 1) // 2
    lo, hi = dt(x["lo"]), dt(x["hi"])
    inv = dt(1.0) / dt(rows * no)
    raw = y[..., no:]
    lv1 = hi - _softplus(hi - raw)
    lv = lo + _softplus(lv1 - lo)
    d = y[..., :no - 1] - t[None, :, :no - 1]
    dc = y[..., no - 1] - t[None, :, no - 1]
    with np.errstate(over="ignore"):
        iv = np.exp(-lv)
    s1 = _sigmoid(hi - raw, dt)
    s2 = dt(1.0) if _on("nll_one_sigmoid") else _sigmoid(lv1 - lo, dt)
    dmean = dt(2.0) * d * iv * inv
    draw = (dt(1.0) - d * d * iv) * s1 * s2 * inv
    dcost = dt(2.0) * dc * inv
    s_mean = _mx(y[..., :no - 1], np.broadcast_to(t[None, :, :no - 1], d.shape)) * 2 * iv * float(inv)
    s_raw = (1 + d * d * iv) * float(inv)
    s_cost = _mx(y[..., no - 1], np.broadcast_to(t[None, :, no - 1], dc.shape)) * 2 * float(inv)
    r.put("dy", np.concatenate([dmean, dcost[..., None], draw], 2), "trans",
          np.concatenate([s_mean, s_cost[..., None], s_raw], 2))
    el = np.concatenate([d * d * iv + lv, (dc * dc)[..., None], np.zeros_like(raw)], 2)
    terms = el.sum((0, 2), dtype=dt) / dt(no)
    inv_r = dt(1.0) / dt(rows)
    r.put("stat", np.array([_pad_again(x, dt, _row_sum(terms) * inv_r, terms, inv_r)]), "tstat")
    r.terms["stat"] = terms
    r.aux["elem"] = el
    return r


REFS = dict(MSE=ref_seed_mse, CPQ_CRITIC=ref_seed_cpq_critic, CPQ_COST=ref_seed_cpq_cost, CPQ_ACTOR=ref_seed_cpq_actor,
            GAUSS_HEAD=ref_seed_gauss_head, BCQ_CRITIC=ref_seed_bcq_critic, FQE=ref_seed_fqe, GAUSS_NLL=ref_seed_gauss_nll)


def _compose(r: Ref, x, dt):
    """dz = dy * out_scale * act'(y / out_scale), in the launch's order (module docstring)."""
    act, osc = x.get("_act", "id"), dt(x.get("_out_scale", 1.0))
    dy = r.out.pop("dy")
    cls, sc, route = r.cls.pop("dy"), r.scale.pop("dy"), "dy" in r.route
    r.route.discard("dy")
    v = dy * osc
    if act == "tanh":
        t = _a(x, "y", dt) * (dt(1.0) / osc)
        v = v * (dt(1.0) - t * t)
    elif act != "id":
        raise ValueError(act)
    r.put("dz", v, cls, sc * abs(float(osc)), route=route)
    return r


# The seeded statistic's gate, relative to the scale the loss oracle gives the statistic (max(1, mean|term|)): 10 x the
# worst error of ``emulate_stat`` -- the launch's own summation order on the fp32 terms -- against fp64 over the case
# table, per class (tests/test_seed_oracle_cpu.py measures it and holds these figures to it).  The loss kernels' gates
# (2e-6 "astat"; "tstat" from 4.8e-7 up) are sized for THEIR order and the emulation reaches 0.11 / 0.27 of them, more
# than the tenth that would let them stand.  Never sized from a GPU's output.
SEED_STAT_GATE = dict(astat=2.21e-6, tstat=2.99e-6)


def _both(fn, x):
    r64, r32 = _compose(fn(x, np.float64), x, np.float64), _compose(fn(x, np.float32), x, np.float32)
    parts = LO.gate_parts(r64, r32)
    for name in ("stat", "stat2"):
        if name in r64.out:
            r64.gate[name] = SEED_STAT_GATE[r64.cls[name]] * parts[name][1]
    return r64, r32


def reference(kind: str, x, mutation=None):
    """(fp64 Ref, honest-fp32 Ref) of one case's inputs."""
    fn = REFS[kind]
    with np.errstate(all="ignore"):
        if mutation is None:
            return _both(fn, x)
        with LO.mutate(mutation):
            return _both(fn, x)


# ---- the launch's reduction order, for sizing the statistic's gate (tests/test_seed_oracle_cpu.py) ----------------------
def _r16(n):
    return (n + 15) // 16 * 16


def _butterfly(v):
    """Six __shfl_xor steps over the last axis (64 lanes); lane 0's value."""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., idx ^ o]).astype(np.float32)
    return v[..., 0]


def _wg_sum(lanes, nw):
    """[..., 64 nw] per-lane sums -> butterfly per wave, waves in order."""
    w = _butterfly(lanes.reshape(lanes.shape[:-1] + (nw, 64)))
    t = np.zeros(w.shape[:-1], np.float32)
    for k in range(nw):
        t = (t + w[..., k]).astype(np.float32)
    return t


def _strided(v, T):
    """[..., n] elements met by T lanes at stride T -> [..., T] sequential fp32 sums."""
    n = v.shape[-1]
    k = (n + T - 1) // T
    p = np.zeros(v.shape[:-1] + (k * T,), np.float32)
    p[..., :n] = v
    p = p.reshape(v.shape[:-1] + (k, T))
    acc = np.zeros(v.shape[:-1] + (T,), np.float32)
    for i in range(k):
        acc = (acc + p[..., i, :]).astype(np.float32)
    return acc


def _tiles(el, bm, width):
    """[..., rows, cols] -> [..., tiles, bm * width]: the (row, column) walk of one tile, padding contributes 0."""
    rows, cols = el.shape[-2:]
    tiles = (rows + bm - 1) // bm
    p = np.zeros(el.shape[:-2] + (tiles * bm, width), np.float32)
    p[..., :rows, :cols] = el
    return p.reshape(el.shape[:-2] + (tiles, bm * width))


def emulate_stat(r32: Ref, bm: int, nw: int, fqe_n_r=None, stat_scale=1.0, stat_scale2=0.0, kl_beta=0.0):
    """The seeded launch's statistic(s) from the fp32 per-element terms, in its order: strided per-lane sums over the
    tile's (row, padded column) walk, six butterfly steps, waves in order -> the tile's partials; the last workgroup's
    lanes each sum a contiguous chunk of ceil(n / lanes) partials, butterfly, waves in order."""
    el = np.asarray(r32.aux["elem"], np.float32)
    E = el.shape[0]
    T = 64 * nw
    p0 = _wg_sum(_strided(_tiles(el, bm, _r16(el.shape[2])), T), nw)  # [E, tiles]
    p1 = np.zeros_like(p0)
    if fqe_n_r is not None:
        p1[fqe_n_r:], p0[fqe_n_r:] = p0[fqe_n_r:], 0
    if "elem_kl" in r32.aux:
        kl = np.asarray(r32.aux["elem_kl"], np.float32)
        p1[0] = _wg_sum(_strided(_tiles(kl, bm, kl.shape[1]), T), nw)
    n = p0.size
    per = (n + T - 1) // T
    out = []
    for p in (p0, p1):
        q = np.zeros(per * T, np.float32)
        q[:n] = p.reshape(-1)
        lanes = np.zeros(T, np.float32)
        for i in range(per):
            lanes = (lanes + q.reshape(T, per)[:, i]).astype(np.float32)
        out.append(_wg_sum(lanes, nw))
    u0, u1 = out
    f = np.float32
    if fqe_n_r is not None:
        return f(u0 * f(stat_scale)), f(u1 * f(stat_scale))
    return f(f(u0 * f(stat_scale)) + f(f(kl_beta) * f(u1 * f(stat_scale2)))), None


def stat_args(kind: str, x) -> dict:
    """The statistic's scale factors as the engines' seed builders set them (fp32), for ``emulate_stat``."""
    f = np.float32
    E, rows, NL = np.asarray(x["y"]).shape
    g = x.get("rows_global", 0)
    inv = f(1.0) / f(g if g > 0 else rows)
    if kind == "MSE" and x.get("head") is not None:
        return dict(stat_scale=inv / f(NL), stat_scale2=inv / f(x["L"]), kl_beta=f(x["beta"]))
    if kind == "MSE":
        ng = x.get("n_global", 0)
        return dict(stat_scale=f(1.0) / f(ng if ng > 0 else rows * NL))
    if kind == "GAUSS_NLL":
        return dict(stat_scale=f(1.0) / f(rows * ((NL + 1) // 2)))
    if kind == "FQE":
        return dict(stat_scale=f(1.0) / f(rows), fqe_n_r=x["n_r"])
    return dict(stat_scale=inv)
