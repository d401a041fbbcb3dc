"""One table of cases for the loss seeds of the backward launch (``osrl_mlp_seed_t``), shared by
tests/test_seed_oracle_cpu.py and tests/test_gpu_seed_kernels.py.

Two axes.  SHAPES: the smallest nets / row counts that reach every instantiation of the backward kernel a seed can run in
(``TILE_SHAPES``), every kind on each.  EDGES: what a random batch never lands on, per kind, on the 4-wave 16-row tile at
63 / 257 rows -- planted with the helpers of tests/loss_cases.py (``_tie``, ``_plant_thres``, ``_big``, ``picks``).

A case's ``build()`` returns the loss oracle's input dict of the kind plus ``y`` [nets, rows, NL] (the planted outputs of
the launch's nets), ``_act`` / ``_out_scale`` (the output activation), ``_BM`` (the tile's rows: the ``pad_row_again``
mutation), ``_plant`` (rows planted exactly ON a switch point), ``_near`` (rows planted one ulp beside one).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Tuple

import numpy as np

import loss_cases as LC
from loss_cases import F, Gen, Q_THRES, _big, _plant_thres, _tie, picks

ROWS1 = (1, 15, 16, 17, 63, 257)  # around one tile, four tiles minus a row, 16 tiles and a row
KIND_IDS = ("MSE_KL", "MSE", "CPQ_CRITIC", "CPQ_COST", "CPQ_ACTOR", "GAUSS_HEAD", "BCQ_CRITIC", "FQE", "GAUSS_NLL")


def tile_choice(dims, nets, rows, tile_rows=0, extra=0) -> Tuple:
    """A restatement of the library's tile choice (csrc/mlp.hip ``choose_tile``): (row blocks, column blocks per wave,
    waves), with "wide" in front for a net the per-layer path takes (its seed stage runs on the one-layer sub-net
    [NL, NL]).  A COVERAGE AID for the CPU test that the table reaches every instantiation it lists -- not a check of
    the library: if the library's choice moves, a GPU test still runs the kernel the library picks."""
    if max(dims) > 448:
        return ("wide",) + tile_choice([dims[-1], dims[-1]], nets, rows)
    maxw = max(max(dims), extra)
    nblk = (maxw + 15) // 16
    cpw = (nblk + 3) // 4
    ncb = 1 if cpw <= 1 else 2 if cpw <= 2 else 4 if cpw <= 4 else 7
    lda = (maxw + 15) // 16 * 16 + 8
    nrb = 2 if (ncb != 7 and ((rows + 31) // 32) * nets >= 1024) else 1
    if tile_rows in (16, 32) or (tile_rows == 64 and ncb != 7):
        return (tile_rows // 16, ncb, 4)
    if nrb == 1 and cpw > 2 and ((rows + 15) // 16) * nets <= 512 and lda >= 128:
        return (1, 2 if (nblk + 7) // 8 <= 2 else 4, 8)
    return (nrb, ncb, 4)


# (hidden dims, nets or None = the kind's own, rows or None = the case's, tile_rows, the instantiation it is there for)
TILE_SHAPES = (
    ([5, 32], None, None, 0, (1, 1, 4)),
    ([7, 96], None, None, 0, (1, 2, 4)),
    ([9, 200], None, None, 0, (1, 2, 8)),
    ([9, 300], None, None, 0, (1, 4, 8)),
    ([9, 200], 2, 4117, 0, (1, 4, 4)),   # 516 partials: three per lane in the last workgroup's sum
    ([9, 300], 2, 4117, 0, (1, 7, 4)),
    ([5, 32], None, 70, 32, (2, 1, 4)),
    ([5, 32], None, 70, 64, (4, 1, 4)),
    ([9, 512], None, None, 0, ("wide", 1, 1, 4)),
)


@dataclass
class SCase:
    kind: str            # a key of seed_oracle.REFS
    tag: str
    dims: List[int]      # the net without its output width
    tile_rows: int
    build: Callable[[], dict]
    nostat: bool = False  # also launched without the statistic (stat NULL; FQE: stat2 NULL)

    @property
    def id(self):
        return f"{self.kind}-{self.tag}"


def _decoy(q, n, by=3.0):
    """One member more than the seed is told about, below every minimum (the launch must not look at it)."""
    return np.concatenate([q, q.min(0, keepdims=True) - F(by)], 0) if n < 4 else q


def _ulp_rows(qc, x, rows_at):
    """min qc one ulp above / below the threshold (mask off / on)."""
    for r, up in zip(rows_at, (True, False)):
        _plant_thres(qc, r)
        qc[0, r] = np.nextafter(F(Q_THRES), F(np.inf if up else -np.inf))
        x["_near"].append(r)


def s_cpq_critic(rows, n_a, n_b, E, seed, edge=()):
    def f():
        x = LC.b_cpq_critic(rows, n_a, n_b, E, seed)()
        x["_near"] = []
        if rows >= 40:
            P = picks(rows)
            if "ulp" in edge:
                _ulp_rows(x["qc_old"], x, (P[8], P[9]))
                x["done"][[P[8], P[9]]] = 0
            if "big" in edge:  # the bootstrap masked out, the backup 1e4 among rows of order 1
                x["rew"][P[10]], x["done"][P[10]] = F(1e4), 0
                x["qc_old"][:, P[10]] = F(Q_THRES + 1.0)
        if "done" in edge:
            x["done"][:] = 1
        if "gamma0" in edge:
            x["gamma"] = 0.0
        x["q_old"], x["qc_old"] = _decoy(x["q_old"], n_a), _decoy(x["qc_old"], n_b)
        x["y"] = x.pop("q")[:, :, None].copy()
        return x
    return f


def s_cpq_cost(rows, n_a, E, seed, edge=()):
    def f():
        x = LC.b_cpq_cost(rows, n_a, E, seed, "deferred")()
        if "gamma0" in edge:
            x["gamma"] = 0.0
        x["qc_old_next"] = _decoy(x["qc_old_next"], n_a)
        x["y"] = x.pop("qc")[:, :, None].copy()
        return x
    return f


def s_cpq_actor(rows, n_q, n_qc, seed, edge=()):
    def f():
        x = LC.b_cpq_actor(rows, n_q, n_qc, seed)()
        x["_near"] = []
        if rows >= 40:
            P = picks(rows)
            if "ties" in edge:  # members 0 and 2, and the last two: the gradient goes to the first
                _tie(x["q"], P[7], members=(0, 2))
                _tie(x["q"], P[8], members=(n_q - 2, n_q - 1))
                x["qc"][:, [P[7], P[8]]] = F(-1.0)
            if "ulp" in edge:
                _ulp_rows(x["qc"], x, (P[9], P[10]))
        x["qc"] = _decoy(x["qc"], n_qc)
        x["y"] = x.pop("q")[:, :, None].copy()
        return x
    return f


def s_bcq_critic(rows, n1, n2, ns, E, seed, done=True, lmbda=0.75, edge=()):
    def f():
        x = LC.b_bcq_critic(rows, n1, n2, ns, E, seed, done=done)()
        x["lmbda"] = lmbda
        if rows >= 40 and "alleq" in edge:  # every sample of a row the same, member by member
            r = picks(rows)[5]
            x["q_t"][:, r, :] = x["q_t"][:, r, :1]
        x["y"] = x.pop("q_on")[:, :, None].copy()
        return x
    return f


def s_gauss_head(rows, ad, n, seed, edge=(), max_action=1.5):
    def f():
        x = LC.b_gauss_head_bwd(rows, ad, n, seed)()
        x["max_action"] = max_action
        x["_near"] = []
        if rows >= 40 and "ulp" in edge:  # one ulp inside and outside each clamp edge
            P = picks(rows)
            for k, (v, to) in enumerate(((-20.0, 0.0), (-20.0, -40.0), (2.0, 0.0), (2.0, 4.0))):
                x["head"][P[8 + k], ad + k % ad] = np.nextafter(F(v), F(to))
                x["_near"].append(P[8 + k])
        x["da_nets"] = _decoy(x["da_nets"], n, by=-5.0)
        x["y"] = x.pop("head")[None].copy()
        return x
    return f


def s_vae(rows, ad, Lz, E, seed, edge=()):
    def f():
        x = LC.b_vae_loss(rows, ad, Lz, seed)()
        g = Gen(seed + 2000)
        y = np.stack([x.pop("u")] + [g.n(rows, ad) for _ in range(E - 1)])
        if "tanh" in edge:  # a tanh output of scale 1.5, saturated on planted elements: the derivative is exactly 0
            y = (F(1.5) * np.tanh(y)).astype(F)
            x["act"] = (F(1.5) * np.tanh(x["act"])).astype(F)
            for k, r in enumerate(picks(rows)[:4]):
                y[0, r, k % ad] = F(1.5 if k % 2 == 0 else -1.5)
            x["_act"], x["_out_scale"] = "tanh", 1.5
        if "rg" in edge:
            x["rows_global"] = 2 * rows + 3
        if "hi" in edge:  # the upper clamp edge and beyond it (exp(15)^2: the statistic is that row's KL)
            x["head"][0, Lz], x["head"][min(1, rows - 1), 2 * Lz - 1] = F(15.0), F(15.5)
        x["y"] = y
        return x
    return f


def s_mse(rows, NL, E, seed, n_global=0):
    def f():
        g = Gen(seed)
        x = dict(y=g.n(E, rows, NL), target=g.n(rows, NL), n_global=n_global, rows=rows)
        _big(x["y"][0, :, 0], rows)
        return x
    return f


def s_fqe(rows, n_r, n_c, seed, edge=()):
    def f():
        g = Gen(seed)
        E = n_r + n_c
        x = dict(y=g.n(E, rows, 1), q_t=g.n(E, rows), rew=g.n(rows), cost=g.flag(0.3, rows), done=g.flag(0.25, rows),
                 n_r=n_r, n_c=n_c, gamma=0.99, rows=rows)
        _big(x["rew"], rows)
        if rows >= 40:
            P = picks(rows)
            x["done"][P[2]], x["done"][P[3]] = 1, 0
        if "scales" in edge:  # the cost nets 100 x off: a swap of the two statistics misses its gate by far
            x["y"][n_r:] *= F(100.0)
        if "done" in edge:
            x["done"][:] = 1
        return x
    return f


NLL_LO, NLL_HI = -10.0, 0.5


def s_gauss_nll(rows, od, E, seed, edge=()):
    def f():
        g = Gen(seed)
        no = od + 2
        x = dict(y=g.n(E, rows, 2 * od + 3), target=g.n(rows, no), lo=NLL_LO, hi=NLL_HI, rows=rows)
        x["y"][..., no:] = g.rs.uniform(NLL_LO - 2.0, NLL_HI + 2.0, (E, rows, od + 1)).astype(F)
        if rows >= 15:  # raw log-variance far outside / exactly on its bounds: the sigmoid factors vanish or are 0.5
            for r, v in enumerate((NLL_HI + 40.0, NLL_LO - 40.0, NLL_HI, NLL_LO)):
                x["y"][:, r, no + r % (od + 1)] = F(v)
            x["y"][0, 4, :od + 1] = x["target"][4, :od + 1]  # residual 0
            x["y"][0, 4, od + 1] = x["target"][4, od + 1]
            if "big" in edge:  # residual 1e3 under the smallest variance
                x["y"][0, 5, 0], x["y"][0, 5, no] = x["target"][5, 0] + F(1e3), F(NLL_LO)
        return x
    return f


def _builder(kind, rows, i, seed, E=None):
    """The kind's case at ``rows``; ``i`` walks the ensemble sizes."""
    n3 = ((1, 1, 1), (3, 4, 2), (4, 3, 8), (1, 3, 2), (3, 1, 1), (4, 4, 2))[i % 6]
    if kind == "MSE_KL":
        ad, Lz = ((1, 1), (3, 6), (17, 3), (3, 5), (1, 6), (17, 6))[i % 6]
        return "MSE", f"kl-ad{ad}-L{Lz}", s_vae(rows, ad, Lz, E or 1, seed)
    if kind == "MSE":
        NL, n = ((1, 1), (3, 2), (17, 1), (3, 3), (1, 8), (17, 2))[i % 6]
        return "MSE", f"NL{NL}", s_mse(rows, NL, E or n, seed)
    if kind == "CPQ_CRITIC":
        return kind, f"n{n3[0]}{n3[1]}", s_cpq_critic(rows, n3[0], n3[1], E or n3[2], seed)
    if kind == "CPQ_COST":
        n = (1, 4, 3, 2, 4, 1)[i % 6]
        return kind, f"n{n}", s_cpq_cost(rows, n, E or n3[2], seed)
    if kind == "CPQ_ACTOR":
        return kind, f"n{n3[0]}{n3[1]}", s_cpq_actor(rows, n3[0], n3[1], seed)
    if kind == "GAUSS_HEAD":
        ad, n = ((1, 1), (3, 4), (8, 3), (3, 1), (8, 4), (1, 3))[i % 6]
        return kind, f"ad{ad}-n{n}", s_gauss_head(rows, ad, n, seed)
    if kind == "BCQ_CRITIC":
        n1, n2, ns, done = ((1, 1, 1, True), (2, 5, 10, False), (5, 2, 10, True), (2, 2, 1, False), (1, 5, 10, True),
                            (5, 1, 1, True))[i % 6]
        return kind, f"n{n1}{n2}-s{ns}" + ("" if done else "-nodone"), s_bcq_critic(rows, n1, n2, ns, E or n3[2], seed, done)
    if kind == "FQE":
        n_r, n_c = ((1, 1), (2, 1), (1, 3), (4, 4), (1, 1), (2, 1))[i % 6] if E is None else (E // 2, E - E // 2)
        return kind, f"n{n_r}{n_c}", s_fqe(rows, n_r, n_c, seed)
    if kind == "GAUSS_NLL":
        od, n = ((1, 1), (3, 2), (11, 1), (3, 1), (1, 2), (11, 2))[i % 6]
        return kind, f"od{od}", s_gauss_nll(rows, od, E or n, seed)
    raise KeyError(kind)


# default seed (5000 + the case's position) -> the seed used instead: the default left an unplanted row within 1e-4 of a
# switch point (tests/test_seed_oracle_cpu.py::test_planted_rows_sit_on_their_kink_and_no_other_row_near_one)
SEED_BUMP: dict = {5094: 6094}


def _table() -> List[SCase]:
    T: List[SCase] = []
    seed = [5000]

    def add(kind, tag, dims, tile_rows, build, nostat=False):
        T.append(SCase(kind, tag, dims, tile_rows, build, nostat))

    def nxt():
        seed[0] += 1
        return SEED_BUMP.get(seed[0], seed[0])
    # ---- every kind on the 4-wave 16-row tile at every row count
    for k in KIND_IDS:
        for i, rows in enumerate(ROWS1):
            kind, tag, b = _builder(k, rows, i, nxt())
            add(kind, f"{tag}-r{rows}", [5, 32], 0, b, nostat=rows == 17)
    # ---- every kind on the other default tiles (two 4-wave column splits, both 8-wave forms) and on the wide path
    for dims, rows in (([7, 96], 37), ([9, 200], 50), ([9, 300], 33), ([9, 512], 21)):
        for j, k in enumerate(KIND_IDS):
            kind, tag, b = _builder(k, rows, j + dims[1], nxt())
            add(kind, f"{tag}-h{dims[1]}-r{rows}", dims, 0, b)
    # ---- the statistic's reduction: > 256 partials, 32- and 64-row tiles (ragged: 70 rows)
    for dims, E, rows, tr, _ in TILE_SHAPES:
        if rows is None:
            continue
        for k in ("CPQ_CRITIC", "MSE_KL", "FQE"):
            kind, tag, b = _builder(k, rows, 1, nxt(), E=E or 2)
            add(kind, f"{tag}-h{dims[1]}-r{rows}" + (f"-t{tr}" if tr else ""), dims, tr, b)
    # ---- edges (63 / 257 rows: the planted rows exist from 40 rows on)
    D = [5, 32]
    for n_a, n_b, E, rows in ((1, 1, 1, 63), (3, 4, 2, 257), (4, 3, 8, 63)):
        add("CPQ_CRITIC", f"ulp-big-n{n_a}{n_b}-e{E}-r{rows}", D, 0, s_cpq_critic(rows, n_a, n_b, E, nxt(), ("ulp", "big")))
    add("CPQ_CRITIC", "all_done-r63", D, 0, s_cpq_critic(63, 3, 3, 2, nxt(), ("done",)))
    add("CPQ_CRITIC", "gamma0-r63", D, 0, s_cpq_critic(63, 4, 1, 2, nxt(), ("gamma0",)))
    for n_q, n_qc, rows in ((3, 1, 63), (4, 3, 257), (3, 4, 257)):
        add("CPQ_ACTOR", f"ties-ulp-n{n_q}{n_qc}-r{rows}", D, 0, s_cpq_actor(rows, n_q, n_qc, nxt(), ("ties", "ulp")))
    add("CPQ_ACTOR", "ulp-n11-r63", D, 0, s_cpq_actor(63, 1, 1, nxt(), ("ulp",)))
    for n in (1, 4):
        add("CPQ_COST", f"gamma0-n{n}-r63", D, 0, s_cpq_cost(63, n, 2, nxt(), ("gamma0",)))
        add("CPQ_COST", f"ties-n{n}-r257", D, 0, s_cpq_cost(257, n, 1, nxt()))
    for lm in (0.0, 0.75, 1.0):
        add("BCQ_CRITIC", f"lmbda{lm}-alleq-r63", D, 0, s_bcq_critic(63, 2, 2, 10, 2, nxt(), True, lm, ("alleq",)))
    add("BCQ_CRITIC", "nodone-n15-s1-r257", D, 0, s_bcq_critic(257, 1, 5, 1, 1, nxt(), False, 0.75, ("alleq",)))
    for ad, n, rows in ((1, 1, 63), (3, 4, 257), (8, 4, 63)):
        add("GAUSS_HEAD", f"ulp-ad{ad}-n{n}-r{rows}", D, 0, s_gauss_head(rows, ad, n, nxt(), ("ulp",), max_action=2.5))
    for ad, Lz, rows in ((1, 5, 63), (3, 6, 257), (17, 3, 63)):
        add("MSE", f"kl-tanh-ad{ad}-L{Lz}-r{rows}", D, 0, s_vae(rows, ad, Lz, 1, nxt(), ("tanh",)))
    add("MSE", "kl-rows_global-r63", D, 0, s_vae(63, 3, 6, 1, nxt(), ("rg",)))
    add("MSE", "kl-upper_edge-r17", D, 0, s_vae(17, 3, 6, 1, nxt(), ("hi",)))
    add("MSE", "n_global-NL3-r63", D, 0, s_mse(63, 3, 2, nxt(), n_global=2 * 63 * 3 + 5))
    for (n_r, n_c), rows in zip(((1, 1), (2, 1), (1, 3), (4, 4)), (63, 257, 63, 257)):
        add("FQE", f"scales-n{n_r}{n_c}-r{rows}", D, 0, s_fqe(rows, n_r, n_c, nxt(), ("scales",)), nostat=True)
    add("FQE", "all_done-n21-r63", D, 0, s_fqe(63, 2, 1, nxt(), ("done",)))
    for od, E in ((1, 2), (3, 1), (11, 2)):
        add("GAUSS_NLL", f"big-od{od}-e{E}-r63", D, 0, s_gauss_nll(63, od, E, nxt(), ("big",)))
    return T


CASES: List[SCase] = _table()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), [c.id for c in CASES if sum(d.id == c.id for d in CASES) > 1]


def shape(c: SCase, x=None):
    """(dims with the output width, nets, rows) of a case."""
    x = x if x is not None else c.build()
    E, rows, NL = x["y"].shape
    return c.dims + [NL], E, rows


def inputs(c: SCase) -> dict:
    x = c.build()
    dims, E, rows = shape(c, x)
    t = tile_choice(dims, E, rows, c.tile_rows)
    x["_tile"] = t
    x["_BM"] = 16 * t[-3]
    x.setdefault("_act", "id")
    x.setdefault("_out_scale", 1.0)
    x.setdefault("_plant", [])
    x.setdefault("_near", [])
    return x
