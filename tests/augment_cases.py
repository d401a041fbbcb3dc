"""Synthetic DSRL-shaped datasets for the Pareto augmentation tests (tests/golden/make_golden_augment.py,
tests/test_augment_oracle_cpu.py, tests/test_gpu_augment.py).

``make_augment_dataset``: ~2000 short trajectories whose (cost return, return) pairs sit in tight clusters (overfull
grid-filter bins, many samples sharing one nearest trajectory) over a sparse background (bins of 1..10 members).
``single_pf`` adds three identical trajectories that dominate everything: a Pareto set of one value.
``make_bc_frontier_dataset``: episodes whose Pareto set makes process_bc_dataset's r^2 rule stop at deg 0, 1 or 2.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

AUG_CLUSTERS = [(10.0, 120.0), (18.0, 260.0), (25.0, 300.0), (33.0, 410.0), (40.0, 380.0), (47.0, 520.0),
                (55.0, 500.0), (62.0, 590.0), (70.0, 560.0), (30.0, 150.0), (50.0, 260.0), (65.0, 400.0)]


def _episodes(targets: List[Tuple[float, float]], rs: np.random.RandomState, od: int, ad: int, max_len: int,
              tail: int = 5) -> Dict[str, np.ndarray]:
    """One episode per (cost return, return) target: length 1..max_len, the totals spread over the steps with a
    little noise; timeouts end the episodes (one in 5 a terminal), a short trailing partial episode."""
    f = np.float32
    rew, cost, term, tout = [], [], [], []
    for k, tg in enumerate(targets):
        c, r = tg[0], tg[1]
        L_ = int(rs.randint(1, max_len + 1))
        w = rs.uniform(0.5, 1.5, L_)
        wc = rs.uniform(0.5, 1.5, L_)
        if len(tg) > 2:  # an exact one-step episode
            L_, w, wc = 1, np.ones(1), np.ones(1)
        rew.append((r * w / w.sum()).astype(f))
        cost.append((c * wc / wc.sum()).astype(f))
        t = np.zeros(L_, f)
        o = np.zeros(L_, f)
        (t if k % 5 == 4 else o)[-1] = 1
        term.append(t)
        tout.append(o)
    rew.append(rs.uniform(0, 2, tail).astype(f))
    cost.append(np.zeros(tail, f))
    term.append(np.zeros(tail, f))
    tout.append(np.zeros(tail, f))
    rew, cost, term, tout = (np.concatenate(x) for x in (rew, cost, term, tout))
    n = rew.shape[0]
    return dict(observations=rs.randn(n, od).astype(f), next_observations=rs.randn(n, od).astype(f),
                actions=rs.uniform(-1, 1, (n, ad)).astype(f), rewards=rew, costs=cost, terminals=term, timeouts=tout)


def make_augment_dataset(seed: int = 0, n_traj: int = 2000, od: int = 3, ad: int = 2, max_len: int = 6,
                         single_pf: bool = False) -> Dict[str, np.ndarray]:
    rs = np.random.RandomState(1000 + seed)
    targets = []
    n_bg = n_traj // 6
    for _ in range(n_traj - n_bg):
        c, r = AUG_CLUSTERS[rs.randint(len(AUG_CLUSTERS))]
        targets.append((c + rs.uniform(-0.6, 0.6), r + rs.uniform(-3.0, 3.0)))
    for _ in range(n_bg):
        targets.append((rs.uniform(2.0, 78.0), rs.uniform(20.0, 640.0)))
    if single_pf:  # three identical one-step episodes at (0.4, 700) dominate every other point: the corner bin
        targets += [(0.4, 700.0, "exact")] * 3  # (the maximum always sits alone in bin ybins unless it is tied)
    order = rs.permutation(len(targets))
    return _episodes([targets[i] for i in order], rs, od, ad, max_len)


def make_bc_frontier_dataset(kind: str, seed: int = 0, n_ep: int = 400, od: int = 3, ad: int = 2,
                             max_len: int = 8) -> Dict[str, np.ndarray]:
    """Pareto set of the episode returns: "deg1" on a line (r^2 of deg 1 ~ 1), "deg2" on a parabola that a line
    fits badly, "deg0" a tied optimum: the Pareto set is three equal points, r^2 is 0/0 or x/0 at every degree (the
    mean fit's r^2 is 0 in exact arithmetic, so deg 0 is only ever kept through rounding) and the rule ends at deg 2
    on a rank-deficient fit."""
    rs = np.random.RandomState(2000 + seed)
    targets = []
    for _ in range(n_ep):
        c = rs.uniform(1.0, 60.0)
        if kind == "deg1":
            top = 50.0 + 8.0 * c
        elif kind == "deg2":
            top = 50.0 + 1.5e-4 * c ** 4
        else:
            top = 300.0
        targets.append((c, top - abs(rs.normal(0.0, 40.0))))
    if kind == "deg0":
        targets += [(0.5, 333.0, "exact")] * 3  # the tied optimum
    order = rs.permutation(len(targets))
    return _episodes([targets[i] for i in order], rs, od, ad, max_len, tail=0)  # frontier: complete episodes only


# the golden cases (tests/golden/make_golden_augment.py)
SEQ_CASES = {  # name: (augment_cases.make_augment_dataset kwargs, SequenceDataset kwargs)
    "d3_p20": (dict(seed=0), dict(deg=3, augment_percent=0.2)),
    "d0_p50": (dict(seed=1), dict(deg=0, augment_percent=0.5, max_rew_decrease=5.0, beta=2.0)),
    "d1_p20": (dict(seed=2), dict(deg=1, augment_percent=0.2, max_reward=800.0, min_reward=10.0)),
    "d2_p50": (dict(seed=3), dict(deg=2, augment_percent=0.5)),
    "d4_p20": (dict(seed=4), dict(deg=4, augment_percent=0.2, max_rew_decrease=20.0)),
    "single_pf": (dict(seed=5, single_pf=True), dict(deg=3, augment_percent=0.2)),
    "rand_aug": (dict(seed=6), dict(random_aug=0.2, aug_rmin=50, aug_rmax=650, aug_cmin=5, aug_cmax=75, cgap=5,
                                    rstd=1.0, cstd=0.2)),
    "pf_only": (dict(seed=7), dict(pf_only=True, augment_percent=0.2, random_aug=0.3)),
}
RNG_SEED = 1234
BC_KINDS = ("deg0", "deg1", "deg2")
BC_COST_LIMIT = 20.0
