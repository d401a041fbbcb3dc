"""numpy restatement of the reference's Pareto augmentation (osrl/common/dataset.py:47-93, :186-396, :557-630) on
the flat trajectory tables of ``oracle.ingest_oracle`` / ``common.ingest.process_sequence_dataset``, with every
random draw taken from an injected array (the tests replay the reference's recorded stream or the device's own).

TEST INFRASTRUCTURE ONLY: nothing under ``osrl_amd/`` imports it.  Pinned by tests/golden/augment.npz
(tests/test_augment_oracle_cpu.py); the GPU tests compare the device against it at sizes the golden does not cover.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Optional

import numpy as np

KEYS = ("observations", "actions", "rewards", "costs", "returns", "cost_returns")


def first_returns(t: Dict[str, np.ndarray]):
    """(return, cost return) of every trajectory at its first step, widened to fp64."""
    s = np.asarray(t["traj_start"], np.int64)
    return np.asarray(t["returns"])[s].astype(np.float64), np.asarray(t["cost_returns"])[s].astype(np.float64)


def grid_filter(c, r, picks, xbins=10, ybins=50, max_per=10, min_per=2):
    """Bins keyed by numpy floor_divide over the data's own range, in order of their first member; ``picks``:
    positions kept in each overfull bin, consumed max_per at a time."""
    c, r = np.asarray(c, np.float64), np.asarray(r, np.float64)
    xs, ys = (c.max() - c.min()) / xbins, (r.max() - r.min()) / ybins
    if xs == 0 or ys == 0:
        raise ValueError("zero bin width")
    kx, ky = np.floor_divide(c - c.min(), xs), np.floor_divide(r - r.min(), ys)
    bins: "OrderedDict[tuple, list]" = OrderedDict()
    for i in range(c.shape[0]):
        bins.setdefault((kx[i], ky[i]), []).append(i)
    out, q = [], 0
    picks = np.asarray(picks, np.int64)
    for members in bins.values():
        if len(members) > max_per:
            out += [members[p] for p in picks[q:q + max_per]]
            q += max_per
        elif len(members) > min_per:
            out += members
    return np.array(out, np.int64)


def pareto_indices(c, r):
    """Indices (ascending) that no point dominates in (-c, r)."""
    c, r = np.asarray(c, np.float64), np.asarray(r, np.float64)
    keep = [i for i in range(c.shape[0])
            if not np.any((c <= c[i]) & (r >= r[i]) & ((c < c[i]) | (r > r[i])))]
    return np.array(keep, np.int64)


def nearest_with_partners(fc, fr, tc, tr, u_part, max_rew_decrease, beta):
    """Masked argmin per target, then for every nearest index used k > 1 times (first-use order) k - 1 partners by
    inverse cdf of 1 / (dist + beta) over c <= c_i, r >= r_i - max_rew_decrease."""
    near = []
    for c, r in zip(tc, tr):
        m = np.flatnonzero(fc <= c)
        near.append(int(m[np.argmin(np.hypot(fc[m] - c, fr[m] - r))]))
    counts: "OrderedDict[int, int]" = OrderedDict()
    for i in near:
        counts[i] = counts.get(i, 0) + 1
    out, d = [], 0
    for i, k in counts.items():
        out.append(i)
        if k > 1:
            m = np.flatnonzero((fc <= fc[i]) & (fr >= fr[i] - max_rew_decrease))
            w = 1.0 / (np.hypot(fc[m] - fc[i], fr[m] - fr[i]) + beta)
            cdf = np.cumsum(w / w.sum())
            cdf /= cdf[-1]
            u = np.asarray(u_part[d:d + k - 1], np.float64)
            d += k - 1
            out += m[np.searchsorted(cdf, u, side="right")].tolist()
    return np.array(out, np.int64)


def combine(t, src, tc, tr, noise_c=None, noise_r=None):
    """Originals followed by one copy of trajectory src[k] per target, returns shifted to the target."""
    s, L = np.asarray(t["traj_start"], np.int64), np.asarray(t["traj_len"], np.int64)
    parts = {k: [np.asarray(t[k])] for k in KEYS}
    row = 0
    for k, j in enumerate(src):
        sl = slice(s[j], s[j] + L[j])
        for key in ("observations", "actions", "rewards", "costs"):
            parts[key].append(np.asarray(t[key])[sl])
        for key, tgt, nz in (("cost_returns", tc[k], noise_c), ("returns", tr[k], noise_r)):
            x = np.asarray(t[key])[sl]
            shift = np.float64(tgt) - np.float64(x[0])
            if nz is not None:
                shift = shift + np.asarray(nz[row:row + L[j]], np.float64)
            parts[key].append((x.astype(np.float64) + shift).astype(np.float32))
        row += L[j]
    out = {k: np.concatenate(v) for k, v in parts.items()}
    lens = np.concatenate([L, L[np.asarray(src, np.int64)]]) if len(src) else L
    out["traj_len"] = lens
    out["traj_start"] = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return out


def augmentation(t, deg=3, max_rew_decrease=1.0, beta=1.0, augment_percent=0.3, max_reward=1000.0, min_reward=0.0,
                 draws: Optional[dict] = None):
    """Returns (combined tables, info) -- info: idx, indices, coef, pareto."""
    r0, c0 = first_returns(t)
    ind = grid_filter(c0, r0, draws.get("pick", []))
    if ind.size == 0:
        raise ValueError("empty filter")
    fc, fr = c0[ind], r0[ind]
    par = pareto_indices(fc, fr)
    coef = np.polyfit(fc[par], fr[par], deg)
    S = int(augment_percent * fc.shape[0])
    tc = np.linspace(fc.min(), fc.max(), S)
    low = np.polyval(coef, tc) + min_reward
    tr = low + (max_reward - low) * np.asarray(draws["u_rew"][:S], np.float64)
    idx = nearest_with_partners(fc, fr, tc, tr, draws.get("u_part", []), max_rew_decrease, beta) if S else \
        np.zeros(0, np.int64)
    return combine(t, ind[idx], tc, tr), dict(idx=idx, indices=ind, coef=coef, pareto=par)


def random_augmentation(t, augment_percent=0.3, aug_rmin=0, aug_rmax=600, aug_cmin=5, aug_cmax=50, cgap=5,
                        draws: Optional[dict] = None):
    r0, c0 = first_returns(t)
    S = int(augment_percent * c0.shape[0])
    u = np.asarray(draws["u_cr"][:2 * S], np.float64).reshape(S, 2)
    tc = aug_cmin + (aug_cmax - aug_cmin) * u[:, 0]
    tr = aug_rmin + (aug_rmax - aug_rmin) * u[:, 1]
    near = []
    for c, r in zip(tc, tr):
        m = np.flatnonzero(c0 <= max(c - cgap, c0.min() + 1))
        near.append(int(m[np.argmin(np.hypot(c0[m] - c, r0[m] - r))]))
    near = np.array(near, np.int64)
    return combine(t, near, tc, tr, draws["noise_c"], draws["noise_r"]), dict(idx=near)


def bc_frontier(ep_cost, ep_rew, cost_returns, rew_returns):
    """process_bc_dataset "frontier": (keep mask over transitions, chosen degree)."""
    ep_cost, ep_rew = np.asarray(ep_cost, np.float64), np.asarray(ep_rew, np.float64)
    par = pareto_indices(ep_cost, ep_rew)
    x, y = ep_cost[par], ep_rew[par]
    with np.errstate(all="ignore"):
        for deg in (0, 1, 2):
            coef = np.polyfit(x, y, deg)
            r2 = 1 - np.sum((y - np.polyval(coef, x)) ** 2) / np.sum((y - y.mean()) ** 2)
            if r2 >= 0.9:
                break
    band = (ep_rew.max() - ep_rew.min()) / 5
    pf = np.polyval(coef, np.asarray(cost_returns, np.float64))
    rr = np.asarray(rew_returns, np.float64)
    return (pf - band <= rr) & (rr <= pf + band), deg
