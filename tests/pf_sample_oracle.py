"""numpy restatement of the frontier-distance sampling weights (csrc/pf_dist.h, common.ingest.compute_sample_prob):
what the reference's ``compute_sample_prob`` (osrl/common/dataset.py:399-436) computes wherever its BFGS solve
behaves, written as a definition instead of a solver.

For trajectory (c, r) = (cost return, return) and the frontier polynomial p (np.polyfit order):
  f(x) = (x - c)^2 + (p(x) - r)^2,   g(x) = (x - c) + (p(x) - r) p'(x)   (= f'(x) / 2)
  x* = c if g(c) == 0; the largest root of g below c where g changes sign if g(c) > 0; the smallest such root
  above c if g(c) < 0 (downhill from x0 = c to the first stationary point);
  x = max(0, x*), dist = sqrt(f(x)), w = 1 / (dist + beta), prob = w / sum(w).

The roots come from ``np.roots`` (companion-matrix eigenvalues, batched over the trajectories).  Their real parts
cut the axis on the downhill side of c into stretches; g is sampled at every stretch's midpoint and, so that a pair
of roots too close for the eigenvalues to separate still shows, at the critical points of g (``np.roots`` of g').
The first sample with the other sign and the sample before it bracket x*, and bisection sharpens it to fp64
resolution (the eigenvalues alone carry the companion matrix's conditioning).
"""
from __future__ import annotations

import numpy as np


def g_coefficients(coef, c, r):
    """[n, 2d] coefficients of g, highest power first (d = deg p >= 1)."""
    a = np.asarray(coef, np.float64)
    d = a.shape[0] - 1
    asc = np.zeros((c.shape[0], 2 * d))  # ascending powers: the product (p - r) p', its terms added in a fixed order
    for i in range(d + 1):
        qi = a[d] - r if i == 0 else np.full_like(r, a[d - i])
        for j in range(d):
            asc[:, i + j] = asc[:, i + j] + qi * ((j + 1.0) * a[d - 1 - j])
    asc[:, 0] = asc[:, 0] - c            # + (x - c)
    asc[:, 1] = asc[:, 1] + 1.0
    return asc[:, ::-1].copy()


def _roots_real(poly):
    """Real parts of np.roots of every row ([n, k+1] -> [n, k]); k >= 1."""
    n, k = poly.shape[0], poly.shape[1] - 1
    if k == 1:
        return -poly[:, 1:] / poly[:, :1]
    comp = np.zeros((n, k, k))
    comp[:, np.arange(1, k), np.arange(0, k - 1)] = 1.0
    comp[:, 0, :] = -poly[:, 1:] / poly[:, :1]
    return np.linalg.eigvals(comp).real


def _polyval_rows(g, x):
    """g [n, k] evaluated at x [n] or [n, s]."""
    gg = g if x.ndim == 1 else g[:, :, None]
    v = np.zeros_like(x)
    with np.errstate(all="ignore"):
        for k in range(g.shape[1]):
            v = v * x + gg[:, k]
    return v


def stationary_points(coef, c, r):
    """x* per trajectory (before the clamp at 0)."""
    coef = np.trim_zeros(np.asarray(coef, np.float64), "f")
    c, r = np.asarray(c, np.float64), np.asarray(r, np.float64)
    if coef.shape[0] <= 1:
        return c.copy()
    g = g_coefficients(coef, c, r)
    n, m = g.shape[0], g.shape[1] - 1
    gc = _polyval_rows(g, c)
    sgn = np.where(gc > 0.0, -1.0, 1.0)                  # walking direction
    bound = 1.0 + np.max(np.abs(g[:, 1:] / g[:, :1]), axis=1)  # Cauchy: every root inside
    t_end = np.maximum(sgn * (sgn * bound - c), 0.0) + 1.0     # walking distance to a point past every root
    def walk(x):  # positions -> walking distances from c, inf for the ones behind c
        t = sgn[:, None] * (x - c[:, None])
        return np.where(t > 0.0, t, np.inf)
    with np.errstate(all="ignore"):
        cuts = np.sort(np.concatenate([np.zeros((n, 1)), np.minimum(walk(_roots_real(g)), t_end[:, None]),
                                       t_end[:, None]], axis=1), axis=1)
        mids = 0.5 * cuts[:, :-1] + 0.5 * cuts[:, 1:]
        parts = [mids, t_end[:, None]]
        if m >= 2:
            dg = g[:, :-1] * np.arange(m, 0, -1)[None, :]
            parts.append(walk(_roots_real(dg)))
        t = np.sort(np.concatenate(parts, axis=1), axis=1)
        t = np.where(t <= t_end[:, None], t, t_end[:, None])
        xs = c[:, None] + sgn[:, None] * t
        v = _polyval_rows(g, xs)
    other = (v * gc[:, None] <= 0.0) & (t > 0.0)         # the other sign (or an exact zero)
    other[:, -1] = True
    first = np.argmax(other, axis=1)
    rows = np.arange(n)
    far = xs[rows, first]
    near = np.where(first > 0, xs[rows, np.maximum(first - 1, 0)], c)
    near = np.where(t[rows, np.maximum(first - 1, 0)] > 0.0, near, c)
    # g(lo) < 0 < g(hi): walking left (g(c) > 0) the far end is the negative one
    lo, hi = np.where(gc > 0.0, far, near), np.where(gc > 0.0, near, far)
    live = gc != 0.0
    for _ in range(2200):
        mid = 0.5 * lo + 0.5 * hi
        act = live & (mid > lo) & (mid < hi)
        if not act.any():
            break
        vm = _polyval_rows(g, mid)
        zero = act & (vm == 0.0)
        lo = np.where(zero | (act & (vm < 0.0)), mid, lo)
        hi = np.where(zero | (act & (vm > 0.0)), mid, hi)
    out = np.where(np.abs(_polyval_rows(g, lo)) <= np.abs(_polyval_rows(g, hi)), lo, hi)
    return np.where(live, out, c)


def solve(coef, c, r):
    """(x, dist): the clamped stationary point and the distance to the curve there."""
    c, r = np.asarray(c, np.float64), np.asarray(r, np.float64)
    x = np.maximum(0.0, stationary_points(coef, c, r))
    p = np.poly1d(np.asarray(coef, np.float64))
    return x, np.sqrt((x - c) ** 2 + (p(x) - r) ** 2)


def distances(coef, c, r):
    return solve(coef, c, r)[1]


def evaluation_noise(coef, x, r):
    """A bound on the rounding error of evaluating p(x) - r by Horner's rule in fp64: 2 (d + 1) eps (sum |a_k| |x|^k
    + |r|) (Higham, Accuracy and Stability of Numerical Algorithms, 5.1).  A trajectory whose distance is below a
    few of these lies ON the curve as far as fp64 can tell: its computed distance is rounding noise."""
    a = np.abs(np.asarray(coef, np.float64))
    return 2.0 * a.shape[0] * np.finfo(np.float64).eps * (np.polyval(a, np.abs(x)) + np.abs(r))


def sample_prob(coef, c, r, beta=1.0):
    """(prob fp64, dist fp64): compute_sample_prob's result under the definition above."""
    dist = distances(coef, c, r)
    w = 1.0 / (dist + beta)
    return w / np.sum(w), dist


def weights_to_cdf(w):
    """fp32 (prob, inclusive cdf) of non-negative weights, sums in fp64."""
    w = np.asarray(w, np.float64)
    return (w / w.sum()).astype(np.float32), (np.cumsum(w) / w.sum()).astype(np.float32)


# what the CPU and the GPU test share: the golden cases (tests/golden/pf_sample.npz) and their gate
EXACT_CASES = ("d0_p50", "d1_p20", "d2_p50", "d3_p20")   # the reference's solver behaves on every trajectory
PATH_DEPENDENT = {"d4_p20": 0.10, "single_pf": 0.03}      # largest share of trajectories allowed to disagree


def golden_case(g, name):
    return g[f"{name}_coef"], g[f"{name}_c"].astype(np.float64), g[f"{name}_r"].astype(np.float64)


def outside(dist, ref):
    """Trajectories whose distance misses the reference's: |dist - ref| > 1e-6 (1 + ref)."""
    return np.abs(dist - ref) > 1e-6 * (1.0 + ref)
