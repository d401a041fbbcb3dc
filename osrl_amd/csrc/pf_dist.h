// Distance of one (cost return, return) point to the fitted Pareto frontier, as the reference's compute_sample_prob
// (osrl/common/dataset.py:399-436) arrives at it: not the nearest point of the curve, but the stationary point of
//   f(x) = (x - c)^2 + (p(x) - r)^2
// that going downhill from x0 = c reaches first.  With g(x) = f'(x) / 2 = (x - c) + (p(x) - r) p'(x):
//   g(c) == 0: x* = c;   g(c) > 0: the largest root of g below c where g changes sign;
//   g(c) < 0: the smallest such root above c.
// For deg p = d >= 1 the degree of g is 2d - 1 (odd) and its leading coefficient d a0^2 is positive, so the root
// exists.  Then x = max(0, x*), dist = sqrt(f(x)).
//
// The roots are isolated through the derivative chain, never by stepping: between two consecutive roots of
// g^(k+1) (and between the outermost ones and the Cauchy bound of g, which holds every root of every derivative by
// Gauss-Lucas) g^(k) is monotone, so it has one root there iff its signs at the two ends differ, and bisection to
// fp64 resolution finds it.  A close pair of roots is therefore never stepped over: the critical point between them
// is a breakpoint.  The last level walks from c over the critical points of g in the downhill direction and stops
// at the first sign change.
//
// One caller = one point.  The per-point tables (coefficients of g, of the current derivative, two root lists) are
// addressed through `mem[slot * stride]`: an LDS slice per thread on the device (no scratch), a plain array on the
// host.  fp64 throughout, no contraction, so a host build gives the device's bits.
#pragma once

#if defined(__HIPCC__)
#define OSRL_PF_HD __host__ __device__ __forceinline__
#else
#define OSRL_PF_HD inline
#endif

namespace osrl_pf {

#pragma clang fp contract(off)

constexpr int kMaxDeg = 7;            // of the frontier polynomial, as osrl_polyfit
constexpr int kMaxG = 2 * kMaxDeg;    // coefficients of g (degree <= 13)
constexpr int kSlotG = 0;             // g, ascending powers                       [kMaxG]
constexpr int kSlotP = kMaxG;         // the current derivative level, ascending   [kMaxG]
constexpr int kSlotR = 2 * kMaxG;     // two root lists (previous / current level) [2][kMaxG]
constexpr int kSlots = 4 * kMaxG;
constexpr int kMaxBisect = 2200;      // halvings from any fp64 interval down to neighbouring doubles

OSRL_PF_HD double pf_abs(double v) { return v < 0.0 ? -v : v; }

// sum_{i <= deg} P[i] x^i
OSRL_PF_HD double pf_eval(const double* P, int stride, int deg, double x) {
  double v = P[deg * stride];
  for (int i = deg - 1; i >= 0; --i) v = v * x + P[i * stride];
  return v;
}

// the root of the monotone stretch (lo, hi): P(lo) and P(hi) have opposite signs (lo_neg: P(lo) < 0); |flo|, |fhi|
// are the magnitudes at the ends (infinity where only the sign is known).  Ends at neighbouring doubles and returns
// the one where |P| is smaller.
OSRL_PF_HD double pf_bisect(const double* P, int stride, int deg, double lo, double hi, bool lo_neg, double flo,
                            double fhi) {
  for (int it = 0; it < kMaxBisect; ++it) {
    const double mid = 0.5 * lo + 0.5 * hi;
    if (!(mid > lo && mid < hi)) break;
    const double v = pf_eval(P, stride, deg, mid);
    if (v == 0.0) return mid;
    if ((v < 0.0) == lo_neg) {
      lo = mid;
      flo = pf_abs(v);
    } else {
      hi = mid;
      fhi = pf_abs(v);
    }
  }
  return flo <= fhi ? lo : hi;
}

// a: frontier coefficients, highest power first, a[0] != 0 unless d == 0.  Returns dist.
OSRL_PF_HD double pf_distance(const double* a, int d, double c, double r, double* mem, int stride) {
  const double kInf = __builtin_huge_val();
  double* G = mem + kSlotG * stride;
  double* P = mem + kSlotP * stride;
  double xs = c;
  if (d >= 1) {
    // g = (p - r) p' + (x - c), ascending: p_i = a[d - i], p'_j = (j + 1) p_{j+1}
    int m = 2 * d - 1;
    for (int k = 0; k <= m; ++k) G[k * stride] = 0.0;
    for (int i = 0; i <= d; ++i) {
      const double qi = i == 0 ? a[d] - r : a[d - i];
      for (int j = 0; j < d; ++j) {
        const double t = qi * ((double)(j + 1) * a[d - 1 - j]);
        G[(i + j) * stride] = G[(i + j) * stride] + t;
      }
    }
    G[0] = G[0] - c;
    G[stride] = G[stride] + 1.0;
    while (m > 0 && G[m * stride] == 0.0) --m;  // d a0^2 underflowed
    const double lead = G[m * stride];
    double B = 0.0;  // Cauchy: every root of g (and of its derivatives) has |x| < 1 + max |g_i / g_m|
    for (int i = 0; i < m; ++i) {
      const double q = pf_abs(G[i * stride] / lead);
      B = q > B ? q : B;
    }
    B = B + 1.0;
    const double gc = pf_eval(G, stride, m, c);
    if (m >= 1 && gc != 0.0 && B < kInf) {
      // roots of g^(m-j) / (m-j)! for j = 1 .. m-1, each level between the roots of the one before
      int nprev = 0, cur = 0;
      for (int j = 1; j < m; ++j) {
        const int k = m - j;
        long long binom = 1;  // C(i + k, k)
        for (int i = 0; i <= j; ++i) {
          P[i * stride] = G[(i + k) * stride] * (double)binom;
          binom = binom * (i + 1 + k) / (i + 1);
        }
        const double* Rp = mem + (kSlotR + (cur ^ 1) * kMaxG) * stride;
        double* Rc = mem + (kSlotR + cur * kMaxG) * stride;
        int n = 0;
        double lo = -B, flo = ((lead < 0.0) != ((j & 1) != 0)) ? -kInf : kInf;  // sign of the leading term at -B
        for (int t = 0; t <= nprev; ++t) {
          const double hi = t == nprev ? B : Rp[t * stride];
          const double fhi = t == nprev ? (lead < 0.0 ? -kInf : kInf) : pf_eval(P, stride, j, hi);
          if ((flo < 0.0 && fhi > 0.0) || (flo > 0.0 && fhi < 0.0))
            Rc[n++ * stride] = pf_bisect(P, stride, j, lo, hi, flo < 0.0, pf_abs(flo), pf_abs(fhi));
          else if (fhi == 0.0)
            Rc[n++ * stride] = hi;  // a root that is also a critical point
          lo = hi;
          flo = fhi;
        }
        nprev = n;
        cur ^= 1;
      }
      // downhill from c over the critical points of g (the last list), to the first sign change
      const double* Rp = mem + (kSlotR + (cur ^ 1) * kMaxG) * stride;
      if (gc > 0.0) {
        double hi = c, fhi = gc;
        bool found = false;
        for (int t = nprev - 1; t >= 0 && !found; --t) {
          const double lo = Rp[t * stride];
          if (!(lo < hi)) continue;
          const double flo = pf_eval(G, stride, m, lo);
          if (flo < 0.0) {
            xs = pf_bisect(G, stride, m, lo, hi, true, -flo, fhi);
            found = true;
          } else if (flo > 0.0) {  // an exact zero here touches the axis: the next stretch decides
            hi = lo;
            fhi = flo;
          } else {
            hi = lo;
            fhi = 0.0;
          }
        }
        if (!found) {
          const bool neg_end = (lead < 0.0) != ((m & 1) != 0);
          xs = (neg_end && -B < hi) ? pf_bisect(G, stride, m, -B, hi, true, kInf, fhi) : (-B < hi ? -B : hi);
        }
      } else {
        double lo = c, flo = -gc;
        bool found = false;
        for (int t = 0; t < nprev && !found; ++t) {
          const double hi = Rp[t * stride];
          if (!(hi > lo)) continue;
          const double fhi = pf_eval(G, stride, m, hi);
          if (fhi > 0.0) {
            xs = pf_bisect(G, stride, m, lo, hi, true, flo, fhi);
            found = true;
          } else {
            lo = hi;
            flo = -fhi;
          }
        }
        if (!found) xs = (lead > 0.0 && B > lo) ? pf_bisect(G, stride, m, lo, B, true, flo, kInf) : (B > lo ? B : lo);
      }
    }
  }
  const double x = xs > 0.0 ? xs : 0.0;
  double p = 0.0 * x + a[0];  // np.poly1d.__call__ = polyval: Horner from zeros_like(x)
  for (int k = 1; k <= d; ++k) p = p * x + a[k];
  const double dx = x - c, dy = p - r;
  return sqrt(dx * dx + dy * dy);
}

}  // namespace osrl_pf
