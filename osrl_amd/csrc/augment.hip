// Pareto-frontier dataset augmentation on device: the reference's CDT return relabelling
// (osrl/common/dataset.py:186-396 get_nearest_point / grid_filter / augmentation), its random_augmentation
// (:557-630) and process_bc_dataset's "frontier" mode (:47-92, :111) -- which the reference runs on the host with
// oapackage's Pareto search and numpy's polyfit -- as kernels over the tables csrc/ingest.hip produced, so the
// augmented tables are built in HBM and never leave it.
//
// Everything per trajectory is fp64 as in numpy (the fp32 returns widened once); the relabelled rows are rounded
// back to fp32 exactly where numpy's in-place add of a float64 operand to a float32 array rounds.  The selection
// work is small (the grid filter keeps <= 10 trajectories per bin of a 11 x 51 grid), so most stages are one
// workgroup; the row copies are a grid.  Every random draw is either Philox (keyed by the caller's seed) or read
// from an injected array in the reference's order of use.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdint>

#include "../../include/osrl_amd.h"
#include "pf_dist.h"
#include "philox.h"

namespace {

#pragma clang fp contract(off)  // numpy rounds every multiply and add on its own

using osrl_rng::philox4x32_10;
using osrl_rng::U4;

constexpr int kWg = 1024;                 // single-workgroup kernels
constexpr int kWaves = kWg / 64;
constexpr int kMaxBins = 576;             // (xbins+1) x (ybins+1): the reference's 10 x 50 grid needs 561
constexpr int kMaxPerBin = 32;
constexpr int kMaxCoef = 8;               // deg <= 7
constexpr uint32_t kAugStream = 0x20000000u;  // Philox counter word 3 (dropout uses 0x40000000 | site)
enum : uint32_t { kDrawPick = 1, kDrawReward = 2, kDrawPartner = 3, kDrawRandCR = 4, kDrawNoise = 5 };

__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {  // [0,1) with 53 random bits, as numpy's next_double
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ U4 aug_words(uint32_t kind, uint64_t i, uint64_t seed) {
  return philox4x32_10(U4{(uint32_t)i, (uint32_t)(i >> 32), kind, kAugStream}, (uint32_t)seed, (uint32_t)(seed >> 32));
}

__device__ __forceinline__ double draw_u(uint32_t kind, uint64_t i, uint64_t seed) {
  const U4 r = aug_words(kind, i, seed);
  return u53(r.x, r.y);
}

// numpy's float floor_divide (npy_divmod): fmod, then (a - mod) / b snapped to the nearest integer; b > 0 here
__device__ __forceinline__ double np_floor_divide(double a, double b) {
  double mod = fmod(a, b);
  double div = (a - mod) / b;
  if (mod != 0.0 && ((b < 0) != (mod < 0))) div -= 1.0;
  if (div != 0.0) {
    double fl = floor(div);
    if (div - fl > 0.5) fl += 1.0;
    return fl;
  }
  return copysign(0.0, a / b);
}

// block-wide reductions / scans over a 1024-thread workgroup (fixed order: deterministic results)
__device__ double wg_sum(double v, double* red /*[kWaves]*/) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
  __syncthreads();
  return t;
}

__device__ double wg_min(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  double t = red[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) t = fmin(t, red[i]);
  __syncthreads();
  return t;
}

__device__ double wg_max(double v, double* red) { return -wg_min(-v, red); }

// exclusive scan of one int per thread; *total = block sum
__device__ int wg_excl_scan(int v, int* total, int* wsum /*[kWaves]*/) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  __syncthreads();
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  int base = 0, all = 0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) {
    const int s = wsum[i];
    if (i < wv) base += s;
    all += s;
  }
  __syncthreads();
  *total = all;
  return base + incl - v;
}

// ---------------------------------------------------------------------------------------------------------------
__global__ void traj_returns_kernel(const float* __restrict__ ret, const float* __restrict__ cret,
                                    const int64_t* __restrict__ start, int n, double* __restrict__ r0,
                                    double* __restrict__ c0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  r0[i] = (double)ret[start[i]];
  c0[i] = (double)cret[start[i]];
}

// grid_filter (dataset.py:239-272) with the bounds augmentation() passes (the data's own min / max).  Bins are
// dict keys in order of their first member; members are in index order; a bin with more than max_per_bin members
// keeps max_per_bin of them in draw order (random.sample); one with min_per_bin or fewer is dropped.
struct FilterLds {
  int whist[kWaves][kMaxBins];
  int run[kMaxBins];
  int first[kMaxBins];
  int boff[kMaxBins];
  int ord[kMaxBins];
  int by_ord_keep[kMaxBins];
  int by_ord_over[kMaxBins];
  int wsum[kWaves];
  double red[kWaves];
};

__global__ __launch_bounds__(kWg) void grid_filter_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                          int n, int xbins, int ybins, int max_per, int min_per,
                                                          const int32_t* __restrict__ pick_in, uint64_t seed,
                                                          int32_t* __restrict__ key, int32_t* __restrict__ rank,
                                                          int32_t* __restrict__ sorted, int32_t* __restrict__ filt,
                                                          double* __restrict__ fx, double* __restrict__ fy,
                                                          int32_t* __restrict__ count) {
  __shared__ FilterLds s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ny = ybins + 1, nbins = (xbins + 1) * ny;
  double xmn = DBL_MAX, xmx = -DBL_MAX, ymn = DBL_MAX, ymx = -DBL_MAX;
  for (int i = tid; i < n; i += kWg) {
    xmn = fmin(xmn, x[i]);
    xmx = fmax(xmx, x[i]);
    ymn = fmin(ymn, y[i]);
    ymx = fmax(ymx, y[i]);
  }
  xmn = wg_min(xmn, s.red);
  xmx = wg_max(xmx, s.red);
  ymn = wg_min(ymn, s.red);
  ymx = wg_max(ymx, s.red);
  const double xstep = (xmx - xmn) / (double)xbins, ystep = (ymx - ymn) / (double)ybins;
  if (!(xstep > 0.0) || !(ystep > 0.0)) {  // the reference divides by a zero bin width here
    if (tid == 0) *count = -1;
    return;
  }
  for (int b = tid; b < kMaxBins; b += kWg) {
    s.run[b] = 0;
    s.first[b] = INT_MAX;
    for (int w = 0; w < kWaves; ++w) s.whist[w][b] = 0;
  }
  __syncthreads();
  // stable rank of every trajectory inside its bin, 1024 trajectories at a time
  for (int c0 = 0; c0 < n; c0 += kWg) {
    const int i = c0 + tid;
    int k = -1;
    if (i < n) {
      int xb = (int)np_floor_divide(x[i] - xmn, xstep), yb = (int)np_floor_divide(y[i] - ymn, ystep);
      xb = min(max(xb, 0), xbins);
      yb = min(max(yb, 0), ybins);
      k = xb * ny + yb;
    }
    int r = 0;
    for (int l = 0; l < 64; ++l) {
      const int kl = __shfl(k, l);
      r += (l < lane && kl == k) ? 1 : 0;
    }
    if (k >= 0) atomicAdd(&s.whist[wv][k], 1);
    __syncthreads();
    if (k >= 0) {
      int rr = s.run[k] + r;
      for (int w = 0; w < wv; ++w) rr += s.whist[w][k];
      key[i] = k;
      rank[i] = rr;
      if (rr == 0) s.first[k] = i;
    }
    __syncthreads();
    for (int b = tid; b < nbins; b += kWg) {
      int t = 0;
      for (int w = 0; w < kWaves; ++w) {
        t += s.whist[w][b];
        s.whist[w][b] = 0;
      }
      s.run[b] += t;
    }
    __syncthreads();
  }
  // bin offsets in bin-id order (counting sort), then dict order = order of first members
  {
    int tot;
    const int v = tid < nbins ? s.run[tid] : 0;
    const int ex = wg_excl_scan(v, &tot, s.wsum);
    if (tid < nbins) s.boff[tid] = ex;
  }
  __syncthreads();
  for (int i = tid; i < n; i += kWg) sorted[s.boff[key[i]] + rank[i]] = i;
  for (int b = tid; b < nbins; b += kWg) {
    int o = 0;
    if (s.run[b] > 0)
      for (int b2 = 0; b2 < nbins; ++b2) o += (s.run[b2] > 0 && s.first[b2] < s.first[b]) ? 1 : 0;
    s.ord[b] = o;
  }
  for (int b = tid; b < kMaxBins; b += kWg) s.by_ord_keep[b] = s.by_ord_over[b] = 0;
  __syncthreads();
  for (int b = tid; b < nbins; b += kWg) {
    const int c = s.run[b];
    if (c == 0) continue;
    const int over = c > max_per;
    s.by_ord_keep[s.ord[b]] = over ? max_per : (c <= min_per ? 0 : c);
    s.by_ord_over[s.ord[b]] = over;
  }
  __syncthreads();
  int keep_off = 0, over_off = 0, n_keep = 0, n_over = 0;
  {
    const int vk = tid < kMaxBins ? s.by_ord_keep[tid] : 0, vo = tid < kMaxBins ? s.by_ord_over[tid] : 0;
    keep_off = wg_excl_scan(vk, &n_keep, s.wsum);
    over_off = wg_excl_scan(vo, &n_over, s.wsum);
  }
  __syncthreads();
  if (tid < kMaxBins) {  // reuse: by_ord_* now hold the exclusive offsets
    s.by_ord_keep[tid] = keep_off;
    s.by_ord_over[tid] = over_off;
  }
  __syncthreads();
  for (int b = tid; b < nbins; b += kWg) {
    const int c = s.run[b];
    if (c == 0) continue;
    const int off = s.by_ord_keep[s.ord[b]];
    const int* mem = sorted + s.boff[b];
    if (c > max_per) {
      const int q = s.by_ord_over[s.ord[b]];
      int chosen[kMaxPerBin];
      for (int k = 0; k < max_per; ++k) {
        int pos;
        if (pick_in) {
          pos = min(max(pick_in[(int64_t)q * max_per + k], 0), c - 1);
        } else {  // uniform without replacement: redraw a taken position (bounded; then the first free one)
          pos = -1;
          for (uint32_t a = 0; a < 4096 && pos < 0; ++a) {
            const U4 r = aug_words(kDrawPick, ((uint64_t)q << 24) | ((uint64_t)k << 12) | a, seed);
            const int p = (int)(((uint64_t)r.x * (uint64_t)c) >> 32);
            bool dup = false;
            for (int j = 0; j < k; ++j) dup |= chosen[j] == p;
            if (!dup) pos = p;
          }
          for (int p = 0; pos < 0 && p < c; ++p) {
            bool dup = false;
            for (int j = 0; j < k; ++j) dup |= chosen[j] == p;
            if (!dup) pos = p;
          }
        }
        chosen[k] = pos;
        filt[off + k] = mem[pos];
      }
    } else if (c > min_per) {
      for (int k = 0; k < c; ++k) filt[off + k] = mem[k];
    }
  }
  __syncthreads();
  __threadfence_block();
  for (int j = tid; j < n_keep; j += kWg) {
    fx[j] = x[filt[j]];
    fy[j] = y[filt[j]];
  }
  if (tid == 0) *count = n_keep;
}

// flag[i] = 1 iff no point dominates (-c_i, r_i): c_j <= c_i and r_j >= r_i with one of them strict
__global__ __launch_bounds__(256) void pareto_mask_kernel(const double* __restrict__ c, const double* __restrict__ r,
                                                          int n, int32_t* __restrict__ flag) {
  __shared__ double tc[256], tr[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < n;
  const double ci = valid ? c[i] : 0.0, ri = valid ? r[i] : 0.0;
  int dom = valid ? 0 : 1;
  for (int j0 = 0; j0 < n; j0 += 256) {
    if (__syncthreads_and(dom)) break;  // every point of this block is dominated already
    const int j = j0 + threadIdx.x;
    tc[threadIdx.x] = j < n ? c[j] : 0.0;
    tr[threadIdx.x] = j < n ? r[j] : 0.0;
    __syncthreads();
    const int m = min(256, n - j0);
    if (!dom)
      for (int t = 0; t < m; ++t) {
        const double cj = tc[t], rj = tr[t];
        if (cj <= ci && rj >= ri && (cj < ci || rj > ri)) {
          dom = 1;
          break;
        }
      }
  }
  if (valid) flag[i] = dom ? 0 : 1;
}

// np.polyfit(x[P], y[P], deg) over the flagged points P in index order (polynomial.py: Vandermonde, columns scaled
// by their 2-norm, lstsq with rcond = len(x) * eps), the least-squares solve as a one-sided Jacobi SVD -- the
// minimum-norm answer when the fit is rank-deficient.  pick: process_bc_dataset's rule (dataset.py:83-90), deg 0,
// 1, 2 until r^2 >= 0.9.  stats = {r2(0), r2(1), r2(2), max y, min y (over ALL n points)}.
__device__ __forceinline__ double horner(const double* cf, int d, double x) {
  double v = 0.0 * x + cf[0];  // numpy's polyval starts from zeros_like(x)
  for (int k = 1; k <= d; ++k) {
    const double t = v * x;
    v = t + cf[k];
  }
  return v;
}

__global__ __launch_bounds__(kWg) void polyfit_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                      const int32_t* __restrict__ flag, int n, int deg, int pick,
                                                      double* __restrict__ coef, int32_t* __restrict__ deg_out,
                                                      int32_t* __restrict__ pidx, int32_t* __restrict__ pcount,
                                                      double* __restrict__ stats, double* __restrict__ px,
                                                      double* __restrict__ py, double* __restrict__ A) {
  __shared__ double red[kWaves];
  __shared__ int wsum[kWaves];
  __shared__ double V[kMaxCoef][kMaxCoef], scale[kMaxCoef], cf[kMaxCoef];
  __shared__ int carry_s;
  const int tid = threadIdx.x;
  double ymx = -DBL_MAX, ymn = DBL_MAX;
  int carry = 0;
  for (int c0 = 0; c0 < n; c0 += kWg) {
    const int i = c0 + tid;
    const int f = i < n ? (flag ? flag[i] : 1) : 0;
    if (i < n) {
      ymx = fmax(ymx, y[i]);
      ymn = fmin(ymn, y[i]);
    }
    int tot;
    const int ex = wg_excl_scan(f, &tot, wsum);
    if (f) {
      pidx[carry + ex] = i;
      px[carry + ex] = x[i];
      py[carry + ex] = y[i];
    }
    carry += tot;
  }
  ymx = wg_max(ymx, red);
  ymn = wg_min(ymn, red);
  const int m = carry;
  if (tid == 0) {
    *pcount = m;
    stats[0] = stats[1] = stats[2] = __builtin_nan("");
    stats[3] = ymx;
    stats[4] = ymn;
    carry_s = 0;
  }
  __threadfence_block();
  __syncthreads();
  if (m == 0) return;
  const int d_lo = pick ? 0 : deg, d_hi = pick ? 2 : deg;
  for (int d = d_lo; d <= d_hi; ++d) {
    const int N = d + 1;
    for (int i = tid; i < m; i += kWg) {  // vander(x, N): column N-1-k holds x^k by repeated multiplication
      double p = 1.0;
      A[(int64_t)(N - 1) * m + i] = p;
      for (int k = 1; k < N; ++k) {
        p = p * px[i];
        A[(int64_t)(N - 1 - k) * m + i] = p;
      }
    }
    __syncthreads();
    for (int j = 0; j < N; ++j) {
      double t = 0.0;
      for (int i = tid; i < m; i += kWg) t += A[(int64_t)j * m + i] * A[(int64_t)j * m + i];
      t = wg_sum(t, red);
      if (tid == 0) scale[j] = sqrt(t);
    }
    __syncthreads();
    for (int j = 0; j < N; ++j)
      for (int i = tid; i < m; i += kWg) A[(int64_t)j * m + i] = A[(int64_t)j * m + i] / scale[j];
    if (tid < kMaxCoef * kMaxCoef) V[tid / kMaxCoef][tid % kMaxCoef] = (tid / kMaxCoef == tid % kMaxCoef) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < 64; ++sweep) {
      int rotated = 0;
      for (int p = 0; p < N - 1; ++p)
        for (int q = p + 1; q < N; ++q) {
          double a = 0.0, b = 0.0, g = 0.0;
          for (int i = tid; i < m; i += kWg) {
            const double ap = A[(int64_t)p * m + i], aq = A[(int64_t)q * m + i];
            a += ap * ap;
            b += aq * aq;
            g += ap * aq;
          }
          a = wg_sum(a, red);
          b = wg_sum(b, red);
          g = wg_sum(g, red);
          if (g == 0.0 || fabs(g) <= DBL_EPSILON * sqrt(a * b)) continue;
          rotated = 1;
          const double zeta = (b - a) / (2.0 * g);
          const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
          for (int i = tid; i < m; i += kWg) {
            const double ap = A[(int64_t)p * m + i], aq = A[(int64_t)q * m + i];
            A[(int64_t)p * m + i] = cs * ap - sn * aq;
            A[(int64_t)q * m + i] = sn * ap + cs * aq;
          }
          if (tid < N) {
            const double vp = V[tid][p], vq = V[tid][q];
            V[tid][p] = cs * vp - sn * vq;
            V[tid][q] = sn * vp + cs * vq;
          }
          __syncthreads();
        }
      if (!rotated) break;
    }
    // singular values = column norms; keep the min(m, N) largest above rcond * max
    double sig[kMaxCoef], uy[kMaxCoef];
    for (int j = 0; j < N; ++j) {
      double t = 0.0, u = 0.0;
      for (int i = tid; i < m; i += kWg) {
        const double aj = A[(int64_t)j * m + i];
        t += aj * aj;
        u += aj * py[i];
      }
      sig[j] = sqrt(wg_sum(t, red));
      uy[j] = wg_sum(u, red);
    }
    if (tid == 0) {
      double smax = 0.0;
      for (int j = 0; j < N; ++j) smax = fmax(smax, sig[j]);
      const double thr = (double)m * DBL_EPSILON * smax;
      bool keep[kMaxCoef];
      for (int j = 0; j < N; ++j) {
        int bigger = 0;  // rank of sig[j] (ties by column)
        for (int k = 0; k < N; ++k) bigger += (sig[k] > sig[j] || (sig[k] == sig[j] && k < j)) ? 1 : 0;
        keep[j] = sig[j] > thr && bigger < min(m, N);
      }
      double sol[kMaxCoef];
      for (int k = 0; k < N; ++k) sol[k] = 0.0;
      for (int j = 0; j < N; ++j)
        if (keep[j]) {
          const double w = uy[j] / (sig[j] * sig[j]);
          for (int k = 0; k < N; ++k) sol[k] += w * V[k][j];
        }
      for (int k = 0; k < N; ++k) cf[k] = sol[k] / scale[k];
    }
    __syncthreads();
    if (pick) {  // r^2 on the Pareto points (dataset.py:83-88)
      double sy = 0.0;
      for (int i = tid; i < m; i += kWg) sy += py[i];
      const double mean = wg_sum(sy, red) / (double)m;
      double tot = 0.0, res = 0.0;
      for (int i = tid; i < m; i += kWg) {
        const double e = py[i] - mean, f = py[i] - horner(cf, d, px[i]);
        tot += e * e;
        res += f * f;
      }
      tot = wg_sum(tot, red);
      res = wg_sum(res, red);
      const double r2 = 1.0 - res / tot;
      if (tid == 0) stats[d] = r2;
      if (r2 >= 0.9 || d == d_hi) {
        if (tid <= d) coef[tid] = cf[tid];
        if (tid == 0) *deg_out = d;
        return;
      }
      __syncthreads();
    } else {
      if (tid <= d) coef[tid] = cf[tid];
      if (tid == 0) *deg_out = d;
    }
  }
}

// augmentation() targets (dataset.py:350-365) and get_nearest_point's first loop (:207-217): one sample per thread
__global__ __launch_bounds__(256) void aug_targets_kernel(const double* __restrict__ coef, const int32_t* __restrict__ deg,
                                                          const double* __restrict__ fx, const double* __restrict__ fy,
                                                          int F, int S, double min_reward, double max_reward,
                                                          const double* __restrict__ u_rew, uint64_t seed,
                                                          double* __restrict__ tc, double* __restrict__ tr,
                                                          int32_t* __restrict__ near_raw) {
  __shared__ double red[4];
  __shared__ double cf[kMaxCoef];
  double mn = DBL_MAX, mx = -DBL_MAX;
  for (int j = threadIdx.x; j < F; j += blockDim.x) {
    mn = fmin(mn, fx[j]);
    mx = fmax(mx, fx[j]);
  }
  mn = wg_min(mn, red);
  mx = wg_max(mx, red);
  const int d = *deg;
  if (threadIdx.x <= (unsigned)d) cf[threadIdx.x] = coef[threadIdx.x];
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  // np.linspace(mn, mx, S): i * step + start, the last element = stop
  double c;
  if (S > 1) {
    const double delta = mx - mn, step = delta / (double)(S - 1);
    const double yi = step == 0.0 ? ((double)i / (double)(S - 1)) * delta : (double)i * step;
    c = i == S - 1 ? mx : yi + mn;
  } else {
    c = 0.0 * (mx - mn) + mn;
  }
  const double low = horner(cf, d, c) + min_reward;
  const double u = u_rew ? u_rew[i] : draw_u(kDrawReward, (uint64_t)i, seed);
  const double r = low + (max_reward - low) * u;
  int best = -1;
  double bd = 0.0;
  for (int j = 0; j < F; ++j) {
    const double cj = fx[j];
    if (!(cj <= c)) continue;
    const double dd = hypot(cj - c, fy[j] - r);
    if (best < 0 || dd < bd) {
      best = j;
      bd = dd;
    }
  }
  tc[i] = c;
  tr[i] = r;
  near_raw[i] = best < 0 ? 0 : best;
}

// Counter(nearest): first occurrence / count per filtered index; output offsets of every unique index (first
// occurrence order) and the offsets of its partner draws.  One workgroup; counts in LDS ([2 F] ints).
__global__ __launch_bounds__(kWg) void aug_dups_kernel(const int32_t* __restrict__ near_raw, int F, int S,
                                                       int32_t* __restrict__ nearest, int32_t* __restrict__ out_off,
                                                       int32_t* __restrict__ draw_off, int32_t* __restrict__ kcount) {
  extern __shared__ int dyn[];
  __shared__ int wsum[kWaves];
  int* cnt = dyn;
  int* first = dyn + F;
  for (int j = threadIdx.x; j < F; j += kWg) {
    cnt[j] = 0;
    first[j] = INT_MAX;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < S; i += kWg) {
    atomicAdd(&cnt[near_raw[i]], 1);
    atomicMin(&first[near_raw[i]], i);
  }
  __syncthreads();
  int co = 0, cd = 0;
  for (int c0 = 0; c0 < S; c0 += kWg) {
    const int i = c0 + threadIdx.x;
    int k = 0;
    if (i < S && first[near_raw[i]] == i) k = cnt[near_raw[i]];
    int to, td;
    const int eo = wg_excl_scan(k, &to, wsum);
    const int ed = wg_excl_scan(k > 0 ? k - 1 : 0, &td, wsum);
    if (i < S) {
      out_off[i] = co + eo;
      draw_off[i] = cd + ed;
      kcount[i] = k;
      if (k > 0) nearest[co + eo] = near_raw[i];
    }
    co += to;
    cd += td;
  }
}

// get_nearest_point's partner draws (dataset.py:219-235): for a unique nearest index with count k > 1, k - 1
// partners by np.random.choice over the mask c <= c_u, r >= r_u - max_rew_decrease with weights 1 / (hypot + beta):
// cdf = cumsum(w / sum w) / cdf[-1], index = searchsorted(cdf, u, 'right').  One block per sample; the cdf lives
// in LDS over all F points (points outside the mask add 0, so the first cdf value above u is a masked one).
__global__ __launch_bounds__(256) void aug_partners_kernel(const double* __restrict__ fx, const double* __restrict__ fy,
                                                           int F, const int32_t* __restrict__ near_raw,
                                                           const int32_t* __restrict__ out_off,
                                                           const int32_t* __restrict__ draw_off,
                                                           const int32_t* __restrict__ kcount, double max_rew_decrease,
                                                           double beta, const double* __restrict__ u_part,
                                                           uint64_t seed, int32_t* __restrict__ nearest) {
  extern __shared__ double cdf[];
  const int i = blockIdx.x;
  const int k = kcount[i];
  if (k <= 1) return;
  const int u = near_raw[i];
  const double pc = fx[u], pr = fy[u];
  for (int j = threadIdx.x; j < F; j += blockDim.x) {
    const bool msk = fx[j] <= pc && fy[j] >= pr - max_rew_decrease;
    cdf[j] = msk ? 1.0 / (hypot(fx[j] - pc, fy[j] - pr) + beta) : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int j = 0; j < F; ++j) tot += cdf[j];
    double acc = 0.0;
    for (int j = 0; j < F; ++j) {
      if (cdf[j] != 0.0) acc += cdf[j] / tot;
      cdf[j] = acc;
    }
  }
  __syncthreads();
  const double last = cdf[F - 1];
  __syncthreads();
  for (int j = threadIdx.x; j < F; j += blockDim.x) cdf[j] = cdf[j] / last;
  __syncthreads();
  for (int dd = threadIdx.x; dd < k - 1; dd += blockDim.x) {
    const int64_t di = (int64_t)draw_off[i] + dd;
    const double v = u_part ? u_part[di] : draw_u(kDrawPartner, (uint64_t)di, seed);
    int lo = 0, hi = F;  // first j with cdf[j] > v
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf[mid] <= v) lo = mid + 1;
      else hi = mid;
    }
    nearest[out_off[i] + 1 + dd] = min(lo, F - 1);
  }
}

// random_augmentation (dataset.py:586-615): uniform (c, r) targets, masked argmin over ALL trajectories
__global__ __launch_bounds__(256) void rand_targets_kernel(const double* __restrict__ c0, const double* __restrict__ r0,
                                                           int n, int S, double cmin_t, double cmax_t, double rmin_t,
                                                           double rmax_t, double cgap,
                                                           const double* __restrict__ u_cr, uint64_t seed,
                                                           double* __restrict__ tc, double* __restrict__ tr,
                                                           int32_t* __restrict__ nearest) {
  __shared__ double red[4];
  double mn = DBL_MAX;
  for (int j = threadIdx.x; j < n; j += blockDim.x) mn = fmin(mn, c0[j]);
  mn = wg_min(mn, red);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  double uc, ur;
  if (u_cr) {
    uc = u_cr[2 * (int64_t)i];
    ur = u_cr[2 * (int64_t)i + 1];
  } else {
    const U4 w = aug_words(kDrawRandCR, (uint64_t)i, seed);
    uc = u53(w.x, w.y);
    ur = u53(w.z, w.w);
  }
  const double c = cmin_t + (cmax_t - cmin_t) * uc, r = rmin_t + (rmax_t - rmin_t) * ur;
  const double bound = fmax(c - cgap, mn + 1.0);
  int best = -1;
  double bd = 0.0;
  for (int j = 0; j < n; ++j) {
    const double cj = c0[j];
    if (!(cj <= bound)) continue;
    const double dd = hypot(cj - c, r0[j] - r);
    if (best < 0 || dd < bd) {
      best = j;
      bd = dd;
    }
  }
  tc[i] = c;
  tr[i] = r;
  nearest[i] = best < 0 ? 0 : best;
}

// combined trajectory table: the n_traj originals, then one copy of trajectory src[k] = map[nearest[k]] per sample
__global__ __launch_bounds__(kWg) void aug_layout_kernel(const int32_t* __restrict__ nearest,
                                                         const int32_t* __restrict__ map, int S,
                                                         const int64_t* __restrict__ traj_start,
                                                         const int32_t* __restrict__ traj_len, int n_traj,
                                                         int64_t n_rows, int64_t* __restrict__ new_start,
                                                         int32_t* __restrict__ new_len, int32_t* __restrict__ src,
                                                         int64_t* __restrict__ total) {
  __shared__ int64_t wsum[kWaves];
  for (int e = threadIdx.x; e < n_traj; e += kWg) {
    new_start[e] = traj_start[e];
    new_len[e] = traj_len[e];
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int64_t carry = n_rows;
  for (int c0 = 0; c0 < S; c0 += kWg) {
    const int k = c0 + threadIdx.x;
    int t = 0, L = 0;
    if (k < S) {
      t = map ? map[nearest[k]] : nearest[k];
      L = traj_len[t];
    }
    int64_t incl = L;
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    __syncthreads();
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int64_t base = 0, all = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wv) base += wsum[w];
      all += wsum[w];
    }
    if (k < S) {
      src[k] = t;
      new_start[n_traj + k] = carry + base + incl - L;
      new_len[n_traj + k] = L;
    }
    carry += all;
  }
  if (threadIdx.x == 0) *total = carry;
}

// relabel + gather (dataset.py:370-395, :617-629): copy k = source trajectory's rows bit for bit; returns /
// cost_returns shifted so their first element is the target: fp32(fp64(x) + ((target - fp64(x[0])) [+ noise])).
__global__ __launch_bounds__(256) void aug_gather_kernel(
    const float* __restrict__ obs, const float* __restrict__ act, const float* __restrict__ rew,
    const float* __restrict__ cost, const float* __restrict__ ret, const float* __restrict__ cret, int od, int ad,
    const int64_t* __restrict__ traj_start, const int32_t* __restrict__ src, int S,
    const int64_t* __restrict__ new_start, const int32_t* __restrict__ new_len, int n_traj, const double* __restrict__ tc,
    const double* __restrict__ tr, int noise, double cstd, double rstd, const double* __restrict__ noise_c,
    const double* __restrict__ noise_r, uint64_t seed, float* __restrict__ o_obs, float* __restrict__ o_act,
    float* __restrict__ o_rew, float* __restrict__ o_cost, float* __restrict__ o_ret, float* __restrict__ o_cret) {
  const int64_t aug0 = new_start[n_traj];
  for (int k = blockIdx.x; k < S; k += gridDim.x) {
    const int t = src[k];
    const int64_t s = traj_start[t], dst = new_start[n_traj + k];
    const int L = new_len[n_traj + k];
    for (int64_t e = threadIdx.x; e < (int64_t)L * od; e += blockDim.x) o_obs[dst * od + e] = obs[s * od + e];
    for (int64_t e = threadIdx.x; e < (int64_t)L * ad; e += blockDim.x) o_act[dst * ad + e] = act[s * ad + e];
    const double dc = tc[k] - (double)cret[s], dr = tr[k] - (double)ret[s];
    for (int r = threadIdx.x; r < L; r += blockDim.x) {
      o_rew[dst + r] = rew[s + r];
      o_cost[dst + r] = cost[s + r];
      double ac = dc, ar = dr;
      if (noise) {
        const int64_t row = dst + r - aug0;  // row of the augmented part
        double nc, nr;
        if (noise_c) {
          nc = noise_c[row];
          nr = noise_r[row];
        } else {  // Box-Muller on two Philox doubles per value
          const U4 w = aug_words(kDrawNoise, (uint64_t)row, seed);
          const double u1 = 1.0 - u53(w.x, w.y), u2 = u53(w.z, w.w);
          const double rad = sqrt(-2.0 * log(u1));
          nc = 0.0 + cstd * (rad * cos(6.283185307179586 * u2));
          nr = 0.0 + rstd * (rad * sin(6.283185307179586 * u2));
        }
        ac = dc + nc;
        ar = dr + nr;
      }
      o_cret[dst + r] = (float)((double)cret[s + r] + ac);
      o_ret[dst + r] = (float)((double)ret[s + r] + ar);
    }
  }
}

// process_bc_dataset's frontier band (dataset.py:91-93): keep iff pf(cr) - band <= rr <= pf(cr) + band with
// band = (rmax - rmin) / 5; written as 0 (keep) / 1 (drop) for osrl_bc_select's SAFE compaction at 0.5
__global__ void bc_frontier_mask_kernel(const float* __restrict__ cr, const float* __restrict__ rr, int64_t n,
                                        const double* __restrict__ coef, const int32_t* __restrict__ deg,
                                        const double* __restrict__ stats, float* __restrict__ mask) {
  const int d = *deg;
  double cf[kMaxCoef];
  for (int k = 0; k <= d; ++k) cf[k] = coef[k];
  const double band = (stats[3] - stats[4]) / 5.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double pf = horner(cf, d, (double)cr[i]);
    const double r = (double)rr[i];
    mask[i] = (pf - band <= r && r <= pf + band) ? 0.f : 1.f;
  }
}

// compute_sample_prob (dataset.py:399-436): w_i = 1 / (distance of trajectory i's (cost return, return) to the
// frontier + beta), the distance as pf_dist.h defines it (the stationary point downhill from the cost return, not the
// nearest point).  One thread per trajectory, fp64; the per-thread tables of the root isolation live in an LDS slice
// [slot][thread] (consecutive threads hit consecutive banks), so nothing is indexed dynamically in registers.
constexpr int kPfThreads = 64;

__global__ __launch_bounds__(kPfThreads) void pf_dist_kernel(const float* __restrict__ ret,
                                                             const float* __restrict__ cret,
                                                             const int64_t* __restrict__ start, int n,
                                                             const double* __restrict__ coef,
                                                             const int32_t* __restrict__ deg, double beta,
                                                             double* __restrict__ w, double* __restrict__ dist) {
  __shared__ double tab[osrl_pf::kSlots][kPfThreads];
  __shared__ double cf[kMaxCoef];
  __shared__ int lead;
  if (threadIdx.x == 0) {  // leading zeros stripped, as np.poly1d does
    const int d = min(max(*deg, 0), kMaxCoef - 1);
    int z = 0;
    while (z < d && coef[z] == 0.0) ++z;
    lead = z;
    for (int k = 0; k < kMaxCoef; ++k) cf[k] = k + z <= d ? coef[k + z] : 0.0;
  }
  __syncthreads();
  const int d = min(max(*deg, 0), kMaxCoef - 1) - lead;
  const int i = blockIdx.x * kPfThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t s = start[i];
  const double c = (double)cret[s], r = (double)ret[s];
  const double dd = osrl_pf::pf_distance(cf, d, c, r, &tab[0][threadIdx.x], kPfThreads);
  w[i] = 1.0 / (dd + beta);
  if (dist) dist[i] = dd;
}

// prob = max(w, 0) / sum, cdf = inclusive running sum / sum, from fp64 weights: one workgroup, every thread a
// contiguous chunk, the chunk totals scanned in LDS -- a fixed order of additions, so the result is the same bits on
// every run.  (The layout of ingest.hip's cost_sample_prob_kernel, on weights computed elsewhere.)
__global__ __launch_bounds__(kWg) void weights_prob_kernel(const double* __restrict__ w, int n,
                                                           float* __restrict__ prob, float* __restrict__ cdf) {
  __shared__ double part[kWg];
  const int chunk = (n + kWg - 1) / kWg;
  const int e0 = min(n, (int)threadIdx.x * chunk), e1 = min(n, e0 + chunk);
  auto weight = [&](int e) {
    const double v = w[e];
    return v > 0.0 ? v : 0.0;
  };
  double mine = 0.0;
  for (int e = e0; e < e1; ++e) mine += weight(e);
  part[threadIdx.x] = mine;
  __syncthreads();
  for (int o = 1; o < kWg; o <<= 1) {  // inclusive Hillis-Steele scan
    const double t = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0.0;
    __syncthreads();
    part[threadIdx.x] += t;
    __syncthreads();
  }
  const double total = part[kWg - 1];
  double run = part[threadIdx.x] - mine;
  for (int e = e0; e < e1; ++e) {
    const double v = weight(e);
    run += v;
    prob[e] = (float)(v / total);
    if (cdf) cdf[e] = (float)(run / total);
  }
}

inline int grid_for(int64_t n, int threads) {
  const int64_t g = (n + threads - 1) / threads;
  return (int)(g < 1 ? 1 : (g > 65535 ? 65535 : g));
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int osrl_traj_returns(const float* ret, const float* cret, const int64_t* traj_start, int32_t n_traj,
                                 double* r0, double* c0, void* stream) {
  if (n_traj == 0) return 0;
  if (!ret || !cret || !traj_start || !r0 || !c0 || n_traj < 0) return -1;
  (void)hipGetLastError();
  hipLaunchKernelGGL(traj_returns_kernel, dim3((n_traj + 255) / 256), dim3(256), 0, S_, ret, cret, traj_start, n_traj,
                     r0, c0);
  return (int)hipGetLastError();
}

extern "C" int64_t osrl_grid_filter_ws_elems(int64_t n) { return (3 * n + 1) / 2 + 64; }

extern "C" int osrl_grid_filter(const double* x, const double* y, int32_t n, int32_t xbins, int32_t ybins,
                                int32_t max_per_bin, int32_t min_per_bin, const int32_t* pick_in, uint64_t seed,
                                int32_t* filt, double* fx, double* fy, int32_t* count, void* ws, void* stream) {
  if (!x || !y || n < 1 || n > (1 << 20) || xbins < 1 || ybins < 1 || (int64_t)(xbins + 1) * (ybins + 1) > kMaxBins ||
      max_per_bin < 1 || max_per_bin > kMaxPerBin || min_per_bin < 0 || !filt || !fx || !fy || !count || !ws)
    return -1;
  int32_t* w = (int32_t*)ws;
  (void)hipGetLastError();
  hipLaunchKernelGGL(grid_filter_kernel, dim3(1), dim3(kWg), 0, S_, x, y, n, xbins, ybins, max_per_bin, min_per_bin,
                     pick_in, seed, w, w + n, w + 2 * n, filt, fx, fy, count);
  return (int)hipGetLastError();
}

extern "C" int osrl_pareto_mask(const double* c, const double* r, int32_t n, int32_t* flag, void* stream) {
  if (!c || !r || !flag || n < 1 || n > (1 << 20)) return -1;
  (void)hipGetLastError();
  hipLaunchKernelGGL(pareto_mask_kernel, dim3((n + 255) / 256), dim3(256), 0, S_, c, r, n, flag);
  return (int)hipGetLastError();
}

extern "C" int64_t osrl_polyfit_ws_elems(int64_t n, int32_t deg) { return n * (int64_t)(deg + 3) + 64; }

extern "C" int osrl_polyfit(const double* x, const double* y, const int32_t* flag, int32_t n, int32_t deg, int32_t pick,
                            double* coef, int32_t* deg_out, int32_t* pidx, int32_t* pcount, double* stats, void* ws,
                            void* stream) {
  if (pick) deg = 2;
  if (!x || !y || n < 1 || n > (1 << 20) || deg < 0 || deg >= kMaxCoef || !coef || !deg_out || !pidx || !pcount ||
      !stats || !ws)
    return -1;
  double* w = (double*)ws;
  (void)hipGetLastError();
  hipLaunchKernelGGL(polyfit_kernel, dim3(1), dim3(kWg), 0, S_, x, y, flag, n, deg, pick, coef, deg_out, pidx, pcount,
                     stats, w, w + n, w + 2 * (int64_t)n);
  return (int)hipGetLastError();
}

extern "C" int64_t osrl_augment_targets_ws_elems(int64_t F, int64_t S) {
  (void)F;
  return 2 * S + 64;  // near_raw, out_off, draw_off, count: [S] int32 each
}

extern "C" int osrl_augment_targets(const double* coef, const int32_t* deg, const double* fx, const double* fy,
                                    int32_t F, int32_t S, double min_reward, double max_reward,
                                    double max_rew_decrease, double beta, const double* u_rew, const double* u_part,
                                    uint64_t seed, double* tc, double* tr, int32_t* nearest, void* ws, void* stream) {
  if (S == 0) return 0;
  // the counts live in LDS ([2 F] ints) and so does one partner cdf ([F] doubles): F <= 8000 (the 10 x 50 filter
  // keeps at most 5610)
  if (!coef || !deg || !fx || !fy || F < 1 || F > 8000 || S < 0 || !tc || !tr || !nearest || !ws) return -1;
  int32_t* w = (int32_t*)ws;
  int32_t *near_raw = w, *out_off = w + S, *draw_off = w + 2 * (int64_t)S, *kc = w + 3 * (int64_t)S;
  (void)hipGetLastError();
  hipLaunchKernelGGL(aug_targets_kernel, dim3((S + 255) / 256), dim3(256), 0, S_, coef, deg, fx, fy, F, S, min_reward,
                     max_reward, u_rew, seed, tc, tr, near_raw);
  hipLaunchKernelGGL(aug_dups_kernel, dim3(1), dim3(kWg), 2 * F * sizeof(int), S_, near_raw, F, S, nearest, out_off,
                     draw_off, kc);
  hipLaunchKernelGGL(aug_partners_kernel, dim3(S), dim3(256), F * sizeof(double), S_, fx, fy, F, near_raw, out_off,
                     draw_off, kc, max_rew_decrease, beta, u_part, seed, nearest);
  return (int)hipGetLastError();
}

extern "C" int osrl_random_aug_targets(const double* c0, const double* r0, int32_t n, int32_t S, double aug_cmin,
                                       double aug_cmax, double aug_rmin, double aug_rmax, double cgap,
                                       const double* u_cr, uint64_t seed, double* tc, double* tr, int32_t* nearest,
                                       void* stream) {
  if (S == 0) return 0;
  if (!c0 || !r0 || n < 1 || S < 0 || !tc || !tr || !nearest) return -1;
  (void)hipGetLastError();
  hipLaunchKernelGGL(rand_targets_kernel, dim3((S + 255) / 256), dim3(256), 0, S_, c0, r0, n, S, aug_cmin, aug_cmax,
                     aug_rmin, aug_rmax, cgap, u_cr, seed, tc, tr, nearest);
  return (int)hipGetLastError();
}

extern "C" int osrl_augment_layout(const int32_t* nearest, const int32_t* map, int32_t S, const int64_t* traj_start,
                                   const int32_t* traj_len, int32_t n_traj, int64_t n_rows, int64_t* new_start,
                                   int32_t* new_len, int32_t* src, int64_t* total, void* stream) {
  if (!traj_start || !traj_len || n_traj < 1 || S < 0 || (S > 0 && (!nearest || !src)) || !new_start || !new_len ||
      !total)
    return -1;
  (void)hipGetLastError();
  hipLaunchKernelGGL(aug_layout_kernel, dim3(1), dim3(kWg), 0, S_, nearest, map, S, traj_start, traj_len, n_traj,
                     n_rows, new_start, new_len, src, total);
  return (int)hipGetLastError();
}

extern "C" int osrl_augment_gather(const float* obs, const float* act, const float* rew, const float* cost,
                                   const float* ret, const float* cret, int32_t od, int32_t ad,
                                   const int64_t* traj_start, const int32_t* src, int32_t S, const int64_t* new_start,
                                   const int32_t* new_len, int32_t n_traj, const double* tc, const double* tr,
                                   int32_t noise, double cstd, double rstd, const double* noise_c,
                                   const double* noise_r, uint64_t seed, float* o_obs, float* o_act, float* o_rew,
                                   float* o_cost, float* o_ret, float* o_cret, void* stream) {
  if (S == 0) return 0;
  if (!obs || !act || !rew || !cost || !ret || !cret || od < 1 || ad < 1 || !traj_start || !src || S < 0 ||
      !new_start || !new_len || n_traj < 1 || !tc || !tr || (!noise_c) != (!noise_r) || !o_obs || !o_act || !o_rew ||
      !o_cost || !o_ret || !o_cret)
    return -1;
  (void)hipGetLastError();
  hipLaunchKernelGGL(aug_gather_kernel, dim3(grid_for(S, 1)), dim3(256), 0, S_, obs, act, rew, cost, ret, cret, od, ad,
                     traj_start, src, S, new_start, new_len, n_traj, tc, tr, noise, cstd, rstd, noise_c, noise_r, seed,
                     o_obs, o_act, o_rew, o_cost, o_ret, o_cret);
  return (int)hipGetLastError();
}

extern "C" int osrl_weights_sample_prob(const double* weights, int32_t n, float* prob, float* cdf, void* stream) {
  if (!weights || !prob || n < 1 || n > (1 << 20)) return -1;
  (void)hipGetLastError();
  hipLaunchKernelGGL(weights_prob_kernel, dim3(1), dim3(kWg), 0, S_, weights, n, prob, cdf);
  return (int)hipGetLastError();
}

extern "C" int osrl_pf_sample_prob(const float* returns, const float* cost_returns, const int64_t* traj_start,
                                   int32_t n_traj, const double* coef, const int32_t* deg, double beta, float* prob,
                                   float* cdf, double* dist, double* ws, void* stream) {
  if (!returns || !cost_returns || !traj_start || n_traj < 1 || n_traj > (1 << 20) || !coef || !deg || !(beta > 0.0) ||
      !prob || !ws)
    return -1;
  (void)hipGetLastError();
  hipLaunchKernelGGL(pf_dist_kernel, dim3((n_traj + kPfThreads - 1) / kPfThreads), dim3(kPfThreads), 0, S_, returns,
                     cost_returns, traj_start, n_traj, coef, deg, beta, ws, dist);
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  return osrl_weights_sample_prob(ws, n_traj, prob, cdf, stream);
}

extern "C" int osrl_bc_frontier_select(const float* cost_returns, const float* rew_returns, int64_t n,
                                       const double* coef, const int32_t* deg, const double* stats, float* mask,
                                       int64_t* idx, int32_t* n_keep, int32_t* ws, void* stream) {
  if (!cost_returns || !rew_returns || n < 1 || n >= (int64_t)1 << 31 || !coef || !deg || !stats || !mask || !idx ||
      !n_keep || !ws)
    return -1;
  (void)hipGetLastError();
  hipLaunchKernelGGL(bc_frontier_mask_kernel, dim3(grid_for(n, 256)), dim3(256), 0, S_, cost_returns, rew_returns, n,
                     coef, deg, stats, mask);
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  return osrl_bc_select(mask, n, OSRL_BC_SAFE, 0.5f, 0.f, idx, n_keep, ws, stream);
}
