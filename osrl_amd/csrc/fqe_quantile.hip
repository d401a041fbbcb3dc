// fqe_quantile.hip -- distributional fitted Q evaluation: the quantile-Huber loss of the critics' M outputs as a launch
// of its own (osrl_fqe_quantile_loss) and the sorted-tail read-out (osrl_fqe_quantile_sums).
//
// The loss launch sits between the online forward and an unseeded backward launch, where osrl_dyn_member_loss sits in
// the bootstrap dynamics step.  theta / theta_t are [n_r + n_c, rows, M]: an ITEM is one (net, row) pair, M contiguous
// floats in both, and the launch walks the n_nets * rows items as one flat list -- one launch for every net.
//
// Loss, work split.  A wave packs R = 64 / M items (M = 2: 32 rows, M = 5: 12 rows in 60 lanes, M = 33 .. 64: one row);
// lane = slot * M + i holds theta_i of its slot's item in a register.  The same lane loads theta_t[i], the row's x and
// done, forms T_i (fqe_backup) and puts it into the wave's 64-float LDS row ONCE; the pair loop then walks j = 0 .. M - 1
// ascending with one LDS read per step, the same address in every lane of a slot (a broadcast), and keeps the two sums of
// loss_terms.h qr_pair in registers: M * M pairs per item, M per lane, no global traffic inside the loop.  Every global
// access of a wave is one contiguous run of R * M floats.  The row loss is the ascending sum over i of the lanes' terms,
// taken through a second LDS row by the slot's lane 0, so that it does not depend on where in a wave the slot lies: a
// row's dy and row_loss are functions of the row alone.  The two statistics (reward nets, cost nets): the wave's slots by
// the butterfly, the workgroup's waves in order into one pair of partials per workgroup, and the last workgroup to arrive
// (dev_util.h arrive_last) adds every pair in a fixed order -- no floating-point atomics, same inputs same bits.
//
// Read-out, work split.  One workgroup of 16 waves per net; a SEGMENT is P = 2^ceil(log2 M) adjacent lanes, 64 / P per
// wave, and owns a contiguous chunk of rows.  Per row: lanes i < M load theta_i, lanes past M hold +inf; a bitonic network
// over the segment's lanes (__shfl_xor, log2 P (log2 P + 1) / 2 compare-exchanges) leaves rank i in lane i; the M ranks are
// then read back in ascending order (M lane broadcasts) and added in fp64 -- all of them, and those of the tail (the
// k_lo smallest for a reward net, the k_hi largest for a cost net).  A segment adds its rows in order, the workgroup its
// segments in order, thread 0 / 1 add the two totals into acc.  min / max keep the multiset, so ties sort either way
// with the same sums.
//
// Neither kernel reads blockDim or gridDim (kernarg preload), neither uses scratch; static LDS only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/osrl_amd.h"
#include "argmem.h"
#include "dev_util.h"
#include "loss_terms.h"

namespace {

constexpr int kWaves = OSRL_FQE_QUANTILE_WAVES;  // waves per workgroup of the loss launch (one pair of partials each)
constexpr int kThreads = 64 * kWaves;

// AR = how the descriptor is reached: `const osrl_fqe_quantile_t&` (the kernarg segment) or the OSRL_CAS form (argmem.h)
template <class AR>
__device__ __forceinline__ void quantile_loss_body(AR a) {
  __shared__ float s_t[kWaves][64];  // T_j of the wave's items
  __shared__ float s_l[kWaves][64];  // the lanes' row-loss terms
  __shared__ float s_part[kWaves][2];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = a.M, rows = a.rows;
  const int R = 64 / M;  // items per wave
  const int n_items = (a.n_r + a.n_c) * rows;
  const int slot = lane / M, i = lane - slot * M;
  const int item = ((int)blockIdx.x * kWaves + wave) * R + slot;
  const bool ok = slot < R && item < n_items;
  const float inv_m = 1.0f / (float)M, inv_kappa = 1.0f / a.kappa, kappa = a.kappa;
  float th = 0.f, tj = 0.f;
  bool reward = true;
  if (ok) {
    const int m = item / rows, b = item - m * rows;
    reward = m < a.n_r;
    const float x = reward ? a.rew[b] : a.cost[b];
    const size_t at = (size_t)item * M + i;
    th = a.theta[at];
    tj = fqe_backup(x, a.done[b], a.theta_t[at], a.gamma);
  }
  s_t[wave][lane] = tj;
  __syncthreads();
  const int base = ok ? slot * M : 0;  // (an idle lane walks slot 0: every read stays inside the wave's row)
  const float tau = qr_tau(i, inv_m);
  QrSums s{0.f, 0.f};
  for (int j = 0; j < M; ++j) qr_pair(s, th, s_t[wave][base + j], tau, kappa);
  if (ok && a.dy) a.dy[(size_t)item * M + i] = qr_grad(s, inv_m, inv_kappa, a.scale);
  s_l[wave][lane] = qr_row_term(s, inv_m, inv_kappa);
  __syncthreads();
  float rl = 0.f;
  if (ok && i == 0) {
    for (int k = 0; k < M; ++k) rl += s_l[wave][lane + k];
    if (a.row_loss) a.row_loss[item] = rl;
  }
  if (!a.stat_r) return;  // (uniform over the launch)
  // the statistics: a wave's slots by the butterfly, waves in order into this workgroup's pair, then the last workgroup
  // to arrive adds every pair in a fixed order (each lane a contiguous chunk, lanes by the butterfly, waves in order)
  const float p0 = wave_sum(reward ? rl : 0.f), p1 = wave_sum(reward ? 0.f : rl);
  if (lane == 0) {
    s_part[wave][0] = p0;
    s_part[wave][1] = p1;
  }
  __syncthreads();
  const int per_wg = R * kWaves;
  const int n_part = (n_items + per_wg - 1) / per_wg;
  if (tid == 0) {
    float u0 = 0.f, u1 = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      u0 += s_part[w][0];
      u1 += s_part[w][1];
    }
    coh_put(a.partials + 2 * blockIdx.x, u0);
    coh_put(a.partials + 2 * blockIdx.x + 1, u1);
    s_last = arrive_last(a.counter, n_part);  // (the pair is acknowledged before the arrival)
  }
  __syncthreads();
  if (!s_last) return;
  const int per = (n_part + kThreads - 1) / kThreads;
  float t0 = 0.f, t1 = 0.f;
  for (int q = tid * per; q < (tid + 1) * per && q < n_part; ++q) {
    t0 += coh_get(a.partials + 2 * q);
    t1 += coh_get(a.partials + 2 * q + 1);
  }
  t0 = wave_sum(t0);
  t1 = wave_sum(t1);
  if (lane == 0) {  // (tid 0 read the waves' pairs before the barrier that published s_last)
    s_part[wave][0] = t0;
    s_part[wave][1] = t1;
  }
  __syncthreads();
  if (tid == 0) {
    float u0 = 0.f, u1 = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      u0 += s_part[w][0];
      u1 += s_part[w][1];
    }
    a.stat_r[0] = u0 * a.stat_scale;
    a.stat_c[0] = u1 * a.stat_scale;
  }
}

__global__ __launch_bounds__(kThreads) void quantile_loss_kernel(const osrl_fqe_quantile_t a) {
  quantile_loss_body<const osrl_fqe_quantile_t&>(a);
}
__global__ __launch_bounds__(kThreads) void quantile_loss_kernel_p(const void* p) {
  quantile_loss_body<const OSRL_CAS osrl_fqe_quantile_t&>(*(const OSRL_CAS osrl_fqe_quantile_t*)p);
}

// ---- the read-out ----------------------------------------------------------------------------------------------------
constexpr int kSumWaves = 16;
constexpr int kSumThreads = 64 * kSumWaves;
constexpr int kMaxSegs = kSumWaves * 32;  // M = 2: 32 segments per wave

__global__ __launch_bounds__(kSumThreads) void quantile_sums_kernel(const float* __restrict__ theta, int n_lo, int rows,
                                                                    int M, int log2p, int k_lo, int k_hi,
                                                                    double* __restrict__ acc) {
  __shared__ double s_seg[kMaxSegs][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int net = blockIdx.x;
  const int P = 1 << log2p, G = 64 >> log2p;  // lanes per segment, segments per wave
  const int seg = lane >> log2p, i = lane & (P - 1);
  const int sg = wave * G + seg, n_seg = kSumWaves * G;
  const int per = (rows + n_seg - 1) / n_seg;  // rows per segment: segment sg owns [sg * per, (sg + 1) * per)
  const bool low = net < n_lo;                 // a reward net: the k_lo smallest; a cost net: the k_hi largest
  const int q0 = low ? 0 : M - k_hi, q1 = low ? k_lo : M;
  const float* __restrict__ tn = theta + (size_t)net * rows * M;
  double all = 0.0, tail = 0.0;
  for (int t = 0; t < per; ++t) {  // (the same trip count in every lane: the shuffles below see whole waves)
    const int r = sg * per + t;
    const bool valid = r < rows;
    float v = (valid && i < M) ? tn[(size_t)r * M + i] : INFINITY;
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
      for (int j = k2 >> 1; j > 0; j >>= 1) {
        const float o = __shfl_xor(v, j);
        const bool keep_min = ((i & j) == 0) == ((i & k2) == 0);  // the lower lane of a pair in an ascending run
        v = keep_min ? fminf(v, o) : fmaxf(v, o);
      }
    }
    double sa = 0.0, st = 0.0;
    for (int q = 0; q < M; ++q) {  // ascending ranks
      const double x = (double)__shfl(v, (seg << log2p) + q);
      sa += x;
      if (q >= q0 && q < q1) st += x;
    }
    if (valid) {
      all += sa;
      tail += st;
    }
  }
  if (i == 0) {
    s_seg[sg][0] = all;
    s_seg[sg][1] = tail;
  }
  __syncthreads();
  if (tid < 2) {
    double u = 0.0;
    for (int s = 0; s < n_seg; ++s) u += s_seg[s][tid];
    acc[2 * net + tid] += u;
  }
}

}  // namespace

extern "C" int osrl_fqe_quantile_loss(const osrl_fqe_quantile_t* d, void* stream) {
  if (!d || !d->theta || !d->theta_t || !d->rew || !d->cost || !d->done) return -1;
  if (d->n_r < 0 || d->n_c < 0 || d->n_r + d->n_c < 1 || d->n_r + d->n_c > OSRL_MAX_NETS || d->rows < 1) return -1;
  if (d->M < 2 || d->M > OSRL_FQE_MAX_QUANTILES || !(d->kappa > 0.f)) return -1;
  if (!d->stat_r != !d->stat_c) return -1;
  if (d->stat_r && (!d->partials || !d->counter)) return -1;
  if (!d->dy && !d->row_loss && !d->stat_r) return -1;  // nothing to do
  if ((int64_t)(d->n_r + d->n_c) * d->rows > INT32_MAX / OSRL_FQE_MAX_QUANTILES) return -1;
  osrl_fqe_quantile_t a;
  memset(&a, 0, sizeof a);  // (the arena finds a block by its bytes: no stray padding)
  a.theta = d->theta;
  a.theta_t = d->theta_t;
  a.rew = d->rew;
  a.cost = d->cost;
  a.done = d->done;
  a.dy = d->dy;
  a.row_loss = d->row_loss;
  a.stat_r = d->stat_r;
  a.stat_c = d->stat_c;
  a.partials = d->stat_r ? d->partials : nullptr;
  a.counter = d->stat_r ? d->counter : nullptr;
  a.n_r = d->n_r;
  a.n_c = d->n_c;
  a.rows = d->rows;
  a.M = d->M;
  a.gamma = d->gamma;
  a.kappa = d->kappa;
  a.scale = d->scale;
  a.stat_scale = d->stat_scale;
  const unsigned per_wg = (unsigned)(64 / d->M) * kWaves;
  const unsigned n_items = (unsigned)(d->n_r + d->n_c) * (unsigned)d->rows;
  return osrl_argmem::launch(quantile_loss_kernel, quantile_loss_kernel_p, dim3((n_items + per_wg - 1) / per_wg),
                             dim3(kThreads), 0, (hipStream_t)stream, a);
}

extern "C" int osrl_fqe_quantile_sums(const float* theta, int32_t n_nets, int32_t n_lo, int32_t rows, int32_t M,
                                      int32_t k_lo, int32_t k_hi, double* acc, void* stream) {
  if (!theta || !acc || n_nets < 1 || n_nets > OSRL_MAX_NETS || n_lo < 0 || n_lo > n_nets || rows < 1) return -1;
  if (M < 2 || M > OSRL_FQE_MAX_QUANTILES || k_lo < 1 || k_lo > M || k_hi < 1 || k_hi > M) return -1;
  int log2p = 1;
  while ((1 << log2p) < M) ++log2p;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(quantile_sums_kernel, dim3(n_nets), dim3(kSumThreads), 0, (hipStream_t)stream, theta, n_lo, rows, M,
                     log2p, k_lo, k_hi, acc);
  return (int)hipGetLastError();
}
