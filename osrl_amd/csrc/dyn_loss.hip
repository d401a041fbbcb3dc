// dyn_loss.hip -- osrl_dyn_member_loss: the dynamics ensemble's per-member loss as a launch of its own.
//
// One launch turns the members' forward outputs y [n_nets, rows, NL] and the target table [rows, od + 2] into any of
//   dy          the output gradient of every member, each row scaled by that member's bootstrap weight,
//   row_loss    the unweighted per-row loss l_m(r)                                  (holdout loss: DynamicsTrainer.validate),
//   stat        stat_scale * sum_{m, r} w_m(r) l_m(r)                               (the logged statistic),
// with the arithmetic of the seeded backward launch (mlp.hip, OSRL_SEED_MSE / OSRL_SEED_GAUSS_NLL): both call the terms of
// loss_terms.h.  The bootstrap weight w_m(r) is a Poisson(1) count that belongs to the STORE ROW
// idx[r] and the member m: word x of Philox4x32-10(counter {idx[r], m, 0, 17}, key *boot_seed) against the cumulative
// table kBootT, so every member trains on one fixed resample of the dataset (include/osrl_amd.h).
//
// Shape: one wave per row, kRows rows per workgroup.  Lane j owns the target columns k = j, j + 64, .. of its row, loads
// them ONCE and reuses them for every member; per member it reads y[k] (and, Gaussian, y[od + 2 + k]) and writes the
// matching dy words -- every access is contiguous along the columns.  The row's loss is each lane's terms in column
// order, then the 64-lane butterfly: a row's dy, row_loss and weight depend on nothing but the row itself.  The statistic
// is the fixed-order sum of one partial per workgroup, taken by the last workgroup to arrive (device-coherent words, one
// arrival atomic per workgroup, no floating-point atomics): the same inputs give the same bits.  The kernel reads neither
// blockDim nor gridDim (the library is built with kernarg preload), uses no scratch and 20 bytes of static LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/osrl_amd.h"
#include "argmem.h"
#include "dev_util.h"
#include "loss_terms.h"
#include "philox.h"

namespace {

using osrl_rng::philox4x32_10;
using osrl_rng::U4;

constexpr int kRows = OSRL_DYN_LOSS_TILE;  // rows (= waves) per workgroup
constexpr int kThreads = 64 * kRows;
constexpr int kColsPerLane = (OSRL_MODEL_ENV_MAX_STATE + 2 + 63) / 64;  // target columns a lane owns (5 at od = 256)
constexpr uint32_t kBootStream = 17;  // Philox stream of the bootstrap weights (13 .. 16: exploration, member, branch, sample)

// T_k = floor(2^32 sum_{j <= k} e^-1 / j!), k = 0 .. 7, evaluated in fp64: w = #{k : word >= T_k} is Poisson(1) cut at 8
__device__ __forceinline__ float boot_weight(uint32_t word) {
  constexpr uint32_t kBootT[8] = {1580030168u, 3160060337u, 3950075421u, 4213413783u,
                                  4279248373u, 4292415291u, 4294609777u, 4294923276u};
  int w = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) w += word >= kBootT[k] ? 1 : 0;
  return (float)w;
}

// AR = how the descriptor is reached: `const osrl_dyn_loss_t&` (the kernarg segment) or the OSRL_CAS form (argmem.h)
template <class AR>
__device__ __forceinline__ void dyn_loss_body(AR a) {
  __shared__ float s_part[kRows];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rows = a.rows, n_nets = a.n_nets;
  const int no = a.state_dim + 2;  // the target's width; Gaussian: the first log-variance column
  const bool gauss = a.kind == OSRL_DYN_LOSS_GAUSS_NLL;
  const int NL = gauss ? 2 * no - 1 : no;
  const float lo = a.lo, hi = a.hi, scale = a.scale;
  const int r = (int)blockIdx.x * kRows + wave;  // wave-uniform
  float wsum = 0.f;                              // sum_m w_m(r) l_m(r)
  if (r < rows) {
    float wv = 1.0f;  // lane m (< 8) holds w_m(r)
    if (a.idx) {
      const uint64_t seed = *a.boot_seed;
      const U4 p = philox4x32_10(U4{(uint32_t)a.idx[r], (uint32_t)(lane & 7), 0u, kBootStream}, (uint32_t)seed,
                                 (uint32_t)(seed >> 32));
      wv = boot_weight(p.x);
    }
    if (a.weights_out && lane < n_nets) a.weights_out[(size_t)lane * rows + r] = wv;
    float t[kColsPerLane];
#pragma unroll
    for (int j = 0; j < kColsPerLane; ++j) {
      const int k = lane + 64 * j;
      t[j] = k < no ? a.target[(size_t)r * no + k] : 0.f;
    }
    for (int m = 0; m < n_nets; ++m) {
      const float w = __shfl(wv, m);
      const size_t base = ((size_t)m * rows + r) * NL;
      const float* __restrict__ y = a.y + base;
      float* __restrict__ dy = a.dy ? a.dy + base : nullptr;
      float l = 0.f;
#pragma unroll
      for (int j = 0; j < kColsPerLane; ++j) {
        if (64 * j >= no) break;  // wave-uniform
        const int k = lane + 64 * j;
        if (k < no) {
          const float d = y[k] - t[j];
          if (!gauss || k == no - 1) {  // MSE; the Gaussian's raw cost column
            l += sq_term(d);
            const float g = sq_grad(d, scale);
            if (dy) dy[k] = w == 0.f ? 0.f : g * w;
          } else {
            const float raw = y[no + k];
            const LogVar v = gauss_nll_logvar(raw, lo, hi);
            l += gauss_nll_term(d, v);
            const float g = gauss_nll_g_mean(d, v, scale);
            const float gv = gauss_nll_g_raw(d, raw, v, lo, hi, scale);
            if (dy) {
              dy[k] = w == 0.f ? 0.f : g * w;
              dy[no + k] = w == 0.f ? 0.f : gv * w;
            }
          }
        }
      }
      l = wave_sum(l);
      if (a.row_loss && lane == 0) a.row_loss[(size_t)m * rows + r] = l;
      wsum += w == 0.f ? 0.f : w * l;
    }
  }
  if (!a.stat) return;  // (uniform over the launch)
  // the statistic: waves in order into this workgroup's partial, then the last workgroup to arrive sums every partial in
  // a fixed order (each lane a contiguous chunk, lanes by the butterfly, waves in order).  Wait-free.
  if (lane == 0) s_part[wave] = wsum;
  __syncthreads();
  const int n_part = (rows + kRows - 1) / kRows;
  if (tid == 0) {
    float p = 0.f;
#pragma unroll
    for (int w = 0; w < kRows; ++w) p += s_part[w];
    coh_put(a.partials + blockIdx.x, p);
    s_last = arrive_last(a.counter, n_part);  // (the partial is acknowledged before the arrival)
  }
  __syncthreads();
  if (!s_last) return;
  const int per = (n_part + kThreads - 1) / kThreads;
  float s = 0.f;
  for (int i = tid * per; i < (tid + 1) * per && i < n_part; ++i) s += coh_get(a.partials + i);
  s = wave_sum(s);
  if (lane == 0) s_part[wave] = s;  // (tid 0 read the waves' sums before the barrier that published s_last)
  __syncthreads();
  if (tid == 0) {
    float u = 0.f;
#pragma unroll
    for (int w = 0; w < kRows; ++w) u += s_part[w];
    a.stat[0] = u * a.stat_scale;
  }
}

__global__ __launch_bounds__(kThreads) void dyn_loss_kernel(const osrl_dyn_loss_t a) {
  dyn_loss_body<const osrl_dyn_loss_t&>(a);
}
__global__ __launch_bounds__(kThreads) void dyn_loss_kernel_p(const void* p) {
  dyn_loss_body<const OSRL_CAS osrl_dyn_loss_t&>(*(const OSRL_CAS osrl_dyn_loss_t*)p);
}

}  // namespace

extern "C" int osrl_dyn_member_loss(const osrl_dyn_loss_t* d, void* stream) {
  if (!d || !d->y || !d->target) return -1;
  if (d->n_nets < 1 || d->n_nets > OSRL_MAX_NETS || d->rows < 1 || d->state_dim < 1 ||
      d->state_dim > OSRL_MODEL_ENV_MAX_STATE)
    return -1;
  if (d->kind != OSRL_DYN_LOSS_MSE && d->kind != OSRL_DYN_LOSS_GAUSS_NLL) return -1;
  if (d->kind == OSRL_DYN_LOSS_GAUSS_NLL && !(d->lo < d->hi)) return -1;
  if (d->idx && !d->boot_seed) return -1;
  if (d->stat && (!d->partials || !d->counter)) return -1;
  if (!d->dy && !d->row_loss && !d->weights_out && !d->stat) return -1;  // nothing to do
  osrl_dyn_loss_t a;
  memset(&a, 0, sizeof a);  // (the arena finds a block by its bytes: no stray padding)
  a.y = d->y;
  a.target = d->target;
  a.idx = d->idx;
  a.boot_seed = d->idx ? d->boot_seed : nullptr;
  a.dy = d->dy;
  a.row_loss = d->row_loss;
  a.weights_out = d->weights_out;
  a.stat = d->stat;
  a.partials = d->stat ? d->partials : nullptr;
  a.counter = d->stat ? d->counter : nullptr;
  a.n_nets = d->n_nets;
  a.rows = d->rows;
  a.state_dim = d->state_dim;
  a.kind = d->kind;
  a.lo = d->lo;
  a.hi = d->hi;
  a.scale = d->scale;
  a.stat_scale = d->stat_scale;
  const unsigned tiles = ((unsigned)d->rows + kRows - 1) / kRows;
  return osrl_argmem::launch(dyn_loss_kernel, dyn_loss_kernel_p, dim3(tiles), dim3(kThreads), 0, (hipStream_t)stream, a);
}
