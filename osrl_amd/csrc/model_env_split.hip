// model_env_split.hip -- osrl_model_env_step_split: the learned-dynamics environment step (model_env.hip) with one
// workgroup per 16-episode tile AND ensemble member, for launches of a few tiles -- a planner's N * K candidates -- where
// model_env.hip's one workgroup per tile leaves the chip idle while it walks M * n_layers layers one after the other.
//
// Grid (tiles, M), 512 threads.  Workgroup (tile, m):
//   1. stages the tile's rows and inputs exactly as model_env.hip does (liveness, the member draw, normalisation, the
//      recorded exploration noise, the clip): a function of global memory only, so the M workgroups of a tile hold the
//      same xin bits;
//   2. runs member m's layers with the same mfma_layer (lane layout, k order, kC = 4), activations ping-pong in LDS;
//   3. writes its output tile to member_out[tile][m][16][W] (W = OSRL_MODEL_ENV_SPLIT_ROW): the od + 2 output columns
//      and, Gaussian, the od + 1 values sigma^2 and the row's sqrt(sum_{k < od} sigma^2 / od) -- device-coherent vector
//      stores (dev_util.h coh_put: the M workgroups sit on different XCDs);
//   4. waits for its own stores and signs in on arrive[tile] (dev_util.h arrive_last_acked, dyn_loss.hip's and
//      mlp_dw.hip's protocol).  Wait-free: a workgroup is the last of the tile's M to arrive, or it returns.  The sign-in
//      of the last one stores 0 to arrive[tile]: the word is zero between launches, a captured graph replays without a
//      memset;
//   5. the last one reads the M member tiles back in ascending m (coh_get) and rebuilds what model_env.hip holds after
//      its member loop -- ysum as y0, + y1, .., ysel, yk[m][q] in registers, the variance tile in member order, amax as
//      the same fmaxf chain -- then runs the same epilogue.  Nobody writes state, acc or the tables before every member
//      of the tile has signed in, i.e. has staged its inputs.
// Every device expression below is model_env.hip's, restated: sharing them through a header moved that file's registers
// (198 -> 204), so it stays as it is and tests/test_gpu_model_env_split.py holds the two together bit for bit.  Only the
// host side -- the descriptor pieces and their checks -- is shared, through model_env_args.h.  The serial chain
// is n_layers long instead of M * n_layers; the price is M times the staging and one trip of the member tiles through
// HBM, which loses once the plain form fills the chip (README: the measured crossover).  The kernels read neither
// blockDim nor gridDim, use no scratch, and the three compile-time flags (record, Gaussian, pessimistic) are template
// parameters of one body: eight kernels, each with its descriptor-pointer twin (argmem.h).
#include "argmem.h"
#include "dev_util.h"
#include "model_env_args.h"
#include "policy_common.h"
#include "rollout_step.h"

using osrl_rng::philox4x32_10;
using osrl_rng::U4;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 512, kWaves = 8, kTile = 16;
constexpr int kPad = 4;  // floats: rows 16 bytes apart in the banks (act_vec.hip)
constexpr int kS = OSRL_MODEL_ENV_MAX_WIDTH + kPad;         // row stride of the activation tiles
constexpr int kYS = OSRL_MODEL_ENV_MAX_STATE + 2 + 2;       // row stride of the output tiles (state_dim + 2 columns)
constexpr int kRowThreads = kThreads / kTile;               // 32 threads share a row in the epilogue
constexpr int kKeep = OSRL_MODEL_ENV_MAX_STATE / kRowThreads;  // state columns a thread keeps per member
constexpr uint32_t kMemberStream = 14;                      // Philox stream of the RANDOM-mode member choice

constexpr uint32_t kGaussStream = 16;  // Philox stream of the sampled next state and reward

// (Gaussian step) beside Lds: 132 KB + 16.3 KB of the 160 KB
struct LdsGauss {
  float v[kTile * kYS];  // sigma^2 per row and column k < od + 1: the members' sum (MEAN) or the followed member's
  int step[kTile];       // the episode's own step: the noise is keyed by it
};

struct Lds {
  __attribute__((aligned(16))) float xin[kTile * kS];     // the staged input rows: every member's layer 0 reads them
  __attribute__((aligned(16))) float buf[2][kTile * kS];  // a member's activations, ping-pong
  float ysum[kTile * kYS];                                // sum over the members so far, then the mean
  float ysel[kTile * kYS];                                // the output of the member the row follows
  int live[kTile];                                        // 1: the row's episode exists and is not finished
  int jsel[kTile];                                        // the member the row follows (-1: the mean)
  int step[kTile];                                        // (recording) the episode's own step: its table row
  float sig[kTile];                                       // (recording) the row's noise scale
};
static_assert(sizeof(Lds) + sizeof(LdsGauss) <= 160 * 1024, "menv_split_kernel: LDS per workgroup");

// y[r][n] = act(b[n] + sum_k W[n][k] x[r][k]) for the tile's 16 rows (act_vec.hip mfma_layer: the same lane layout, the same
// k order); x, y in LDS, row stride kS.  Columns out .. round16(out) are written as zero: the next layer's k padding.
__device__ __forceinline__ void mfma_layer(const float* __restrict__ PF, const float* __restrict__ b, int in, int out,
                                           int act, const float* x, float* y) {
  // (act_vec.hip runs 8 k-blocks per round; beside the 64 kept output registers that spills: 256 VGPRs + 18 in scratch
  // against 198 and none at 4)
  constexpr int kC = 4;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ar = lane & 15, kq = lane >> 4;
  const int Np = round16(out), nkb = round16(in) >> 4, nct = Np >> 4;
  const f32x4* __restrict__ W4 = reinterpret_cast<const f32x4*>(PF);
  const float* xr = x + ar * kS + 4 * kq;
  for (int c0 = w; c0 < nct; c0 += 2 * kWaves) {
    const int c1 = c0 + kWaves;
    const bool two = c1 < nct;  // (wave-uniform)
    const f32x4* __restrict__ p0 = W4 + (size_t)kq * Np + 16 * c0 + ar;
    const f32x4* __restrict__ p1 = W4 + (size_t)kq * Np + 16 * (two ? c1 : c0) + ar;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < nkb; kc += kC) {  // kC k-blocks per round: every load of the round before its first MFMA
      f32x4 b0[kC], b1[kC], av[kC];
#pragma unroll
      for (int u = 0; u < kC; ++u) {
        const int kb = kc + u;
        b0[u] = b1[u] = av[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kb < nkb) {
          b0[u] = p0[(size_t)4 * kb * Np];
          if (two) b1[u] = p1[(size_t)4 * kb * Np];
          av[u] = *reinterpret_cast<const f32x4*>(xr + 16 * kb);
        }
      }
#pragma unroll
      for (int u = 0; u < kC; ++u) {
        if (kc + u < nkb) {
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][t], b0[u][t], acc0, 0, 0, 0);
            if (two) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][t], b1[u][t], acc1, 0, 0, 0);
          }
        }
      }
    }
    {
      const int col = 16 * c0 + ar;
      const float bb = col < out ? b[col] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) y[(4 * kq + i) * kS + col] = col < out ? act_fwd(act, acc0[i] + bb) : 0.f;
    }
    if (two) {
      const int col = 16 * c1 + ar;
      const float bb = col < out ? b[col] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) y[(4 * kq + i) * kS + col] = col < out ? act_fwd(act, acc1[i] + bb) : 0.f;
    }
  }
  __syncthreads();
}

// The three stages below are model_env.hip's model_env_body cut at its member loop, with its template parameters, always
// given explicitly: AR, RR, GR and PR are reference types, and deducing them would copy the descriptor.

// ---- the tile's rows: which are live, at which step, which member each follows.  Ends with a barrier.
template <bool kRecord, bool kGauss, class AR, class RR>
__device__ __forceinline__ void stage_rows(AR a, RR rc, Lds& l, LdsGauss* lg) {
  const int tid = threadIdx.x;
  const int M = a.d.n_models;
  const int e0 = blockIdx.x * kTile;  // the tile's first episode
  if (tid < kTile) {
    const int e = e0 + tid;
    bool lv = e < a.episodes;
    int st = 0;
    if constexpr (kRecord) {  // the step is read once, here: the member draw, the noise and the table row all use it
      lv = lv && osrl_rollout::live_step(a.acc + (size_t)e * 4, a.d.episode_len, st);
      l.step[tid] = st;
      l.sig[tid] = lv ? rc.c.sigma[e] : 0.f;
    } else {
      lv = lv && a.acc[(size_t)e * 4 + 3] == 0.f;
    }
    int js = -1;
    if (lv && a.d.mode == OSRL_MODEL_ENV_MEMBER) js = a.d.member;
    if (lv && a.d.mode == OSRL_MODEL_ENV_RANDOM) {
      if (a.d.member_in) {
        js = (int)((uint32_t)a.d.member_in[e] % (uint32_t)M);
      } else {
        const uint64_t seed = *a.d.seed;
        const uint32_t t = kRecord ? (uint32_t)st : (uint32_t)a.acc[(size_t)e * 4 + 2];
        const U4 w = philox4x32_10(U4{a.d.episode_base + (uint32_t)e, t, 0u, kMemberStream}, (uint32_t)seed,
                                   (uint32_t)(seed >> 32));
        js = (int)(w.x % (uint32_t)M);
      }
    }
    l.live[tid] = lv;
    l.jsel[tid] = js;
    if constexpr (kGauss) lg->step[tid] = kRecord ? st : (lv ? (int)a.acc[(size_t)e * 4 + 2] : 0);
  }
  __syncthreads();
}

// ---- the state columns this thread advances at the end, and the staged input rows; idle rows are zero.  Ends with a
// barrier.
template <bool kRecord, class AR, class RR>
__device__ __forceinline__ void stage_inputs(AR a, RR rc, Lds& l, float (&sreg)[kKeep]) {
  const int tid = threadIdx.x;
  const int od = a.d.state_dim, ad = a.d.action_dim;
  const int e0 = blockIdx.x * kTile;
  const int r = tid / kRowThreads, j = tid % kRowThreads;
  const bool alive = l.live[r] != 0;
  const int ep = e0 + r;
#pragma unroll
  for (int q = 0; q < kKeep; ++q) {
    const int k = j + kRowThreads * q;
    sreg[q] = alive && k < od ? a.state[(size_t)ep * od + k] : 0.f;
  }
  const int in0 = round16(od + ad);
  for (int i = tid; i < kTile * in0; i += kThreads) {
    const int rr = i / in0, c = i - rr * in0, e = e0 + rr;
    float v = 0.f;
    if (l.live[rr]) {
      if (c < od)
        v = (a.state[(size_t)e * od + c] - a.d.mu_s[c]) / a.d.sd_s[c];
      else if (c < od + ad) {
        v = a.act[(size_t)e * ad + (c - od)];
        if constexpr (kRecord) {
          v = osrl_rollout::explore(v, l.sig[rr], [&] {
            const int k = c - od, st = l.step[rr];
            return osrl_rollout::explore_eps(rc.c, e, st, k, ((size_t)st * a.episodes + e) * ad + k);
          });
        }
        v = fminf(fmaxf(v, -a.d.max_action), a.d.max_action);
      }
    }
    l.xin[rr * kS + c] = v;
  }
  __syncthreads();
}

// ---- from the members' outputs to the step's stores.  On entry l.ysum holds the members' sum (y0, + y1, .. in that
// order), l.ysel the followed member's row, yk[m][q] member m's state column j + 32 q of this thread's row, (Gaussian) lg->v
// the variance tile and amax the running max_m rms(sigma_m); every thread has written its own elements only.
template <bool kRecord, bool kGauss, bool kPess, class AR, class RR, class GR, class PR>
__device__ __forceinline__ void step_epilogue(AR a, RR rc, Lds& l, GR g, LdsGauss* lg, PR ps, const float (&sreg)[kKeep],
                                              const float (&yk)[OSRL_MAX_NETS][kKeep], float amax) {
  const int tid = threadIdx.x;
  const int od = a.d.state_dim, ad = a.d.action_dim, M = a.d.n_models, no = od + 2;
  const int e0 = blockIdx.x * kTile;
  const int r = tid / kRowThreads, j = tid % kRowThreads;
  const bool alive = l.live[r] != 0;
  const int ep = e0 + r;
  const float inv_m = 1.0f / (float)M;
  for (int i = tid; i < kTile * no; i += kThreads) {
    const int rr = i / no, c = i - rr * no;
    l.ysum[rr * kYS + c] *= inv_m;
  }
  __syncthreads();
  // ---- disagreement: the row's 32 threads hold its state columns; a butterfly over them gives every one the sum
  const float* ybar = l.ysum + r * kYS;
  float d = 0.f;
#pragma unroll
  for (int m = 0; m < OSRL_MAX_NETS; ++m) {
    if (m < M) {
      float p = 0.f;
#pragma unroll
      for (int q = 0; q < kKeep; ++q) {
        const int k = j + kRowThreads * q;
        if (k < od) {
          const float df = yk[m][q] - ybar[k];
          p = fmaf(df, df, p);
        }
      }
#pragma unroll
      for (int o = kRowThreads / 2; o >= 1; o >>= 1) p += __shfl_xor(p, o);
      d = fmaxf(d, sqrtf(p / (float)od));
    }
  }
  if (!alive) return;  // finished episodes keep their state and totals
  const float* yh = (a.d.mode == OSRL_MODEL_ENV_MEAN ? l.ysum : l.ysel) + r * kYS;
  const bool clamp = a.d.s_lo != nullptr && a.d.s_hi != nullptr;
  size_t row = 0;  // (recording) the live row's: inside the tables by live_step's rule
  if constexpr (kRecord) row = (size_t)ep * a.d.episode_len + l.step[r];
  // (Gaussian) the signal in use, and column k's draw: mean + sqrt(v) eps, v the followed member's variance or the mean of all
  float u = d;
  if constexpr (kGauss) u = g.unc == OSRL_MODEL_ENV_UNC_MAX_STD ? amax : d;
  auto drawn = [&](int k, float mean) {
    if constexpr (kGauss) {
      if (g.sample) {
        float v = lg->v[r * kYS + k];
        if (a.d.mode == OSRL_MODEL_ENV_MEAN) v *= inv_m;
        uint32_t k0 = 0, k1 = 0;
        if (!g.noise_in) {
          const uint64_t seed = *a.d.seed;
          k0 = (uint32_t)seed;
          k1 = (uint32_t)(seed >> 32);
        }
        const float eps = osrl_rollout::explore_eps(a.d.episode_base + (uint32_t)ep, (uint32_t)lg->step[r], k, k0, k1,
                                                    g.noise_in, (size_t)ep * (od + 1) + k, kGaussStream);
        return fmaf(sqrtf(v), eps, mean);
      }
    }
    return mean;
  };
#pragma unroll
  for (int q = 0; q < kKeep; ++q) {
    const int k = j + kRowThreads * q;
    if (k < od) {
      float sn = sreg[q] + fmaf(a.d.sd_d[k], drawn(k, yh[k]), a.d.mu_d[k]);
      if (clamp) sn = fminf(fmaxf(sn, a.d.s_lo[k]), a.d.s_hi[k]);
      a.state[(size_t)ep * od + k] = sn;
      a.obs[(size_t)ep * a.obs_ld + k] = sn;
      if constexpr (kRecord) {
        rc.c.observations[row * od + k] = sreg[q];
        rc.c.next_observations[row * od + k] = sn;
      }
    }
  }
  if constexpr (kRecord) {  // the clipped action taken: what the members read
    for (int c = j; c < ad; c += kRowThreads) rc.c.actions[row * ad + c] = l.xin[r * kS + od + c];
  }
  if (j == 0) {
    float rew = fmaf(a.d.sd_r[0], drawn(od, yh[od]), a.d.mu_r[0]);
    if (a.d.reward_penalty != 0.f) rew -= a.d.reward_penalty * u;
    float cost = yh[od + 1] > 0.5f ? 1.f : 0.f;
    bool halt = false;
    int t_halt = 0;
    if constexpr (kPess) {  // the pessimistic cost, and "unknown" as an absorbing state with a fixed reward and cost
      const float c = yh[od + 1];
      cost = (ps.cost_penalty != 0.f ? fmaf(ps.cost_penalty, u, c) : c) > 0.5f ? 1.f : 0.f;
      halt = u > ps.halt_threshold;  // (strict: +inf never halts, and neither does a NaN u)
      if (halt) {
        rew = ps.halt_reward;
        cost = ps.halt_cost;
        t_halt = (int)a.acc[(size_t)ep * 4 + 2];  // the episode's own step, before the tick
      }
    }
    const bool last = osrl_rollout::tick(a.acc + (size_t)ep * 4, rew, cost, a.d.cost_scale, a.d.episode_len,
                                         a.step_out ? a.step_out + (size_t)ep * 2 : nullptr);
    if constexpr (kPess) {
      if (halt) {  // the done latch: finished for every later launch, by live_step's rule
        a.acc[(size_t)ep * 4 + 3] = 1.f;
        if (ps.halt_step) ps.halt_step[ep] = t_halt;
      }
    }
    float* un = a.unc + (size_t)ep * 2;
    un[0] = fmaxf(un[0], u);
    un[1] += u;
    if constexpr (kRecord) {
      if (rc.row_unc) rc.row_unc[row] = u;
      osrl_rollout::record(rc.c, row, ep, rew, cost, a.d.cost_scale, last);
      if constexpr (kPess) {
        if (halt) {  // a terminal row, also at the episode's last step
          rc.c.terminals[row] = 1.f;
          rc.c.timeouts[row] = 0.f;
        }
      }
    }
  }
}

// One descriptor for the eight kernels: what a flag does not use stays zero and is never read.
struct SplitArgs {
  RecArgs r;          // r.s: the step; r.c and r.row_unc: kRecord
  GaussArgs g;        // kGauss
  PessArgs p;         // kPess
  float* member_out;  // [tiles][M][16][W]: the members' output tiles of this launch
  unsigned* arrive;   // [tiles]: the members signed in; zero between launches
  int32_t W, pad_;    // OSRL_MODEL_ENV_SPLIT_ROW(state_dim, kGauss)
};

// how the descriptor is reached: the kernarg segment, or device memory through the constant address space (argmem.h)
struct ByValue {
  typedef const SplitArgs& Split;
  typedef const StepArgs& Step;
  typedef const RecArgs& Rec;
  typedef const GaussArgs& Gauss;
  typedef const PessArgs& Pess;
};
struct ByPointer {
  typedef const OSRL_CAS SplitArgs& Split;
  typedef const OSRL_CAS StepArgs& Step;
  typedef const OSRL_CAS RecArgs& Rec;
  typedef const OSRL_CAS GaussArgs& Gauss;
  typedef const OSRL_CAS PessArgs& Pess;
};

template <bool kRecord, bool kGauss, bool kPess, class Ref>
__device__ __forceinline__ void menv_split_body(typename Ref::Split a, Lds& l, LdsGauss* lg) {
  __shared__ int s_last;
  typename Ref::Step s = a.r.s;
  const int tid = threadIdx.x;
  const int od = s.d.state_dim, M = s.d.n_models, no = od + 2, W = a.W;
  const int tile = blockIdx.x, m = blockIdx.y;  // (uniform)
  const int r = tid / kRowThreads, j = tid % kRowThreads;
  stage_rows<kRecord, kGauss, typename Ref::Step, typename Ref::Rec>(s, a.r, l, lg);
  float sreg[kKeep];
  stage_inputs<kRecord, typename Ref::Step, typename Ref::Rec>(s, a.r, l, sreg);
  // ---- member m alone
  {
    const float* x = l.xin;
    int cur = 0;
    const int nl = s.d.net[m].n_layers;
    for (int ly = 0; ly < nl; ++ly) {
      mfma_layer(s.d.net[m].Wf[ly], s.d.net[m].b[ly], s.d.net[m].dims[ly], s.d.net[m].dims[ly + 1], s.d.net[m].acts[ly], x,
                 l.buf[cur]);
      x = l.buf[cur];
      cur ^= 1;
    }
    float* mo = a.member_out + ((size_t)tile * M + m) * (size_t)(kTile * W);
    for (int i = tid; i < kTile * no; i += kThreads) {
      const int rr = i / no, c = i - rr * no;
      coh_put(mo + rr * W + c, x[rr * kS + c]);
    }
    if constexpr (kGauss) {  // sigma^2 of columns j, j + 32, .. < od + 1 of this thread's row, and the row's rms
      // (model_env.hip's listing squares and adds in two roundings -- its add sits behind a branch of its own; here the
      // two meet in one block and would be fused into one)
#pragma clang fp contract(off)
      float p = 0.f;
      for (int k = j; k <= od; k += kRowThreads) {
        const float sg = expf(0.5f * bounded_logvar(x[r * kS + no + k], a.g.lo, a.g.hi));
        const float v2 = sg * sg;
        if (k < od) p += v2;
        coh_put(mo + r * W + no + k, v2);
      }
#pragma unroll
      for (int o = kRowThreads / 2; o >= 1; o >>= 1) p += __shfl_xor(p, o);
      if (j == 0) coh_put(mo + r * W + no + od + 1, sqrtf(p / (float)od));
    }
  }
  // ---- sign in once every wave's stores are acknowledged; all but the last of the tile's M workgroups leave
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) s_last = arrive_last_acked(a.arrive + tile, M);  // (every wave waited above; the last one re-arms)
  __syncthreads();
  if (!s_last) return;
  // ---- the members, in order, from their tiles (the loop is unrolled: yk is indexed by constants and stays in registers)
  float yk[OSRL_MAX_NETS][kKeep];
  float amax = 0.f;
#pragma unroll
  for (int mm = 0; mm < OSRL_MAX_NETS; ++mm) {
#pragma unroll
    for (int q = 0; q < kKeep; ++q) yk[mm][q] = 0.f;
    if (mm < M) {  // (uniform)
      const float* t = a.member_out + ((size_t)tile * M + mm) * (size_t)(kTile * W);
#pragma unroll
      for (int q = 0; q < kKeep; ++q) {
        const int k = j + kRowThreads * q;
        if (k < od) yk[mm][q] = coh_get(t + r * W + k);
      }
      if constexpr (kGauss) {  // (element (r, k) of the variance tile is this thread's own)
        const int js = l.jsel[r];
        for (int k = j; k <= od; k += kRowThreads) {
          const float v2 = coh_get(t + r * W + no + k);
          float* vp = lg->v + r * kYS + k;
          if (s.d.mode == OSRL_MODEL_ENV_MEAN)
            *vp = mm == 0 ? v2 : *vp + v2;
          else if (js == mm)
            *vp = v2;
        }
        amax = fmaxf(amax, coh_get(t + r * W + no + od + 1));
      }
      for (int i = tid; i < kTile * no; i += kThreads) {  // (element i is this thread's for every member)
        const int rr = i / no, c = i - rr * no;
        const float v = coh_get(t + rr * W + c);
        l.ysum[rr * kYS + c] = mm == 0 ? v : l.ysum[rr * kYS + c] + v;
        if (l.jsel[rr] == mm) l.ysel[rr * kYS + c] = v;
      }
    }
  }
  step_epilogue<kRecord, kGauss, kPess, typename Ref::Step, typename Ref::Rec, typename Ref::Gauss, typename Ref::Pess>(
      s, a.r, l, a.g, lg, a.p, sreg, yk, amax);
}

template <bool kRecord, bool kGauss, bool kPess>
__global__ __launch_bounds__(kThreads) void menv_split_kernel(const SplitArgs a) {
  __shared__ Lds l;
  if constexpr (kGauss) {
    __shared__ LdsGauss lg;
    menv_split_body<kRecord, kGauss, kPess, ByValue>(a, l, &lg);
  } else {
    menv_split_body<kRecord, kGauss, kPess, ByValue>(a, l, nullptr);
  }
}
// the same kernels with their descriptor in device memory (argmem.h)
template <bool kRecord, bool kGauss, bool kPess>
__global__ __launch_bounds__(kThreads) void menv_split_kernel_p(const void* p) {
  __shared__ Lds l;
  if constexpr (kGauss) {
    __shared__ LdsGauss lg;
    menv_split_body<kRecord, kGauss, kPess, ByPointer>(*(const OSRL_CAS SplitArgs*)p, l, &lg);
  } else {
    menv_split_body<kRecord, kGauss, kPess, ByPointer>(*(const OSRL_CAS SplitArgs*)p, l, nullptr);
  }
}

template <bool kRecord, bool kGauss, bool kPess>
int launch_split(const SplitArgs& a, hipStream_t stream) {
  const unsigned tiles = ((unsigned)a.r.s.episodes + kTile - 1) / kTile;
  return osrl_argmem::launch(menv_split_kernel<kRecord, kGauss, kPess>, menv_split_kernel_p<kRecord, kGauss, kPess>,
                             dim3(tiles, (unsigned)a.r.s.d.n_models), dim3(kThreads), 0, stream, a);
}

}  // namespace

// osrl_model_env_step's arguments and refusals (model_env_args.h holds the checks of both), plus member_out and arrive
extern "C" int osrl_model_env_step_split(const osrl_model_env_t* env, const osrl_model_env_gauss_t* gauss,
                                         const osrl_model_env_pess_t* pess, const osrl_collect_t* rec, float* row_unc,
                                         const float* act, float* state, float* obs, int32_t obs_ld, float* acc,
                                         float* unc, float* step_out, int32_t episodes, float* member_out,
                                         int32_t* arrive, void* stream) {
  if ((env != nullptr) == (gauss != nullptr) || !member_out || !arrive) return -1;
  const osrl_model_env_t* d = gauss ? &gauss->env : env;
  if (rec && (!osrl_rollout::valid_collect(rec) || d->episode_len < 1)) return -1;
  SplitArgs a;
  memset(&a, 0, sizeof a);
  if (!fill_step(a.r.s, d, act, state, obs, obs_ld, acc, unc, rec ? nullptr : step_out, episodes, gauss != nullptr))
    return -1;
  if (gauss && !fill_gauss(a.g, gauss)) return -1;
  if (pess && !fill_pess(a.p, pess)) return -1;
  if (rec) {
    a.r.c = *rec;
    a.r.row_unc = row_unc;
  }
  a.member_out = member_out;
  a.arrive = reinterpret_cast<unsigned*>(arrive);
  a.W = OSRL_MODEL_ENV_SPLIT_ROW(d->state_dim, gauss != nullptr);
  const hipStream_t st = (hipStream_t)stream;
  switch ((rec ? 4 : 0) | (gauss ? 2 : 0) | (pess ? 1 : 0)) {
    case 0: return launch_split<false, false, false>(a, st);
    case 1: return launch_split<false, false, true>(a, st);
    case 2: return launch_split<false, true, false>(a, st);
    case 3: return launch_split<false, true, true>(a, st);
    case 4: return launch_split<true, false, false>(a, st);
    case 5: return launch_split<true, false, true>(a, st);
    case 6: return launch_split<true, true, false>(a, st);
    default: return launch_split<true, true, true>(a, st);
  }
}
