// model_env.hip -- the learned-dynamics vector environment for gfx950 (MI355X): an ensemble of MLPs fitted on logged
// transitions (algorithms/dynamics.py), stepped with osrl_env_step's interface (include/osrl_amd.h osrl_model_env_t).
//
// ONE launch per environment step for all E episodes; one workgroup (512 threads, 8 waves) per 16-episode tile runs the
// whole ensemble with its activations in LDS:
//   * the layers are act_vec.hip's: v_mfma_f32_16x16x4_f32 over the packed forward weights PF[k/4][n][k%4] and the canonical
//     biases of the flat group -- what the fused Adam step keeps current, so the environment follows training in place; a
//     layer's 16-column output tiles are dealt to the 8 waves, two per wave and pass, and a wave walks ALL of K for its
//     tiles (no split-K, no arithmetic across rows): an episode's trajectory is the same bits whatever E is, whichever
//     tile row it sits in and whatever its neighbours do;
//   * the members run one after the other on the same staged input tile; thread (row = tid / 32, j = tid % 32) keeps the
//     state columns j, j + 32, .. of every member's output in registers until the mean exists (the disagreement needs
//     both), the running sum and the chosen member's output live in LDS;
//   * the member a RANDOM-mode episode follows is a Philox word keyed by (seed, episode id, the episode's own step): a
//     function of nothing else.
//
// The same body records (model_rec_kernel, osrl_model_env_collect): the compile-time flag kRecord adds csrc/rollout_step.h's
// per-episode exploration noise on the action while it is staged, one row of a DSRL-layout dataset per episode and step,
// and the discounted sums; with sigma == 0 the step is model_env_kernel's bit for bit.  A row of the tile stores only
// while it is live, and with kRecord live means e < episodes AND rollout_step.h's live_step: its rule keeps every write
// inside the tables.
//
// A second compile-time flag, kGauss (osrl_model_env_step_gauss / osrl_model_env_collect_gauss: model_env_gauss_kernel,
// model_rec_gauss_kernel and their twins), reads members that are diagonal Gaussians -- (od + 1 means | cost | od + 1 raw
// log-variances), the first od + 2 columns exactly as before.  Right after a member's last layer the row's 32 threads turn
// its raw log-variances into sigma^2 (PETS' soft clamp), add them into or copy them to ONE extra LDS tile (the mean
// variance or the followed member's) and reduce sum_{k < od} sigma^2 into a running maximum: no per-member variance is
// kept in registers.  The epilogue draws yh[k] += sqrt(v[k]) eps[k] (Philox stream 16, keyed by seed, episode id, the
// episode's own step and the column, or injected) and uses max_m rms(sigma_m) in the disagreement's place when asked to.
// With the flag off nothing of this exists: the four kernels above keep their listing.
//
// A third compile-time flag, kPess (osrl_model_env_step_halt / _collect_halt / _step_gauss_halt / _collect_gauss_halt:
// halt_env_kernel, halt_rec_kernel, halt_env_gauss_kernel, halt_rec_gauss_kernel and their twins), makes the step
// pessimistic where lane j == 0 of a row forms reward and cost: the cost threshold is applied to c + cost_penalty u
// (CAP's inflation), and u > halt_threshold ends the episode with a fixed reward and cost (MOReL's absorbing "unknown"):
// the done latch is set, halt_step[e] takes the step, a recorded row is terminal.  Nothing else moves; with the threshold
// at +inf and the penalty 0 the eight kernels give the other eight's bits.  With the flag off nothing of this exists.
//
// model_branch_kernel (osrl_model_env_branch) starts every episode at a row drawn uniformly from a store's observations.
#include "argmem.h"
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
constexpr uint32_t kBranchStream = 15;                      // Philox stream of the branch starts (13: the exploration noise)

struct StepArgs {
  osrl_model_env_t d;
  const float* act;
  float* state;
  float* obs;
  float* acc;
  float* unc;
  float* step_out;
  int32_t obs_ld, episodes;
};

struct RecArgs {
  StepArgs s;  // (step_out is unused: the tables carry the step's reward and cost)
  osrl_collect_t c;
  float* row_unc;
};
struct NoRec {};

// what the Gaussian step adds to either descriptor (osrl_model_env_gauss_t beyond its osrl_model_env_t)
struct GaussArgs {
  const float* noise_in;
  float lo, hi;
  int32_t sample, unc;
};
struct GStepArgs {
  StepArgs s;
  GaussArgs g;
};
struct GRecArgs {
  RecArgs r;
  GaussArgs g;
};
struct NoGauss {};
// what the pessimistic step adds to any of the four descriptors (osrl_model_env_pess_t, by value)
struct PessArgs {
  float halt_threshold, halt_reward, halt_cost, cost_penalty;
  int32_t* halt_step;
};
struct HStepArgs {
  StepArgs s;
  PessArgs p;
};
struct HRecArgs {
  RecArgs r;
  PessArgs p;
};
struct HGStepArgs {
  GStepArgs s;
  PessArgs p;
};
struct HGRecArgs {
  GRecArgs r;
  PessArgs p;
};
struct NoPess {};
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
static_assert(sizeof(Lds) <= 160 * 1024, "model_env_kernel: LDS per workgroup");

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

// AR = how the descriptor is reached: `const StepArgs&` (the kernarg segment) or `const OSRL_CAS StepArgs&` (argmem.h).
// kRecord: the step is recorded; RR reaches the RecArgs the same way (NoRec otherwise).
// kGauss: the members are diagonal Gaussians (osrl_model_env_gauss_t); GR reaches the GaussArgs, lg is the extra LDS.
// kPess: the step halts where u > halt_threshold and inflates the cost by cost_penalty * u (osrl_model_env_pess_t); PR
// reaches the PessArgs.  Only the row's lane j == 0 reads them.
template <bool kRecord, class AR, class RR, bool kGauss = false, class GR = NoGauss, bool kPess = false, class PR = NoPess>
__device__ __forceinline__ void model_env_body(AR a, RR rc, Lds& l, GR g = GR{}, LdsGauss* lg = nullptr, PR ps = PR{}) {
  const int tid = threadIdx.x;
  const int od = a.d.state_dim, ad = a.d.action_dim, M = a.d.n_models, no = od + 2;
  const int e0 = blockIdx.x * kTile;  // the tile's first episode
  const int r = tid / kRowThreads, j = tid % kRowThreads;
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
  const bool alive = l.live[r] != 0;
  const int ep = e0 + r;
  // ---- the state columns this thread advances at the end, and the staged input rows; idle rows are zero
  float sreg[kKeep];
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
  // ---- the members, in order (the loop is unrolled: yk is indexed by constants and stays in registers)
  float yk[OSRL_MAX_NETS][kKeep];
  float amax = 0.f;  // (Gaussian) max over the members so far of sqrt(mean_{k < od} sigma^2): no per-member variance is kept
#pragma unroll
  for (int m = 0; m < OSRL_MAX_NETS; ++m) {
#pragma unroll
    for (int q = 0; q < kKeep; ++q) yk[m][q] = 0.f;
    if (m < M) {  // (uniform)
      const float* x = l.xin;
      int cur = 0;
      const int nl = a.d.net[m].n_layers;
      for (int ly = 0; ly < nl; ++ly) {
        mfma_layer(a.d.net[m].Wf[ly], a.d.net[m].b[ly], a.d.net[m].dims[ly], a.d.net[m].dims[ly + 1],
                   a.d.net[m].acts[ly], x, l.buf[cur]);
        x = l.buf[cur];
        cur ^= 1;
      }
#pragma unroll
      for (int q = 0; q < kKeep; ++q) {
        const int k = j + kRowThreads * q;
        if (k < od) yk[m][q] = x[r * kS + k];
      }
      if constexpr (kGauss) {  // sigma^2 of columns j, j + 32, .. < od + 1 of this thread's row (element (r, k) is its own)
        const int js = l.jsel[r];
        float p = 0.f;
        for (int k = j; k <= od; k += kRowThreads) {
          const float sg = expf(0.5f * bounded_logvar(x[r * kS + no + k], g.lo, g.hi));
          const float v2 = sg * sg;
          if (k < od) p += v2;
          float* vp = lg->v + r * kYS + k;
          if (a.d.mode == OSRL_MODEL_ENV_MEAN)
            *vp = m == 0 ? v2 : *vp + v2;
          else if (js == m)
            *vp = v2;
        }
#pragma unroll
        for (int o = kRowThreads / 2; o >= 1; o >>= 1) p += __shfl_xor(p, o);
        amax = fmaxf(amax, sqrtf(p / (float)od));
      }
      for (int i = tid; i < kTile * no; i += kThreads) {  // (element i is this thread's for every member)
        const int rr = i / no, c = i - rr * no;
        const float v = x[rr * kS + c];
        l.ysum[rr * kYS + c] = m == 0 ? v : l.ysum[rr * kYS + c] + v;
        if (l.jsel[rr] == m) l.ysel[rr * kYS + c] = v;
      }
      __syncthreads();  // the next member's first layers write the tile this one's output sits in
    }
  }
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

__global__ __launch_bounds__(kThreads) void model_env_kernel(const StepArgs a) {
  __shared__ Lds l;
  model_env_body<false, const StepArgs&, NoRec>(a, NoRec{}, l);
}
// the same kernel with its descriptor in device memory (argmem.h)
__global__ __launch_bounds__(kThreads) void model_env_kernel_p(const void* p) {
  __shared__ Lds l;
  model_env_body<false, const OSRL_CAS StepArgs&, NoRec>(*(const OSRL_CAS StepArgs*)p, NoRec{}, l);
}

// the recording step (osrl_model_env_collect) and its descriptor-pointer twin
__global__ __launch_bounds__(kThreads) void model_rec_kernel(const RecArgs a) {
  __shared__ Lds l;
  model_env_body<true, const StepArgs&, const RecArgs&>(a.s, a, l);
}
__global__ __launch_bounds__(kThreads) void model_rec_kernel_p(const void* p) {
  __shared__ Lds l;
  const OSRL_CAS RecArgs& a = *(const OSRL_CAS RecArgs*)p;
  model_env_body<true, const OSRL_CAS StepArgs&, const OSRL_CAS RecArgs&>(a.s, a, l);
}

// the Gaussian step and recording step (osrl_model_env_step_gauss / _collect_gauss), each with its descriptor-pointer twin
__global__ __launch_bounds__(kThreads) void model_env_gauss_kernel(const GStepArgs a) {
  __shared__ Lds l;
  __shared__ LdsGauss lg;
  model_env_body<false, const StepArgs&, NoRec, true, const GaussArgs&>(a.s, NoRec{}, l, a.g, &lg);
}
__global__ __launch_bounds__(kThreads) void model_env_gauss_kernel_p(const void* p) {
  __shared__ Lds l;
  __shared__ LdsGauss lg;
  const OSRL_CAS GStepArgs& a = *(const OSRL_CAS GStepArgs*)p;
  model_env_body<false, const OSRL_CAS StepArgs&, NoRec, true, const OSRL_CAS GaussArgs&>(a.s, NoRec{}, l, a.g, &lg);
}
__global__ __launch_bounds__(kThreads) void model_rec_gauss_kernel(const GRecArgs a) {
  __shared__ Lds l;
  __shared__ LdsGauss lg;
  model_env_body<true, const StepArgs&, const RecArgs&, true, const GaussArgs&>(a.r.s, a.r, l, a.g, &lg);
}
__global__ __launch_bounds__(kThreads) void model_rec_gauss_kernel_p(const void* p) {
  __shared__ Lds l;
  __shared__ LdsGauss lg;
  const OSRL_CAS GRecArgs& a = *(const OSRL_CAS GRecArgs*)p;
  model_env_body<true, const OSRL_CAS StepArgs&, const OSRL_CAS RecArgs&, true, const OSRL_CAS GaussArgs&>(a.r.s, a.r, l,
                                                                                                         a.g, &lg);
}
static_assert(sizeof(Lds) + sizeof(LdsGauss) <= 160 * 1024, "model_env_gauss_kernel: LDS per workgroup");

// the pessimistic step (osrl_model_env_step_halt / _collect_halt / _step_gauss_halt / _collect_gauss_halt): the four
// kernels above with kPess on, each with its descriptor-pointer twin.  No LDS beside theirs.
__global__ __launch_bounds__(kThreads) void halt_env_kernel(const HStepArgs a) {
  __shared__ Lds l;
  model_env_body<false, const StepArgs&, NoRec, false, NoGauss, true, const PessArgs&>(a.s, NoRec{}, l, NoGauss{}, nullptr,
                                                                                     a.p);
}
__global__ __launch_bounds__(kThreads) void halt_env_kernel_p(const void* p) {
  __shared__ Lds l;
  const OSRL_CAS HStepArgs& a = *(const OSRL_CAS HStepArgs*)p;
  model_env_body<false, const OSRL_CAS StepArgs&, NoRec, false, NoGauss, true, const OSRL_CAS PessArgs&>(
      a.s, NoRec{}, l, NoGauss{}, nullptr, a.p);
}
__global__ __launch_bounds__(kThreads) void halt_rec_kernel(const HRecArgs a) {
  __shared__ Lds l;
  model_env_body<true, const StepArgs&, const RecArgs&, false, NoGauss, true, const PessArgs&>(a.r.s, a.r, l, NoGauss{},
                                                                                             nullptr, a.p);
}
__global__ __launch_bounds__(kThreads) void halt_rec_kernel_p(const void* p) {
  __shared__ Lds l;
  const OSRL_CAS HRecArgs& a = *(const OSRL_CAS HRecArgs*)p;
  model_env_body<true, const OSRL_CAS StepArgs&, const OSRL_CAS RecArgs&, false, NoGauss, true, const OSRL_CAS PessArgs&>(
      a.r.s, a.r, l, NoGauss{}, nullptr, a.p);
}
__global__ __launch_bounds__(kThreads) void halt_env_gauss_kernel(const HGStepArgs a) {
  __shared__ Lds l;
  __shared__ LdsGauss lg;
  model_env_body<false, const StepArgs&, NoRec, true, const GaussArgs&, true, const PessArgs&>(a.s.s, NoRec{}, l, a.s.g, &lg,
                                                                                             a.p);
}
__global__ __launch_bounds__(kThreads) void halt_env_gauss_kernel_p(const void* p) {
  __shared__ Lds l;
  __shared__ LdsGauss lg;
  const OSRL_CAS HGStepArgs& a = *(const OSRL_CAS HGStepArgs*)p;
  model_env_body<false, const OSRL_CAS StepArgs&, NoRec, true, const OSRL_CAS GaussArgs&, true, const OSRL_CAS PessArgs&>(
      a.s.s, NoRec{}, l, a.s.g, &lg, a.p);
}
__global__ __launch_bounds__(kThreads) void halt_rec_gauss_kernel(const HGRecArgs a) {
  __shared__ Lds l;
  __shared__ LdsGauss lg;
  model_env_body<true, const StepArgs&, const RecArgs&, true, const GaussArgs&, true, const PessArgs&>(a.r.r.s, a.r.r, l,
                                                                                                     a.r.g, &lg, a.p);
}
__global__ __launch_bounds__(kThreads) void halt_rec_gauss_kernel_p(const void* p) {
  __shared__ Lds l;
  __shared__ LdsGauss lg;
  const OSRL_CAS HGRecArgs& a = *(const OSRL_CAS HGRecArgs*)p;
  model_env_body<true, const OSRL_CAS StepArgs&, const OSRL_CAS RecArgs&, true, const OSRL_CAS GaussArgs&, true,
                 const OSRL_CAS PessArgs&>(a.r.r.s, a.r.r, l, a.r.g, &lg, a.p);
}

struct BranchArgs {
  const float* table;         // [n_rows, od]
  const int64_t* n_rows_dev;  // the store's live-count word, or nullptr
  const uint64_t* seed;
  float *state, *obs, *acc, *unc, *disc;
  int64_t* start_rows;
  int64_t n_rows, n_limit;
  int32_t od, obs_ld, episodes;
  uint32_t episode_base;
};

// one wave per episode; the index never leaves [0, n_rows): n is capped by the allocation and is at least 1
__global__ __launch_bounds__(256) void model_branch_kernel(const BranchArgs a) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= a.episodes) return;
  int64_t n = a.n_rows_dev ? *a.n_rows_dev : a.n_rows;
  if (n > a.n_rows) n = a.n_rows;
  if (a.n_limit > 0 && n > a.n_limit) n = a.n_limit;
  if (n < 1) n = 1;
  const uint64_t seed = *a.seed;
  const U4 w = philox4x32_10(U4{a.episode_base + (uint32_t)e, 0u, 0u, kBranchStream}, (uint32_t)seed,
                             (uint32_t)(seed >> 32));
  const int64_t idx = (int64_t)__umul64hi(((uint64_t)w.x << 32) | w.y, (uint64_t)n);  // (gather.h's uniform draw)
  for (int k = lane; k < a.od; k += 64) {
    const float v = a.table[(size_t)idx * a.od + k];
    a.state[(size_t)e * a.od + k] = v;
    a.obs[(size_t)e * a.obs_ld + k] = v;
  }
  if (lane < 4) {
    a.acc[(size_t)e * 4 + lane] = 0.f;
    a.disc[(size_t)e * 4 + lane] = lane == 2 ? 1.f : 0.f;
  }
  if (lane < 2) a.unc[(size_t)e * 2 + lane] = 0.f;
  if (lane == 0) a.start_rows[e] = idx;
}

struct PrepArgs {
  const float *obs, *nobs, *rew, *cost, *mu_s, *sd_s, *mu_d, *sd_d, *mu_r, *sd_r;
  float *xs, *target;
  int32_t rows, od;
};

__global__ __launch_bounds__(256) void dyn_prepare_kernel(const PrepArgs a) {
  const int no = a.od + 2;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)a.rows * no) return;
  const int b = (int)(i / no), c = (int)(i - (int64_t)b * no);
  float t;
  if (c < a.od) {
    const float o = a.obs[(size_t)b * a.od + c];
    a.xs[(size_t)b * a.od + c] = (o - a.mu_s[c]) / a.sd_s[c];
    t = (a.nobs[(size_t)b * a.od + c] - o - a.mu_d[c]) / a.sd_d[c];
  } else if (c == a.od) {
    t = (a.rew[b] - a.mu_r[0]) / a.sd_r[0];
  } else {
    t = a.cost[b];
  }
  a.target[i] = t;
}

bool valid_member(const osrl_gemv_net_t& n, int in, int out) {
  if (n.n_layers < 1 || n.n_layers > OSRL_MAX_LAYERS || n.out_scale != 1.0f) return false;
  for (int l = 0; l <= n.n_layers; ++l)
    if (n.dims[l] < 1 || n.dims[l] > OSRL_MODEL_ENV_MAX_WIDTH) return false;
  for (int l = 0; l < n.n_layers; ++l)
    if (!n.Wf[l] || !n.b[l]) return false;
  return n.dims[0] == in && n.dims[n.n_layers] == out;
}

// the step's descriptor, checked (false: a bad argument)
bool fill_step(StepArgs& a, const osrl_model_env_t* env, const float* act, float* state, float* obs, int32_t obs_ld,
               float* acc, float* unc, float* step_out, int32_t episodes, bool gauss = false) {
  if (!env || !act || !state || !obs || !acc || !unc || episodes < 1) return false;
  const osrl_model_env_t& d = *env;
  if (d.n_models < 1 || d.n_models > OSRL_MAX_NETS || d.state_dim < 1 || d.state_dim > OSRL_MODEL_ENV_MAX_STATE ||
      d.action_dim < 1 || obs_ld < d.state_dim || !d.mu_s || !d.sd_s || !d.mu_d || !d.sd_d || !d.mu_r || !d.sd_r ||
      (d.s_lo == nullptr) != (d.s_hi == nullptr))
    return false;
  if (d.mode < OSRL_MODEL_ENV_MEAN || d.mode > OSRL_MODEL_ENV_RANDOM) return false;
  if (d.mode == OSRL_MODEL_ENV_MEMBER && (d.member < 0 || d.member >= d.n_models)) return false;
  if (d.mode == OSRL_MODEL_ENV_RANDOM && !d.seed && !d.member_in) return false;
  for (int m = 0; m < d.n_models; ++m)
    if (!valid_member(d.net[m], d.state_dim + d.action_dim, gauss ? 2 * d.state_dim + 3 : d.state_dim + 2)) return false;
  memset(&a, 0, sizeof a);  // (the arena finds a block by its bytes: no stray padding)
  a.d = d;
  for (int m = d.n_models; m < OSRL_MAX_NETS; ++m) memset(&a.d.net[m], 0, sizeof a.d.net[m]);
  a.d.pad_ = 0;
  a.d.pad2_ = 0.f;
  a.act = act;
  a.state = state;
  a.obs = obs;
  a.acc = acc;
  a.unc = unc;
  a.step_out = step_out;
  a.obs_ld = obs_ld;
  a.episodes = episodes;
  return true;
}

}  // namespace

extern "C" int osrl_model_env_step(const osrl_model_env_t* env, const float* act, float* state, float* obs,
                                   int32_t obs_ld, float* acc, float* unc, float* step_out, int32_t episodes,
                                   void* stream) {
  StepArgs a;
  if (!fill_step(a, env, act, state, obs, obs_ld, acc, unc, step_out, episodes)) return -1;
  const int tiles = (episodes + kTile - 1) / kTile;
  return osrl_argmem::launch(model_env_kernel, model_env_kernel_p, dim3(tiles), dim3(kThreads), 0, (hipStream_t)stream,
                             a);
}

extern "C" int osrl_model_env_collect(const osrl_model_env_t* env, const osrl_collect_t* rec, const float* act,
                                      float* state, float* obs, int32_t obs_ld, float* acc, float* unc, float* row_unc,
                                      int32_t episodes, void* stream) {
  if (!osrl_rollout::valid_collect(rec) || !env || env->episode_len < 1) return -1;
  RecArgs a;
  memset(&a, 0, sizeof a);
  if (!fill_step(a.s, env, act, state, obs, obs_ld, acc, unc, nullptr, episodes)) return -1;
  a.c = *rec;
  a.row_unc = row_unc;
  const int tiles = (episodes + kTile - 1) / kTile;
  return osrl_argmem::launch(model_rec_kernel, model_rec_kernel_p, dim3(tiles), dim3(kThreads), 0, (hipStream_t)stream,
                             a);
}

namespace {
// the Gaussian additions, checked (false: a bad argument)
bool fill_gauss(GaussArgs& g, const osrl_model_env_gauss_t* env) {
  if (!env || !(env->logvar_min < env->logvar_max)) return false;
  if (env->uncertainty != OSRL_MODEL_ENV_UNC_DISAGREEMENT && env->uncertainty != OSRL_MODEL_ENV_UNC_MAX_STD) return false;
  if (env->sample && !env->noise_in && !env->env.seed) return false;
  g.noise_in = env->sample ? env->noise_in : nullptr;
  g.lo = env->logvar_min;
  g.hi = env->logvar_max;
  g.sample = env->sample ? 1 : 0;
  g.unc = env->uncertainty;
  return true;
}
}  // namespace

extern "C" int osrl_model_env_step_gauss(const osrl_model_env_gauss_t* env, const float* act, float* state, float* obs,
                                         int32_t obs_ld, float* acc, float* unc, float* step_out, int32_t episodes,
                                         void* stream) {
  GStepArgs a;
  memset(&a, 0, sizeof a);
  if (!env || !fill_step(a.s, &env->env, act, state, obs, obs_ld, acc, unc, step_out, episodes, true)) return -1;
  if (!fill_gauss(a.g, env)) return -1;
  const int tiles = (episodes + kTile - 1) / kTile;
  return osrl_argmem::launch(model_env_gauss_kernel, model_env_gauss_kernel_p, dim3(tiles), dim3(kThreads), 0,
                             (hipStream_t)stream, a);
}

extern "C" int osrl_model_env_collect_gauss(const osrl_model_env_gauss_t* env, const osrl_collect_t* rec,
                                            const float* act, float* state, float* obs, int32_t obs_ld, float* acc,
                                            float* unc, float* row_unc, int32_t episodes, void* stream) {
  if (!osrl_rollout::valid_collect(rec) || !env || env->env.episode_len < 1) return -1;
  GRecArgs a;
  memset(&a, 0, sizeof a);
  if (!fill_step(a.r.s, &env->env, act, state, obs, obs_ld, acc, unc, nullptr, episodes, true)) return -1;
  if (!fill_gauss(a.g, env)) return -1;
  a.r.c = *rec;
  a.r.row_unc = row_unc;
  const int tiles = (episodes + kTile - 1) / kTile;
  return osrl_argmem::launch(model_rec_gauss_kernel, model_rec_gauss_kernel_p, dim3(tiles), dim3(kThreads), 0,
                             (hipStream_t)stream, a);
}

namespace {
// the pessimistic additions, checked (false: a bad argument; +-inf thresholds are values like any other)
bool fill_pess(PessArgs& p, const osrl_model_env_pess_t* ps) {
  if (!ps || ps->halt_threshold != ps->halt_threshold || !(ps->halt_reward == ps->halt_reward)) return false;
  if (ps->halt_cost != 0.f && ps->halt_cost != 1.f) return false;
  if (!(ps->cost_penalty >= 0.f) || ps->cost_penalty > 3.0e38f) return false;
  p.halt_threshold = ps->halt_threshold;
  p.halt_reward = ps->halt_reward;
  p.halt_cost = ps->halt_cost;
  p.cost_penalty = ps->cost_penalty;
  p.halt_step = ps->halt_step;
  return true;
}
}  // namespace

extern "C" int osrl_model_env_step_halt(const osrl_model_env_t* env, const osrl_model_env_pess_t* pess, const float* act,
                                        float* state, float* obs, int32_t obs_ld, float* acc, float* unc,
                                        float* step_out, int32_t episodes, void* stream) {
  HStepArgs a;
  memset(&a, 0, sizeof a);
  if (!fill_step(a.s, env, act, state, obs, obs_ld, acc, unc, step_out, episodes) || !fill_pess(a.p, pess)) return -1;
  const int tiles = (episodes + kTile - 1) / kTile;
  return osrl_argmem::launch(halt_env_kernel, halt_env_kernel_p, dim3(tiles), dim3(kThreads), 0, (hipStream_t)stream, a);
}

extern "C" int osrl_model_env_collect_halt(const osrl_model_env_t* env, const osrl_model_env_pess_t* pess,
                                           const osrl_collect_t* rec, const float* act, float* state, float* obs,
                                           int32_t obs_ld, float* acc, float* unc, float* row_unc, int32_t episodes,
                                           void* stream) {
  if (!osrl_rollout::valid_collect(rec) || !env || env->episode_len < 1) return -1;
  HRecArgs a;
  memset(&a, 0, sizeof a);
  if (!fill_step(a.r.s, env, act, state, obs, obs_ld, acc, unc, nullptr, episodes) || !fill_pess(a.p, pess)) return -1;
  a.r.c = *rec;
  a.r.row_unc = row_unc;
  const int tiles = (episodes + kTile - 1) / kTile;
  return osrl_argmem::launch(halt_rec_kernel, halt_rec_kernel_p, dim3(tiles), dim3(kThreads), 0, (hipStream_t)stream, a);
}

extern "C" int osrl_model_env_step_gauss_halt(const osrl_model_env_gauss_t* env, const osrl_model_env_pess_t* pess,
                                              const float* act, float* state, float* obs, int32_t obs_ld, float* acc,
                                              float* unc, float* step_out, int32_t episodes, void* stream) {
  HGStepArgs a;
  memset(&a, 0, sizeof a);
  if (!env || !fill_step(a.s.s, &env->env, act, state, obs, obs_ld, acc, unc, step_out, episodes, true)) return -1;
  if (!fill_gauss(a.s.g, env) || !fill_pess(a.p, pess)) return -1;
  const int tiles = (episodes + kTile - 1) / kTile;
  return osrl_argmem::launch(halt_env_gauss_kernel, halt_env_gauss_kernel_p, dim3(tiles), dim3(kThreads), 0,
                             (hipStream_t)stream, a);
}

extern "C" int osrl_model_env_collect_gauss_halt(const osrl_model_env_gauss_t* env, const osrl_model_env_pess_t* pess,
                                                 const osrl_collect_t* rec, const float* act, float* state, float* obs,
                                                 int32_t obs_ld, float* acc, float* unc, float* row_unc,
                                                 int32_t episodes, void* stream) {
  if (!osrl_rollout::valid_collect(rec) || !env || env->env.episode_len < 1) return -1;
  HGRecArgs a;
  memset(&a, 0, sizeof a);
  if (!fill_step(a.r.r.s, &env->env, act, state, obs, obs_ld, acc, unc, nullptr, episodes, true)) return -1;
  if (!fill_gauss(a.r.g, env) || !fill_pess(a.p, pess)) return -1;
  a.r.r.c = *rec;
  a.r.r.row_unc = row_unc;
  const int tiles = (episodes + kTile - 1) / kTile;
  return osrl_argmem::launch(halt_rec_gauss_kernel, halt_rec_gauss_kernel_p, dim3(tiles), dim3(kThreads), 0,
                             (hipStream_t)stream, a);
}

extern "C" int osrl_model_env_branch(const float* table, int64_t n_rows, const int64_t* n_rows_dev, int64_t n_limit,
                                     int32_t state_dim, const uint64_t* seed, uint32_t episode_base, float* state,
                                     float* obs, int32_t obs_ld, float* acc, float* unc, float* disc,
                                     int64_t* start_rows, int32_t episodes, void* stream) {
  if (!table || !seed || !state || !obs || !acc || !unc || !disc || !start_rows || n_rows < 1 || n_limit < 0 ||
      state_dim < 1 || obs_ld < state_dim || episodes < 1)
    return -1;
  const BranchArgs a{table, n_rows_dev, seed,    state,     obs,    acc,      unc,         disc,
                     start_rows, n_rows, n_limit, state_dim, obs_ld, episodes, episode_base};
  return osrl_argmem::launch(model_branch_kernel, nullptr, dim3((unsigned)((episodes + 3) / 4)), dim3(256), 0,
                             (hipStream_t)stream, a);
}

extern "C" int osrl_dyn_prepare(const float* obs, const float* nobs, const float* rew, const float* cost,
                                const float* mu_s, const float* sd_s, const float* mu_d, const float* sd_d,
                                const float* mu_r, const float* sd_r, int32_t rows, int32_t state_dim, float* xs,
                                float* target, void* stream) {
  if (!obs || !nobs || !rew || !cost || !mu_s || !sd_s || !mu_d || !sd_d || !mu_r || !sd_r || !xs || !target ||
      rows < 1 || state_dim < 1)
    return -1;
  const PrepArgs a{obs, nobs, rew, cost, mu_s, sd_s, mu_d, sd_d, mu_r, sd_r, xs, target, rows, state_dim};
  const int64_t n = (int64_t)rows * (state_dim + 2);
  return osrl_argmem::launch(dyn_prepare_kernel, nullptr, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                             (hipStream_t)stream, a);
}
