// plan.hip -- policy-guided shooting on the learned model (engine/mpc.py ModelPlanner): the two launches around the
// recorded model steps of a planning call.  N real states ("slots") fan out into N K imagined episodes, episode
// e = n K + k being candidate k of slot n; after H recorded steps (csrc/model_env.hip, untouched) one candidate per slot is
// chosen from the discounted sums the recording step keeps.
//
//   plan_fanout_kernel (osrl_plan_fanout)  one wave per episode, four per workgroup -- model_branch_kernel's shape and its
//       stores, the row coming from states[e / K] instead of a store draw, plus halt_step[e] = -1 where the environment
//       can halt.  Nothing but plain vector stores; every index is below N K rows of its table.
//   plan_select_kernel (osrl_plan_select)  one workgroup of 256 threads per slot; a thread looks at candidates tid,
//       tid + 256, .. (K <= 1024: at most four).  The choice is a reduction under a total order, so it is the same
//       whatever tree reduces it: within a wave by shuffles, across the four waves through LDS.  The softmax weights of
//       the MPPI rule are staged in LDS (4 KB) and summed by ONE thread per action column, in fp64, in ascending k: no
//       float atomics, the same bits on every launch.  The copied row moves as 32-bit words.
// Neither kernel reads blockDim / gridDim (the launch shapes are the constants below).  DESIGN.md "Planning at act time"
// restates the rule and keeps the registers / LDS of both.
#include "argmem.h"
#include "rollout_step.h"

namespace {

constexpr int kFanThreads = 256, kFanWaves = 4;
constexpr int kSelThreads = 256, kSelWaves = 4;

struct FanoutArgs {
  const float* states;  // [slots, od]
  float *state, *obs, *acc, *unc, *disc;
  int32_t* halt_step;   // [slots * candidates] or nullptr
  int32_t od, obs_ld, candidates, episodes;
};

__global__ __launch_bounds__(kFanThreads) void plan_fanout_kernel(const FanoutArgs a) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * kFanWaves + (threadIdx.x >> 6);
  if (e >= a.episodes) return;
  const int n = e / a.candidates;
  for (int k = lane; k < a.od; k += 64) {
    const float v = a.states[(size_t)n * a.od + k];
    a.state[(size_t)e * a.od + k] = v;
    a.obs[(size_t)e * a.obs_ld + k] = v;
  }
  if (lane < 4) {
    a.acc[(size_t)e * 4 + lane] = 0.f;
    a.disc[(size_t)e * 4 + lane] = lane == 2 ? 1.f : 0.f;
  }
  if (lane < 2) a.unc[(size_t)e * 2 + lane] = 0.f;
  if (lane == 0 && a.halt_step) a.halt_step[e] = -1;
}

struct SelectArgs {
  const uint32_t* actions;   // [slots * candidates * horizon, ad] as words: row e * horizon is candidate e's first action
  const float* disc;         // [slots * candidates, 4]: (J, C, gamma^t, -)
  const float* budget;       // [slots]
  const float* temperature;  // [1]
  uint32_t* action;          // [slots, ad] as words
  int32_t *chosen, *n_feasible;
  int32_t candidates, horizon, ad;
};

// a candidate as the two orders see it; k < 0: none
struct Best {
  float j, c;
  int k;
};

// the feasible order: larger J, then lower k
__device__ __forceinline__ bool better_j(const Best& a, const Best& b) {
  return a.k >= 0 && (b.k < 0 || a.j > b.j || (a.j == b.j && a.k < b.k));
}
// the order of an empty feasible set: smaller C, then larger J, then lower k
__device__ __forceinline__ bool better_c(const Best& a, const Best& b) {
  return a.k >= 0 && (b.k < 0 || a.c < b.c || (a.c == b.c && (a.j > b.j || (a.j == b.j && a.k < b.k))));
}

__device__ __forceinline__ Best shfl_xor(const Best& b, int m) {
  return Best{__shfl_xor(b.j, m), __shfl_xor(b.c, m), __shfl_xor(b.k, m)};
}

__global__ __launch_bounds__(kSelThreads) void plan_select_kernel(const SelectArgs a) {
  __shared__ float w[1024];  // OSRL_PLAN_MAX_CANDIDATES softmax weights (0 outside the feasible set)
  __shared__ Best red_f[kSelWaves], red_c[kSelWaves];
  __shared__ int red_n[kSelWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x, K = a.candidates;
  const size_t e0 = (size_t)n * K;
  const float budget = a.budget[n], temp = *a.temperature;

  Best bf{0.f, 0.f, -1}, bc{0.f, 0.f, -1};
  int cnt = 0;
  for (int k = tid; k < K; k += kSelThreads) {  // ascending k within a thread
    const float J = a.disc[(e0 + k) * 4], C = a.disc[(e0 + k) * 4 + 1];
    if (J != J || C != C) continue;  // a NaN: neither feasible nor chosen
    const Best b{J, C, k};
    if (C <= budget) {
      ++cnt;
      if (better_j(b, bf)) bf = b;
    }
    if (better_c(b, bc)) bc = b;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const Best of = shfl_xor(bf, m), oc = shfl_xor(bc, m);
    if (better_j(of, bf)) bf = of;
    if (better_c(oc, bc)) bc = oc;
    cnt += __shfl_xor(cnt, m);
  }
  if (lane == 0) {
    red_f[wave] = bf;
    red_c[wave] = bc;
    red_n[wave] = cnt;
  }
  __syncthreads();
  bf = red_f[0];
  bc = red_c[0];
  cnt = red_n[0];
#pragma unroll
  for (int i = 1; i < kSelWaves; ++i) {  // (every thread: the result is uniform without another barrier)
    if (better_j(red_f[i], bf)) bf = red_f[i];
    if (better_c(red_c[i], bc)) bc = red_c[i];
    cnt += red_n[i];
  }
  const int kstar = cnt > 0 ? bf.k : (bc.k >= 0 ? bc.k : 0);  // (all K NaN: candidate 0)
  if (tid == 0) {
    a.chosen[n] = kstar;
    a.n_feasible[n] = cnt;
  }
  if (!(cnt > 0 && temp > 0.f)) {  // argmax, or the empty feasible set: row k* bit for bit
    const uint32_t* row = a.actions + (e0 + kstar) * (size_t)a.horizon * a.ad;
    for (int j = tid; j < a.ad; j += kSelThreads) a.action[(size_t)n * a.ad + j] = row[j];
    return;
  }
  // MPPI: w_k = expf((J_k - max_F J) / temperature) on F; the maximum has weight 1, so the denominator is >= 1
  for (int k = tid; k < K; k += kSelThreads) {
    const float J = a.disc[(e0 + k) * 4], C = a.disc[(e0 + k) * 4 + 1];
    w[k] = (J == J && C <= budget) ? (J == bf.j ? 1.f : expf((J - bf.j) / temp)) : 0.f;  // (J = max = +inf: still 1)
  }
  __syncthreads();
  const size_t pitch = (size_t)a.horizon * a.ad;
  const float* first = reinterpret_cast<const float*>(a.actions) + e0 * pitch;
  for (int j = tid; j < a.ad; j += kSelThreads) {
    double num = 0.0, den = 0.0;
    for (int k = 0; k < K; ++k) {  // ascending k, fp64: one order, one result
      const float wk = w[k];
      if (wk == 0.f) continue;  // (an infeasible candidate's action may be anything, a NaN included)
      den += (double)wk;
      num += (double)wk * (double)first[(size_t)k * pitch + j];
    }
    a.action[(size_t)n * a.ad + j] = __float_as_uint((float)(num / den));
  }
}

}  // namespace

extern "C" int osrl_plan_fanout(const float* states, int32_t slots, int32_t candidates, int32_t state_dim, float* state,
                                float* obs, int32_t obs_ld, float* acc, float* unc, float* disc, int32_t* halt_step,
                                void* stream) {
  if (!states || !state || !obs || !acc || !unc || !disc || slots < 1 || candidates < 1 ||
      candidates > OSRL_PLAN_MAX_CANDIDATES || state_dim < 1 || obs_ld < state_dim)
    return -1;
  const int64_t episodes = (int64_t)slots * candidates;
  if (episodes > INT32_MAX) return -1;
  const FanoutArgs a{states, state, obs, acc, unc, disc, halt_step, state_dim, obs_ld, candidates, (int32_t)episodes};
  return osrl_argmem::launch(plan_fanout_kernel, nullptr, dim3((unsigned)((episodes + kFanWaves - 1) / kFanWaves)),
                             dim3(kFanThreads), 0, (hipStream_t)stream, a);
}

extern "C" int osrl_plan_select(const float* actions, int32_t horizon, const float* disc, const float* budget,
                                const float* temperature, int32_t slots, int32_t candidates, int32_t action_dim,
                                float* action, int32_t* chosen, int32_t* n_feasible, void* stream) {
  if (!actions || !disc || !budget || !temperature || !action || !chosen || !n_feasible || horizon < 1 || slots < 1 ||
      candidates < 1 || candidates > OSRL_PLAN_MAX_CANDIDATES || action_dim < 1)
    return -1;
  if ((int64_t)slots * candidates > INT32_MAX) return -1;
  const SelectArgs a{reinterpret_cast<const uint32_t*>(actions), disc, budget, temperature,
                     reinterpret_cast<uint32_t*>(action), chosen, n_feasible, candidates, horizon, action_dim};
  return osrl_argmem::launch(plan_select_kernel, nullptr, dim3((unsigned)slots), dim3(kSelThreads), 0,
                             (hipStream_t)stream, a);
}
