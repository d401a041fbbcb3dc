// collect.hip -- the rollout step that makes data (engine/collect.py): env_step_kernel's step with per-episode
// exploration noise on the action, recorded as one row of a DSRL-layout dataset in HBM, plus the discounted sums the
// FQE estimate is stated in.  One workgroup per episode, ceil(od / 64) * 64 lanes, like env_step_kernel; the environment
// arithmetic is the shared csrc/env_step.h, and the noise, the bookkeeping, the recorded row and the rule by which no write
// can leave the tables (live_step) are csrc/rollout_step.h's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/osrl_amd.h"
#include "rollout_step.h"

namespace {

namespace ro = osrl_rollout;

__global__ __launch_bounds__(256) void env_collect_kernel(osrl_env_t e, osrl_collect_t c, const float* __restrict__ act,
                                                          float* __restrict__ state, float* __restrict__ obs, int obs_ld,
                                                          float* __restrict__ acc /*[E,4]*/, int E) {
  __shared__ osrl_env::Lds l;
  const int ep = blockIdx.x, t = threadIdx.x;
  const int od = e.state_dim, ad = e.action_dim, L = e.episode_len;
  float* st = state + (size_t)ep * od;
  float* ac = acc + (size_t)ep * 4;
  int step;
  if (!ro::live_step(ac, L, step)) return;  // uniform per workgroup, ahead of every barrier and every store
  if (t < od) l.s[t] = st[t];
  if (t < ad) {
    const float v = ro::explore(act[(size_t)ep * ad + t], c.sigma[ep],
                                [&] { return ro::explore_eps(c, ep, step, t, ((size_t)step * E + ep) * ad + t); });
    l.a[t] = osrl_env::clip_action(v, e.max_action);
  }
  __syncthreads();
  const float sn = osrl_env::advance(e, l, t);
  const size_t row = (size_t)ep * L + step;
  if (t < od) {
    st[t] = sn;
    obs[(size_t)ep * obs_ld + t] = sn;
    c.observations[row * od + t] = l.s[t];
    c.next_observations[row * od + t] = sn;
  }
  if (t < ad) c.actions[row * ad + t] = l.a[t];
  if (t == 0) {
    float rew, cost;
    osrl_env::outcome(e, l, rew, cost);
    ro::record(c, row, ep, rew, cost, e.cost_scale, ro::tick(ac, rew, cost, e.cost_scale, L));
  }
}

}  // namespace

extern "C" int osrl_env_collect(const osrl_env_t* env, const osrl_collect_t* rec, const float* act, float* state,
                                float* obs, int32_t obs_ld, float* acc, int32_t episodes, void* stream) {
  if (!act || !state || !obs || !acc || episodes < 1) return -1;
  if (!ro::valid_env(env, obs_ld) || env->episode_len < 1 || !ro::valid_collect(rec)) return -1;
  (void)hipGetLastError();
  const int threads = ((env->state_dim + 63) / 64) * 64;
  hipLaunchKernelGGL(env_collect_kernel, dim3(episodes), dim3(threads), 0, (hipStream_t)stream, *env, *rec, act, state,
                     obs, obs_ld, acc, episodes);
  return (int)hipGetLastError();
}
