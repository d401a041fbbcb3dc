// collect.hip -- the rollout step that makes data (engine/collect.py): env_step_kernel's step with per-episode
// exploration noise on the action, recorded as one row of a DSRL-layout dataset in HBM, plus the discounted sums the
// FQE estimate is stated in.  One workgroup per episode, ceil(od / 64) * 64 lanes, like env_step_kernel; the environment
// arithmetic is the shared csrc/env_step.h.
//
// Why no write can leave the tables: a workgroup writes only while its episode's done latch (acc[ep][3]) is clear AND
// its step t = acc[ep][2] is below episode_len; then row ep * episode_len + t < episodes * episode_len.  The captured
// graph replays whole chunks of steps and overshoots the episode's end: those launches return before any store.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/osrl_amd.h"
#include "env_step.h"
#include "philox.h"

namespace {

using namespace osrl_rng;

__global__ __launch_bounds__(256) void env_collect_kernel(osrl_env_t e, osrl_collect_t c, const float* __restrict__ act,
                                                          float* __restrict__ state, float* __restrict__ obs, int obs_ld,
                                                          float* __restrict__ acc /*[E,4]*/, int E) {
  __shared__ osrl_env::Lds l;
  const int ep = blockIdx.x, t = threadIdx.x;
  const int od = e.state_dim, ad = e.action_dim, L = e.episode_len;
  float* st = state + (size_t)ep * od;
  float* ac = acc + (size_t)ep * 4;
  const int step = (int)ac[2];
  if (ac[3] != 0.f || step < 0 || step >= L) return;  // uniform per workgroup, ahead of every barrier and every store
  if (t < od) l.s[t] = st[t];
  if (t < ad) {
    float v = act[(size_t)ep * ad + t];
    const float sg = c.sigma[ep];
    if (sg != 0.f) {  // (sigma == 0: the deterministic action exactly; eps is not even read)
      float eps;
      if (c.eps_in) {
        eps = c.eps_in[((size_t)step * E + ep) * ad + t];
      } else {
        const uint64_t seed = *c.seed;
        const U4 r = philox4x32_10(U4{c.episode_base + (uint32_t)ep, (uint32_t)step, (uint32_t)(t >> 2), c.stream_id},
                                   (uint32_t)seed, (uint32_t)(seed >> 32));
        eps = normal_word(r, t & 3);
      }
      v = fmaf(sg, eps, v);
    }
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
    const float len = ac[2] + 1.f;
    ac[0] += rew;
    ac[1] += cost * e.cost_scale;
    ac[2] = len;
    const bool last = len >= (float)L;
    if (last) ac[3] = 1.f;
    c.rewards[row] = rew;
    c.costs[row] = cost;
    c.terminals[row] = 0.f;
    c.timeouts[row] = last ? 1.f : 0.f;
    // discounted sums: one rounding per step each (fmaf), gamma^t by repeated multiplication
    float* dc = c.disc + (size_t)ep * 4;
    const float pw = dc[2];
    dc[0] = fmaf(pw, rew, dc[0]);
    dc[1] = fmaf(pw, cost * e.cost_scale, dc[1]);
    dc[2] = pw * *c.gamma;
  }
}

}  // namespace

extern "C" int osrl_env_collect(const osrl_env_t* env, const osrl_collect_t* rec, const float* act, float* state,
                                float* obs, int32_t obs_ld, float* acc, int32_t episodes, void* stream) {
  if (!env || !rec || !act || !state || !obs || !acc || episodes < 1) return -1;
  if (env->state_dim < 1 || env->state_dim > osrl_env::kMaxDim || env->action_dim < 1 ||
      env->action_dim > osrl_env::kMaxAct || obs_ld < env->state_dim || env->episode_len < 1 || !env->At || !env->Bt ||
      !env->w || !env->goal)
    return -1;
  if (!rec->observations || !rec->actions || !rec->next_observations || !rec->rewards || !rec->costs ||
      !rec->terminals || !rec->timeouts || !rec->disc || !rec->sigma || !rec->gamma || (!rec->seed && !rec->eps_in))
    return -1;
  (void)hipGetLastError();
  const int threads = ((env->state_dim + 63) / 64) * 64;
  hipLaunchKernelGGL(env_collect_kernel, dim3(episodes), dim3(threads), 0, (hipStream_t)stream, *env, *rec, act, state,
                     obs, obs_ld, acc, episodes);
  return (int)hipGetLastError();
}
