// rollout_step.h -- the pieces of one rollout step that every environment and act kernel shares, each written once: the
// exploration draw (collect.hip, cdt_collect.hip, model_env.hip, act_vec.hip, cdt_act.hip), the episode bookkeeping
// (those three and env.hip), the recorded row with its discounted sums and the liveness rule of the three recording
// kernels, and the host-side checks of their descriptors.  The paths agree bit for bit because they run this code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/osrl_amd.h"
#include "env_step.h"
#include "philox.h"

namespace osrl_rollout {

constexpr uint32_t kExploreStream = 13;  // Philox stream of the exploration noise (engine/collect.py _EPS_STREAM)

// eps of (episode id, the episode's own step, action column j): the injected value eps_in[idx] when there is one, else
// normal_word(philox4x32_10({episode id, step, j >> 2, stream}, key = (k0, k1)), j & 3) -- a function of nothing else.
// stream: the act paths draw on kExploreStream; a recording kernel passes its descriptor's stream_id (the C ABI's word,
// which engine/collect.py sets to the same 13).
__device__ __forceinline__ float explore_eps(uint32_t episode, uint32_t step, int j, uint32_t k0, uint32_t k1,
                                             const float* eps_in, size_t idx, uint32_t stream = kExploreStream) {
  if (eps_in) return eps_in[idx];
  const osrl_rng::U4 r = osrl_rng::philox4x32_10(osrl_rng::U4{episode, step, (uint32_t)(j >> 2), stream}, k0, k1);
  return osrl_rng::normal_word(r, j & 3);
}
// the same for a recording kernel: key and stream are the descriptor's; *seed is read only when the draw is made (it may
// be null beside eps_in).  C: osrl_collect_t behind whatever reference the kernel reaches it by.
template <class C>
__device__ __forceinline__ float explore_eps(const C& c, int ep, int step, int j, size_t idx) {
  if (c.eps_in) return c.eps_in[idx];
  const uint64_t s = *c.seed;
  return explore_eps(c.episode_base + (uint32_t)ep, (uint32_t)step, j, (uint32_t)s, (uint32_t)(s >> 32), nullptr, 0,
                     c.stream_id);
}

// v + sg * eps() in one rounding.  sg == 0 is the deterministic action exactly and eps() is not even called: nothing it
// would read (noise, key, episode id, step) is touched.  The clip that follows is the caller's.
template <class Eps>
__device__ __forceinline__ float explore(float v, float sg, Eps eps) {
  return sg != 0.f ? fmaf(sg, eps(), v) : v;
}

// One more step of the episode whose totals are ac = acc[ep] (return, cost * cost_scale, length, done latch); step_out,
// where given, takes the step's (reward, raw cost).  True when this was the episode's last step (the latch is then set).
__device__ __forceinline__ bool tick(float* ac, float rew, float cost, float cost_scale, int episode_len,
                                     float* step_out = nullptr) {
  const float len = ac[2] + 1.f;
  ac[0] += rew;
  ac[1] += cost * cost_scale;
  if (step_out) {
    step_out[0] = rew;
    step_out[1] = cost;
  }
  ac[2] = len;
  const bool last = len >= (float)episode_len;
  if (last) ac[3] = 1.f;
  return last;
}

// Whether a recording kernel may store for the episode with totals ac, and the step it is at.  Live = the done latch
// ac[3] is clear AND 0 <= step = ac[2] < episode_len.  This is why no write can leave the tables: a kernel stores only for
// live episodes ep < episodes, at row ep * episode_len + step < episodes * episode_len.  A captured graph replays whole
// chunks of steps and overshoots the episode's end; those launches find the episode not live and return before any store.
__device__ __forceinline__ bool live_step(const float* ac, int episode_len, int& step) {
  step = (int)ac[2];
  return ac[3] == 0.f && step >= 0 && step < episode_len;
}

// Row `row` of the four scalar tables and episode ep's discounted sums: one rounding per step each (fmaf), gamma^t by
// repeated multiplication.  C: osrl_collect_t behind whatever reference the kernel reaches it by.
template <class C>
__device__ __forceinline__ void record(const C& c, size_t row, int ep, float rew, float cost, float cost_scale,
                                       bool last) {
  c.rewards[row] = rew;
  c.costs[row] = cost;
  c.terminals[row] = 0.f;
  c.timeouts[row] = last ? 1.f : 0.f;
  float* dc = c.disc + (size_t)ep * 4;
  const float pw = dc[2];
  dc[0] = fmaf(pw, rew, dc[0]);
  dc[1] = fmaf(pw, cost * cost_scale, dc[1]);
  dc[2] = pw * *c.gamma;
}

// ---- host side: the descriptors' checks (false: a bad argument)
inline bool valid_env(const osrl_env_t* e, int obs_ld) {
  return e && e->state_dim >= 1 && e->state_dim <= osrl_env::kMaxDim && e->action_dim >= 1 &&
         e->action_dim <= osrl_env::kMaxAct && obs_ld >= e->state_dim && e->At && e->Bt && e->w && e->goal;
}
inline bool valid_collect(const osrl_collect_t* r) {
  return r && r->observations && r->actions && r->next_observations && r->rewards && r->costs && r->terminals &&
         r->timeouts && r->disc && r->sigma && r->gamma && (r->seed || r->eps_in);
}

}  // namespace osrl_rollout
