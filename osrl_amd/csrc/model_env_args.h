// model_env_args.h -- the host side of the learned-dynamics environment step, shared by model_env.hip (one workgroup per
// tile) and model_env_split.hip (one per tile and member): the pieces their kernel descriptors are made of and the checks
// that fill them, so that osrl_model_env_step and osrl_model_env_step_split refuse the same arguments.  Plain structs and
// host functions only: the device code stays in each file (model_env_split.hip's top comment says why).  The namespace
// is anonymous, as in the two files: the kernels' names carry their descriptor types.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/osrl_amd.h"

namespace {

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

// what the Gaussian step adds to a descriptor (osrl_model_env_gauss_t beyond its osrl_model_env_t)
struct GaussArgs {
  const float* noise_in;
  float lo, hi;
  int32_t sample, unc;
};
struct NoGauss {};

// what the pessimistic step adds to a descriptor (osrl_model_env_pess_t, by value)
struct PessArgs {
  float halt_threshold, halt_reward, halt_cost, cost_penalty;
  int32_t* halt_step;
};
struct NoPess {};

// ---- the checks (false: a bad argument).  The argument arena (argmem.h) finds a block by its bytes, so a descriptor is
// zeroed as a whole -- memset(&a, 0, sizeof a) by the entry that owns the composite, fill_step for its own part -- before
// any field is set: no stray padding.
inline bool valid_member(const osrl_gemv_net_t& n, int in, int out) {
  if (n.n_layers < 1 || n.n_layers > OSRL_MAX_LAYERS || n.out_scale != 1.0f) return false;
  for (int l = 0; l <= n.n_layers; ++l)
    if (n.dims[l] < 1 || n.dims[l] > OSRL_MODEL_ENV_MAX_WIDTH) return false;
  for (int l = 0; l < n.n_layers; ++l)
    if (!n.Wf[l] || !n.b[l]) return false;
  return n.dims[0] == in && n.dims[n.n_layers] == out;
}

// the step's descriptor, checked
inline bool fill_step(StepArgs& a, const osrl_model_env_t* env, const float* act, float* state, float* obs,
                      int32_t obs_ld, float* acc, float* unc, float* step_out, int32_t episodes, bool gauss = false) {
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
  memset(&a, 0, sizeof a);
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

// the Gaussian additions, checked
inline bool fill_gauss(GaussArgs& g, const osrl_model_env_gauss_t* env) {
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

// the pessimistic additions, checked (+-inf thresholds are values like any other)
inline bool fill_pess(PessArgs& p, const osrl_model_env_pess_t* ps) {
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
