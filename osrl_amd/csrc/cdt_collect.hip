// cdt_collect.hip -- the CDT rollout step that makes data (engine/collect.py ``CDTCollector``): what the evaluating rollout
// does in four launches after the transformer forward (cdt_pick_kernel, env_step_kernel, cdt_push_kernel, the cursor) and
// what env_collect_kernel adds to a step (noise on the action, a table row, the discounted sums), as ONE launch.  One
// workgroup per episode, ceil(od / 64) * 64 lanes like env_step_kernel, so env_step.h's reduction sums the same partials in
// the same order and a run without noise is the evaluating rollout bit for bit.
//
// No shared cursor: an episode's step is its own t = acc[ep][2], the window holds n = min(t + 1, T) filled positions and
// the head row read is position n - 1.  No workgroup reads what another writes.
//
// No write can leave the tables by csrc/rollout_step.h's rule (live_step), nor the window: for a live episode every window
// position touched is < T, and the time step written is t + 1 <= episode_len (the embedding table has episode_len + T
// rows).
//
// The slide of a full window is one code path for every T: chunks of kPer * nt elements go through registers, each chunk
// read completely before any of it is written (its sources lie past everything written so far) -- cdt_push_kernel's
// register slide, widened; there is no LDS staging and so no second variant to keep equal.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/osrl_amd.h"
#include "rollout_step.h"

namespace {

namespace ro = osrl_rollout;

constexpr int kPer = 4;  // elements a lane carries per slide chunk

// in-place left shift p[i] = p[sh + i], i < n; every lane of the workgroup calls it (barriers inside)
template <typename V>
__device__ __forceinline__ void slide_left(V* p, int sh, int n, int t, int nt) {
  for (int c = 0; c < n; c += kPer * nt) {
    V v[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = c + u * nt + t;
      v[u] = i < n ? p[sh + i] : V(0);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = c + u * nt + t;
      if (i < n) p[i] = v[u];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void cdt_collect_kernel(osrl_env_t e, osrl_collect_t c, osrl_cdt_window_t w,
                                                          float* __restrict__ state, float* __restrict__ acc /*[E,4]*/,
                                                          int E, int nt) {
  __shared__ osrl_env::Lds l;
  const int ep = blockIdx.x, t = threadIdx.x;
  const int od = e.state_dim, ad = e.action_dim, L = e.episode_len, T = w.seq_len;
  float* st = state + (size_t)ep * od;
  float* ac = acc + (size_t)ep * 4;
  int step;
  if (!ro::live_step(ac, L, step)) return;  // uniform per workgroup, ahead of every barrier and every store
  const int n = min(step + 1, T);                     // filled window positions; the step being taken is position n - 1
  float* S = w.states + (size_t)ep * T * od;
  float* A = w.actions + (size_t)ep * T * ad;
  float* R = w.returns + (size_t)ep * T;
  float* C = w.costs_to_go + (size_t)ep * T;
  int64_t* TS = w.time_steps + (size_t)ep * T;
  if (t < od) l.s[t] = st[t];
  if (t < ad) {
    const float* h = w.head + ((size_t)ep * T + (n - 1)) * w.head_width;
    const float sg = w.sample ? expf(h[ad + t]) : c.sigma[ep];  // head rows are [mu | log_std], no log-std bounds
    const float v = ro::explore(h[t] /* mu (cdt.py:489-493) */, sg,
                                [&] { return ro::explore_eps(c, ep, step, t, ((size_t)step * E + ep) * ad + t); });
    l.a[t] = osrl_env::clip_action(v, e.max_action);
  }
  __syncthreads();
  const float sn = osrl_env::advance(e, l, t);
  const size_t row = (size_t)ep * L + step;
  if (t < od) {
    st[t] = sn;
    c.observations[row * od + t] = l.s[t];
    c.next_observations[row * od + t] = sn;
  }
  if (t < ad) {
    c.actions[row * ad + t] = l.a[t];
    A[(size_t)(n - 1) * ad + t] = l.a[t];  // the window records the action actually taken
  }
  float r_new = 0.f, c_new = 0.f;  // lane 0's: the to-go values of the appended step
  if (t == 0) {
    float rew, cost;
    osrl_env::outcome(e, l, rew, cost);
    ro::record(c, row, ep, rew, cost, e.cost_scale, ro::tick(ac, rew, cost, e.cost_scale, L));
    // to-go values: cdt_push_kernel's arithmetic (cdt.py:507-508), read before the slide moves them
    const float cw = (w.cost_reverse ? 1.f - cost : cost) * w.cost_scale;
    r_new = R[n - 1] - rew;
    c_new = C[n - 1] - cw;
  }
  __syncthreads();  // A[n - 1] and lane 0's reads are done before the slide
  int pos = n;
  if (n == T) {  // (uniform)
    slide_left(S, od, (T - 1) * od, t, nt);
    slide_left(A, ad, (T - 1) * ad, t, nt);
    slide_left(R, 1, T - 1, t, nt);
    slide_left(C, 1, T - 1, t, nt);
    slide_left(TS, 1, T - 1, t, nt);
    pos = T - 1;
  }
  if (t < od) S[(size_t)pos * od + t] = sn;
  if (t < ad) A[(size_t)pos * ad + t] = 0.f;  // "last action is dummy with zeros"
  if (t == 0) {
    R[pos] = r_new;
    C[pos] = c_new;
    TS[pos] = step + 1;
    w.mask[(size_t)ep * T + pos] = 1.f;
  }
}

}  // namespace

extern "C" int osrl_cdt_collect(const osrl_env_t* env, const osrl_collect_t* rec, const osrl_cdt_window_t* win,
                                float* state, float* acc, int32_t episodes, void* stream) {
  if (!env || !win || !state || !acc || episodes < 1) return -1;
  if (!ro::valid_env(env, env->state_dim /* no obs rows here */) || env->episode_len < 1 || !ro::valid_collect(rec))
    return -1;
  if (!win->states || !win->actions || !win->returns || !win->costs_to_go || !win->time_steps || !win->mask ||
      !win->head || win->seq_len < 1 || win->seq_len > 1024 ||
      win->head_width < (win->sample ? 2 : 1) * env->action_dim)
    return -1;
  (void)hipGetLastError();
  const int threads = ((env->state_dim + 63) / 64) * 64;  // osrl_env_step's shape: env_step.h sums blockDim / 64 partials
  hipLaunchKernelGGL(cdt_collect_kernel, dim3(episodes), dim3(threads), 0, (hipStream_t)stream, *env, *rec, *win, state,
                     acc, episodes, threads);
  return (int)hipGetLastError();
}
