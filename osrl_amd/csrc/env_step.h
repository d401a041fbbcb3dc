// env_step.h -- one step of the synthetic safe environment for one episode (= one workgroup), shared by env_step_kernel
// (env.hip), env_collect_kernel (collect.hip) and cdt_collect_kernel (cdt_collect.hip): they must agree bit for bit, so the
// arithmetic exists once.  What a step does besides the environment's arithmetic is csrc/rollout_step.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/osrl_amd.h"

namespace osrl_env {

constexpr int kMaxDim = 256;
constexpr int kMaxAct = 64;

struct Lds {
  float s[kMaxDim];  // the state before the step
  float a[kMaxAct];  // the clipped action
  float red[2][4];   // per-wave partial sums of |s' - goal|^2 and s'.w
};

__device__ __forceinline__ float clip_action(float v, float max_action) {
  return fminf(fmaxf(v, -max_action), max_action);
}

// Lane t's component of s' = A s + Bm a (0 for t >= state_dim).  The caller has filled l.s / l.a and passed a barrier;
// on return (after another barrier) l.red holds the reduction partials that `outcome` sums.  Every lane of the
// workgroup must call this.
__device__ __forceinline__ float advance(const osrl_env_t& e, Lds& l, int t) {
  const int od = e.state_dim, ad = e.action_dim;
  float sn = 0.f, d2 = 0.f, sw = 0.f;
  if (t < od) {
    // At / Bt are stored transposed: lane t reads column t of each row -> coalesced, L2-resident for all episodes
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
    int j = 0;
    for (; j + 4 <= od; j += 4) {
      p0 = fmaf(e.At[(size_t)(j + 0) * od + t], l.s[j + 0], p0);
      p1 = fmaf(e.At[(size_t)(j + 1) * od + t], l.s[j + 1], p1);
      p2 = fmaf(e.At[(size_t)(j + 2) * od + t], l.s[j + 2], p2);
      p3 = fmaf(e.At[(size_t)(j + 3) * od + t], l.s[j + 3], p3);
    }
    for (; j < od; ++j) p0 = fmaf(e.At[(size_t)j * od + t], l.s[j], p0);
    float sb = 0.f;
    for (int k = 0; k < ad; ++k) sb = fmaf(e.Bt[(size_t)k * od + t], l.a[k], sb);
    sn = ((p0 + p1) + (p2 + p3)) + sb;
    const float d = sn - e.goal[t];
    d2 = d * d;
    sw = sn * e.w[t];
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    d2 += __shfl_xor(d2, o);
    sw += __shfl_xor(sw, o);
  }
  if ((t & 63) == 0) {
    l.red[0][t >> 6] = d2;
    l.red[1][t >> 6] = sw;
  }
  __syncthreads();
  return sn;
}

// this step's reward and raw 0/1 cost from the partials `advance` left (one lane calls it)
__device__ __forceinline__ void outcome(const osrl_env_t& e, const Lds& l, float& rew, float& cost) {
  const int nw = (blockDim.x + 63) >> 6;
  float D = 0.f, W = 0.f;
  for (int i = 0; i < nw; ++i) {
    D += l.red[0][i];
    W += l.red[1][i];
  }
  rew = 1.f - 0.1f * D;
  cost = W > e.cost_threshold ? 1.f : 0.f;
}

}  // namespace osrl_env
