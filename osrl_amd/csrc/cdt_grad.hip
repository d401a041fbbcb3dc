// cdt_grad.hip -- input gradients of the CDT token embeddings (osrl/algorithms/cdt.py:178-213) for the differentiable
// forward (ops.cdt_apply).
//
// The emb LayerNorm's backward leaves dseq [B, S, E], S = R*T + prefix: the gradient of every pre-LayerNorm token
// embedding.  Each token is an nn.Linear of one input (plus bias and timestep embedding), so the input gradients are
//   dstates[b,t,:]  = dseq[state token of (b,t)]  . W_state   ([E] x [E, od])
//   dactions[b,t,:] = dseq[action token of (b,t)] . W_action  ([E] x [E, ad])
//   dreturns[b,t]   = <dseq[return token], W_return[:, 0]>,  dcosts_to_go[b,t] = <dseq[cost token], W_cost[:, 0]>
//   depisode_cost[b] = <dseq[b, 0], W_prefix[:, 0]>          (the cost-prefix token)
// One workgroup per timestep (b, t): the R token rows (and the prefix row at t = 0) are staged in LDS, then every one
// of the od + ad + (1-wide) dot products is ONE wave's job: lane l sums features l, l + 64, ... in ascending order, a
// fixed butterfly adds the 64 partials.  Every output is written by exactly one lane: no atomics, and the summation
// order does not depend on the launch (bit-reproducible).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/osrl_amd.h"
#include "dev_util.h"

namespace {

constexpr int kMaxE = 1024;  // the CDT constructor's embedding_dim limit
constexpr int kWaves = 4;


struct InputGradArgs {
  const float *dseq, *Ws, *Wa, *Wr, *Wc, *Wp;
  float *dstates, *dactions, *dreturns, *dcost, *dprefix;
  int32_t B, T, od, ad, E, R, prefix, slot_rew, slot_cost;
};

__global__ __launch_bounds__(64 * kWaves) void cdt_embed_input_grad_kernel(const InputGradArgs a) {
  __shared__ float rows[5 * kMaxE];  // R <= 4 token rows + the prefix row: 20 KB
  const int bt = blockIdx.x;
  const int b = bt / a.T, t = bt - b * a.T;
  const int E = a.E, S = a.R * a.T + a.prefix;
  const bool pre = a.prefix && t == 0 && a.dprefix;
  const float* __restrict__ src = a.dseq + ((size_t)b * S + a.prefix + (size_t)t * a.R) * E;
  for (int i = threadIdx.x; i < a.R * E; i += 64 * kWaves) rows[i] = src[i];
  if (pre)
    for (int i = threadIdx.x; i < E; i += 64 * kWaves) rows[4 * kMaxE + i] = a.dseq[(size_t)b * S * E + i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_st = a.dstates ? a.od : 0, n_ac = a.dactions ? a.ad : 0;
  const int n_ret = a.dreturns ? 1 : 0, n_cost = a.dcost ? 1 : 0, n_pre = pre ? 1 : 0;
  const int n_out = n_st + n_ac + n_ret + n_cost + n_pre;
  for (int k = wave; k < n_out; k += kWaves) {
    // output k -> (token row in LDS, weight column, its stride, destination)
    const float* d;
    const float* w;
    int ldw;
    float* dst;
    if (k < n_st) {
      d = rows + (a.R - 2) * E, w = a.Ws + k, ldw = a.od, dst = a.dstates + (size_t)bt * a.od + k;
    } else if (k < n_st + n_ac) {
      const int j = k - n_st;
      d = rows + (a.R - 1) * E, w = a.Wa + j, ldw = a.ad, dst = a.dactions + (size_t)bt * a.ad + j;
    } else if (k < n_st + n_ac + n_ret) {
      d = rows + a.slot_rew * E, w = a.Wr, ldw = 1, dst = a.dreturns + bt;
    } else if (k < n_st + n_ac + n_ret + n_cost) {
      d = rows + a.slot_cost * E, w = a.Wc, ldw = 1, dst = a.dcost + bt;
    } else {
      d = rows + 4 * kMaxE, w = a.Wp, ldw = 1, dst = a.dprefix + b;
    }
    float s = 0.f;
    for (int f = lane; f < E; f += 64) s += d[f] * w[(size_t)f * ldw];
    s = wave_sum(s);
    if (lane == 0) *dst = s;
  }
}

}  // namespace

extern "C" {

int osrl_cdt_embed_input_grad(const float* dseq, const float* Ws, const float* Wa, const float* Wr, const float* Wc,
                              const float* Wp, int32_t B, int32_t T, int32_t od, int32_t ad, int32_t E,
                              int32_t use_rew, int32_t use_cost, int32_t prefix, float* dstates,
                              float* dactions, float* dreturns, float* dcosts_to_go, float* depisode_cost,
                              void* stream) {
  if (!dseq || B < 1 || T < 1 || od < 1 || ad < 1 || E < 1 || E > kMaxE) return -1;
  if ((dstates && !Ws) || (dactions && !Wa)) return -1;
  if (dreturns && (!use_rew || !Wr)) return -1;
  if (dcosts_to_go && (!use_cost || !Wc)) return -1;
  if (depisode_cost && (!prefix || !Wp)) return -1;
  const int R = 2 + (use_rew ? 1 : 0) + (use_cost ? 1 : 0);
  InputGradArgs a{dseq, Ws, Wa, Wr, Wc, Wp, dstates, dactions, dreturns, dcosts_to_go, depisode_cost, B, T, od, ad, E,
                  R, prefix ? 1 : 0, 0, use_rew ? 1 : 0};
  (void)hipGetLastError();
  hipLaunchKernelGGL(cdt_embed_input_grad_kernel, dim3((unsigned)(B * T)), dim3(64 * kWaves), 0,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
