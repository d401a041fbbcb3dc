// plan_layer.h -- what the planner's two terminal launches share (plan_value.hip osrl_plan_terminal, one-output critics;
// plan_value_quantile.hip osrl_plan_terminal_quantile, M-output critics): the workgroup's shape, the launch arguments,
// the MFMA layer on a 16-row LDS tile, stage 1 (the policy's action into the critics' input tile), the closing of a
// candidate's sums and the host's judgement of the descriptors.  Each kernel keeps its own critics' stage and its own
// member reduction.  Everything is internal to the including translation unit.
#pragma once
#include "argmem.h"
#include "policy_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 512, kWaves = 8, kTile = 16;
constexpr int kPad = 4;  // floats: rows 16 bytes apart in the banks (act_vec.hip)
constexpr int kMaxQ = OSRL_PLAN_TERMINAL_MAX_Q, kMaxCritics = 2 * kMaxQ;
// narrow: every width (policy, critics, od + ad) <= kNarrowW, four members in parallel; wide: widths <= OSRL_MAX_WIDTH, an
// input tile of od + ad <= OSRL_PLAN_TERMINAL_WIDE_INPUT columns beside the two 1024-wide buffers
constexpr int kNarrowW = OSRL_PLAN_TERMINAL_NARROW, kWideIn = OSRL_PLAN_TERMINAL_WIDE_INPUT;

struct TermArgs {
  osrl_policy_t p;
  osrl_gemv_net_t q[kMaxCritics];  // reward members 0 .. num_q - 1, then the cost members
  const float* obs;                // [episodes, obs_ld]
  const int32_t* halt_step;        // [episodes] or nullptr
  float *disc, *last_V;            // [episodes, 4], [episodes, 2]
  int32_t obs_ld, episodes, num_q, reduce;
  float r_mul, c_mul, halt_r, halt_c;
};

// y[r][n] = act(b[n] + sum_k W[n][k] x[r][k]) * scale for the tile's 16 rows; x (row stride XS), y (row stride YS) in LDS.
// Wave wv of the nw waves that share this layer takes column tiles wv, wv + nw (one pass), wv + 2 nw, ..; lane (ar, kq)
// holds A = x[ar][16 kb + 4 kq + t], B = W[n0 + ar][16 kb + 4 kq + t]; accumulator element i is y[4 kq + i][n0 + ar].
// Columns out .. round16(out) are written as zero (the next layer's k padding).  No barrier: the caller's.
template <int XS, int YS>
__device__ __forceinline__ void wave_layer(const float* __restrict__ PF, const float* __restrict__ b, int in, int out,
                                           int act, float scale, const float* x, float* y, int wv, int nw) {
  constexpr int kC = 8;
  const int lane = threadIdx.x & 63, ar = lane & 15, kq = lane >> 4;
  const int Np = round16(out), nkb = round16(in) >> 4, nct = Np >> 4;
  const f32x4* __restrict__ W4 = reinterpret_cast<const f32x4*>(PF);
  const float* xr = x + ar * XS + 4 * kq;
  for (int c0 = wv; c0 < nct; c0 += 2 * nw) {
    const int c1 = c0 + nw;
    const bool two = c1 < nct;  // (wave-uniform)
    const f32x4* __restrict__ p0 = W4 + (size_t)kq * Np + 16 * c0 + ar;
    const f32x4* __restrict__ p1 = W4 + (size_t)kq * Np + 16 * (two ? c1 : c0) + ar;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < nkb; kc += kC) {  // kC k-blocks per round: every load is issued before the round's first MFMA
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
      for (int i = 0; i < 4; ++i) y[(4 * kq + i) * YS + col] = col < out ? act_fwd(act, acc0[i] + bb) * scale : 0.f;
    }
    if (two) {
      const int col = 16 * c1 + ar;
      const float bb = col < out ? b[col] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) y[(4 * kq + i) * YS + col] = col < out ? act_fwd(act, acc1[i] + bb) * scale : 0.f;
    }
  }
}

// Stage 1 of both kernels, on all 8 waves: the tile's observation rows (rows past `episodes`: zeros) into columns
// 0 .. od of xin, the policy net from there through the ping-pong pair pp0 / pp1 (row stride S), the head's action (MLP:
// the net's own tanh; GAUSS: squashed_gauss at eps = 0) into columns od .. od + ad.  Ends behind a barrier.
template <int XS, int S>
__device__ __forceinline__ void policy_stage(const TermArgs& a, int e0, int w, float* xin, float* pp0, float* pp1) {
  const int tid = threadIdx.x;
  const osrl_policy_t& p = a.p;
  const int od = p.obs_dim, ad = p.act_dim;
  const int xw = round16(od + ad);
  for (int i = tid; i < kTile * xw; i += kThreads) {
    const int r = i / xw, c = i - r * xw, e = e0 + r;
    xin[r * XS + c] = (c < od && e < a.episodes) ? a.obs[(size_t)e * a.obs_ld + c] : 0.f;
  }
  __syncthreads();
  const osrl_gemv_net_t& pn = p.net[0];
  int cur = 0;
  for (int l = 0; l < pn.n_layers; ++l) {
    const float sc = l == pn.n_layers - 1 ? pn.out_scale : 1.0f;
    if (l == 0) {
      wave_layer<XS, S>(pn.Wf[0], pn.b[0], pn.dims[0], pn.dims[1], pn.acts[0], sc, xin, pp0, w, kWaves);
    } else {
      wave_layer<S, S>(pn.Wf[l], pn.b[l], pn.dims[l], pn.dims[l + 1], pn.acts[l], sc, cur ? pp1 : pp0, cur ? pp0 : pp1, w,
                       kWaves);
      cur ^= 1;
    }
    __syncthreads();
  }
  for (int i = tid; i < kTile * ad; i += kThreads) {
    const int r = i / ad, j = i - r * ad;
    const float* h = (cur ? pp1 : pp0) + r * S;
    float v = h[j];  // OSRL_POLICY_MLP: tanh and act_limit are the net's last layer
    if (p.kind == OSRL_POLICY_GAUSS) {
      float lp = 0.f;
      squashed_gauss(h[j], h[ad + j], 0.f, p.max_action, &v, lp);
    }
    xin[r * XS + od + j] = v;
  }
  __syncthreads();
}

// The last step of both kernels, candidate e's own thread: last_V[e] = (vr, vc) and the two fmaf into disc[e][0..1]
// (a halted candidate: the absorbing state's tail).
__device__ __forceinline__ void close_sums(const TermArgs& a, int e, float vr, float vc) {
  a.last_V[(size_t)e * 2] = vr;
  a.last_V[(size_t)e * 2 + 1] = vc;
  float* dc = a.disc + (size_t)e * 4;
  const bool halted = a.halt_step && a.halt_step[e] >= 0;
  const float pw = dc[2];
  dc[0] = fmaf(pw, halted ? a.halt_r : vr, dc[0]);
  dc[1] = fmaf(pw, halted ? a.halt_c : vc, dc[1]);
}

inline int widest(const osrl_gemv_net_t& n) {
  int m = 0;
  for (int l = 0; l <= n.n_layers; ++l) m = n.dims[l] > m ? n.dims[l] : m;
  return m;
}

// What either entry point refuses, with `out_w` the critics' last width; on true `a` is filled and *wide says which
// instantiation the widths take.
inline bool term_args(const osrl_policy_t* policy, const osrl_gemv_net_t* critics, int32_t num_q, int32_t out_w,
                      int32_t reduce, const float* obs, int32_t obs_ld, int32_t episodes, float r_mul, float c_mul,
                      float halt_r, float halt_c, const int32_t* halt_step, float* disc, float* last_V, TermArgs& a,
                      bool* wide) {
  int noise_dim = 0;
  if (!policy || !critics || !obs || !disc || !last_V || episodes < 1 || num_q < 1 || num_q > kMaxQ ||
      (reduce != OSRL_PLAN_REDUCE_MEAN && reduce != OSRL_PLAN_REDUCE_PESSIMISTIC))
    return false;
  const osrl_policy_t& p = *policy;
  if (!valid_policy(p, &noise_dim) || p.kind == OSRL_POLICY_BCQ || obs_ld < p.obs_dim) return false;
  int wmax = widest(p.net[0]);
  const osrl_gemv_net_t& q0 = critics[0];
  for (int m = 0; m < 2 * num_q; ++m) {  // one shape for all members: they meet at the same barriers
    const osrl_gemv_net_t& q = critics[m];
    if (!valid_net(q) || q.n_layers != q0.n_layers || q.dims[0] != p.obs_dim + p.act_dim || q.dims[q.n_layers] != out_w)
      return false;
    for (int l = 0; l < q.n_layers; ++l)
      if (q.dims[l] != q0.dims[l] || q.acts[l] != q0.acts[l]) return false;
  }
  wmax = widest(q0) > wmax ? widest(q0) : wmax;  // (valid_net: every width <= OSRL_MAX_WIDTH)
  *wide = wmax > kNarrowW;
  if (*wide && p.obs_dim + p.act_dim > kWideIn) return false;
  memset(&a, 0, sizeof a);
  a.p = p;
  memset(&a.p.net[1], 0, sizeof a.p.net[1]);
  for (int m = 0; m < 2 * num_q; ++m) a.q[m] = critics[m];
  a.obs = obs;
  a.halt_step = halt_step;
  a.disc = disc;
  a.last_V = last_V;
  a.obs_ld = obs_ld;
  a.episodes = episodes;
  a.num_q = num_q;
  a.reduce = reduce;
  a.r_mul = r_mul;
  a.c_mul = c_mul;
  a.halt_r = halt_r;
  a.halt_c = halt_c;
  return true;
}

}  // namespace
