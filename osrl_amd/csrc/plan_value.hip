// plan_value.hip -- the terminal value of a planning call (engine/mpc.py ModelPlanner(terminal=...)): ONE launch between
// the last recorded model step and osrl_plan_select that closes every candidate's H-step sums with what an FQE's reward
// and cost critics say about the state the candidate ended in,
//   a_H = pi(obs_e);  Vr = reduce_m Q_r,m([obs_e, a_H]) r_mul;  Vc = reduce_m Q_c,m([obs_e, a_H]) c_mul;
//   J_e += gamma^H Vr,  C_e += gamma^H Vc        (a halted candidate: the absorbing state's tail halt_r / halt_c instead)
// where the launch chain of engine/fqe.py ValueReadout would be 3 to 5 launches of pure latency at N K = 64 .. 4096 rows.
//
//   plan_terminal_kernel (osrl_plan_terminal)  one workgroup of 8 waves per 16-candidate tile, act_vec.hip's shape: every
//       layer is v_mfma_f32_16x16x4_f32 over the packed PF[k/4][n][k%4] copies and the canonical biases, a wave walks ALL
//       of K for its 16-column tiles (no split-K), activations never leave LDS.  Three stages:
//       1. policy: the obs tile goes to columns 0 .. od of the critics' input tile `xin`; the policy net runs on all 8 waves
//          from it; the head (MLP: the net's own tanh; GAUSS: squashed_gauss at eps = 0) writes the action into columns
//          od .. od + ad of `xin`.  The action exists nowhere else.
//       2. critics: the 2 num_q nets share `xin` and are independent behind it.  Narrow instantiation (every width <= 256):
//          four members side by side, two waves and two ping-pong buffers (33 KB) each, ONE barrier per layer for all of
//          them; 2 num_q > 4 takes a second round.  Wide instantiation (<= OSRL_MAX_WIDTH): one member at a time on all 8
//          waves.  The one-output last layer is no MFMA layer (a 16-column pass for one column): lane (row, part p) of the
//          member's waves walks the k-quads p, p + P, .. of the last hidden activations as an fmaf chain, the P partials of
//          a row are added in ascending p by one lane.
//       3. one thread per candidate reduces the members in ascending order and applies the two fmaf to disc[e][0..1].
//       A candidate's numbers depend on the layer shapes and on the instantiation (both fixed by the widths) and on
//       nothing else: not on N, K, its tile, its row or its neighbours.  Rows past `episodes` are computed on zeros and not
//       stored.  Plain vector stores only (disc[e][0..1], last_V[e][0..1]); no blockDim / gridDim.
// The layer routine (plan_layer.h, shared with plan_value_quantile.hip as are stage 1 and the closing of the sums) is
// act_vec.hip's mfma_layer with the two strides and the wave group as parameters and the barrier left to the caller
// (members in different groups meet at one barrier); act_vec.hip is untouched.
// DESIGN.md "Terminal value at the horizon" keeps the registers / LDS of both instantiations.
#include "plan_layer.h"

namespace {

// The one-output last layer on the activations x (row stride XS; columns K .. round16(K) are zero, as the packed copy's
// are).  gl = the lane's index among the member's 64 nw lanes: row gl & 15, part p = gl >> 4 of NP = 4 nw.  Part p is the
// fmaf chain over the k-quads p, p + NP, .. in ascending k from +0; w[k] is column 0 of PF[k/4][16][k%4].
template <int XS>
__device__ __forceinline__ void head_parts(const float* __restrict__ PF, int K, const float* x, float* part, int gl,
                                           int NP) {
  const int row = gl & 15, p = gl >> 4, nq = round16(K) >> 2;
  const f32x4* __restrict__ W4 = reinterpret_cast<const f32x4*>(PF);
  float acc = 0.f;
  for (int q = p; q < nq; q += NP) {
    const f32x4 wv = W4[(size_t)q * 16];
    const f32x4 av = *reinterpret_cast<const f32x4*>(x + row * XS + 4 * q);
#pragma unroll
    for (int t = 0; t < 4; ++t) acc = __builtin_fmaf(av[t], wv[t], acc);
  }
  part[row * NP + p] = acc;
}

// W: widest layer of the policy and the critics; XW: widest critic input od + ad; MP: members side by side.
template <int W, int XW, int MP>
__global__ __launch_bounds__(kThreads) void plan_terminal_kernel(const TermArgs a) {
  constexpr int S = W + kPad, XS = XW + kPad, GW = kWaves / MP, NP = 4 * GW;
  static_assert(sizeof(float) * (kTile * XS + MP * 2 * kTile * S + MP * kTile * NP + kMaxCritics * kTile) <= 160 * 1024,
                "plan_terminal_kernel: LDS per workgroup");
  __shared__ __attribute__((aligned(16))) float xin[kTile * XS];        // [obs | pi(obs) | 0]: every critic's input
  __shared__ __attribute__((aligned(16))) float buf[MP][2][kTile * S];  // a member's ping-pong activations
  __shared__ float part[MP * kTile * NP];                               // the heads' partial dot products
  __shared__ float qv[kMaxCritics * kTile];                             // Q_m of the tile's rows
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int e0 = blockIdx.x * kTile;  // the tile's first candidate

  // ---- 1. the observation rows, the policy, its action into xin
  policy_stage<XS, S>(a, e0, w, xin, buf[0][0], buf[0][1]);

  // ---- 2. the critics: member n0 + g on the GW waves of group g
  const int g = w / GW, wv = w - g * GW, gl = wv * 64 + lane;
  const int nets = 2 * a.num_q, L = a.q[0].n_layers;
  for (int n0 = 0; n0 < nets; n0 += MP) {
    const int net = n0 + g;
    const bool on = net < nets;  // (wave-uniform; an idle group still meets the barriers)
    const osrl_gemv_net_t& qn = a.q[on ? net : 0];
    int c = 0;
    for (int l = 0; l < L - 1; ++l) {
      if (on) {
        if (l == 0) {
          wave_layer<XS, S>(qn.Wf[0], qn.b[0], qn.dims[0], qn.dims[1], qn.acts[0], 1.0f, xin, buf[g][0], wv, GW);
        } else {
          wave_layer<S, S>(qn.Wf[l], qn.b[l], qn.dims[l], qn.dims[l + 1], qn.acts[l], 1.0f, buf[g][c], buf[g][c ^ 1], wv,
                           GW);
        }
      }
      if (l > 0) c ^= 1;
      __syncthreads();
    }
    if (on) {
      if (L == 1)
        head_parts<XS>(qn.Wf[0], qn.dims[0], xin, part + g * kTile * NP, gl, NP);
      else
        head_parts<S>(qn.Wf[L - 1], qn.dims[L - 1], buf[g][c], part + g * kTile * NP, gl, NP);
    }
    __syncthreads();
    if (on && gl < kTile) {
      const float* pr = part + (g * kTile + gl) * NP;
      float s = 0.f;
      for (int q = 0; q < NP; ++q) s += pr[q];  // ascending part
      qv[net * kTile + gl] = act_fwd(qn.acts[L - 1], s + qn.b[L - 1][0]) * qn.out_scale;
    }
    __syncthreads();
  }

  // ---- 3. members in ascending order, then one fmaf per sum
  const int e = e0 + tid;
  if (tid >= kTile || e >= a.episodes) return;
  const int nq = a.num_q;
  float vr = qv[tid], vc = qv[nq * kTile + tid];
  for (int m = 1; m < nq; ++m) {
    const float r = qv[m * kTile + tid], c = qv[(nq + m) * kTile + tid];
    if (a.reduce == OSRL_PLAN_REDUCE_MEAN) {
      vr += r;
      vc += c;
    } else {  // pessimistic: the lowest return, the highest cost
      vr = fminf(vr, r);
      vc = fmaxf(vc, c);
    }
  }
  if (a.reduce == OSRL_PLAN_REDUCE_MEAN) {
    vr /= (float)nq;
    vc /= (float)nq;
  }
  vr *= a.r_mul;
  vc *= a.c_mul;
  close_sums(a, e, vr, vc);
}

}  // namespace

extern "C" int osrl_plan_terminal(const osrl_policy_t* policy, const osrl_gemv_net_t* critics, int32_t num_q,
                                  int32_t reduce, const float* obs, int32_t obs_ld, int32_t episodes, float r_mul,
                                  float c_mul, float halt_r, float halt_c, const int32_t* halt_step, float* disc,
                                  float* last_V, void* stream) {
  TermArgs a;
  bool wide = false;
  if (!term_args(policy, critics, num_q, 1, reduce, obs, obs_ld, episodes, r_mul, c_mul, halt_r, halt_c, halt_step, disc,
                 last_V, a, &wide))
    return -1;
  const dim3 grid((unsigned)((episodes + kTile - 1) / kTile));
  if (wide)
    return osrl_argmem::launch(plan_terminal_kernel<OSRL_MAX_WIDTH, kWideIn, 1>, nullptr, grid, dim3(kThreads), 0,
                               (hipStream_t)stream, a);
  return osrl_argmem::launch(plan_terminal_kernel<kNarrowW, kNarrowW, 4>, nullptr, grid, dim3(kThreads), 0,
                             (hipStream_t)stream, a);
}
