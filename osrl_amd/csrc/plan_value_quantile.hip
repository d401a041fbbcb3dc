// plan_value_quantile.hip -- the DISTRIBUTIONAL terminal value of a planning call (engine/mpc.py ModelPlanner(terminal=
// <quantile FQE>, risk_alpha=)): plan_value.hip's one launch between the last recorded model step and osrl_plan_select,
// for critics whose last layer holds the M quantiles theta_0 .. theta_{M-1} of the return from (s_H, pi(s_H)).  Every
// candidate's sums are closed with a tail mean of its OWN row's quantiles,
//   Vr = reduce_m CVaR^lower_{k_r}(theta_r,m) r_mul,   Vc = reduce_m CVaR^upper_{k_c}(theta_c,m) c_mul,
// where engine/fqe.py QuantileReadout + osrl_fqe_quantile_sums reduce over the rows of a store and give one number per net.
//
//   plan_terminal_quantile_kernel (osrl_plan_terminal_quantile)  one workgroup of 8 waves per 16-candidate tile, the two
//       instantiations of plan_terminal_kernel (narrow: four members side by side on two waves each; wide: one member on
//       all 8 waves).  Four stages:
//       1. policy (plan_layer.h policy_stage, shared): pi(obs) into columns od .. od + ad of the critics' input tile xin.
//       2. critics: ALL L layers are MFMA layers (plan_layer.h wave_layer).  The last one has M outputs, round16(M) / 16
//          <= 4 column tiles for the member's waves, and leaves theta[16][round16(M)] in the member's free ping-pong
//          buffer (L == 1: xin -> buf[g][0]) with bias, activation and out_scale applied -- where the one-output head of
//          the scalar kernel is an fmaf chain because a 16-column pass for one column wastes 15/16 of the matrix core,
//          here a pass is 1/8 (M = 2) to fully used (M = 16, 32, 48, 64), and the chain would be M chains.
//       3. sort and tails, per member behind the head's barrier: a SEGMENT is P = 2^ceil(log2 M) adjacent lanes, 64 / P per
//          wave; the member's waves hold nw 64 / P segments, segment s takes rows s, s + n_seg, ..  Lanes i < M load
//          theta_i from LDS, lanes past M hold +inf; a bitonic network over the segment's lanes (__shfl_xor: registers to
//          registers, no LDS round trip) leaves rank i in lane i; the M ranks are read back ascending by lane broadcast
//          and added in fp64 in that order three times over: all M, ranks 0 .. k_r - 1, ranks M - k_c .. M - 1
//          (quantile_sums_kernel's order and precision); each sum is divided in fp64 and rounded to fp32 ONCE into
//          qv[member][row][3].  A row with a NaN among its M values (a ballot before the sort: the network never orders
//          a NaN) gets three NaNs.
//       4. one thread per candidate: the members in ascending order (mean; pessimistic = min of the reward members'
//          lower tails, max of the cost members' upper tails), r_mul / c_mul, last_V, the same reduction of the all-M
//          means into last_V_mean, and the two fmaf into disc[e][0..1] (plan_layer.h close_sums, shared).
//       A candidate's numbers depend on the layer shapes, M, k_r, k_c and the instantiation, and on nothing else: not on
//       N, K, its tile, its row or its neighbours (the segment a row falls into changes which lanes sort it, not what they
//       compute).  Rows past `episodes` are computed on zeros and not stored.  Plain vector stores only; no blockDim /
//       gridDim; static LDS: the scalar kernel's xin and buffers, the 1536 B qv table in place of its partials.
// DESIGN.md "A distributional terminal value" keeps the registers / LDS of both instantiations.
#include <math.h>

#include "plan_layer.h"

namespace {

struct QTermArgs {
  TermArgs t;
  float* last_V_mean;            // [episodes, 2]
  int32_t M, log2p, k_r, k_c;  // P = 1 << log2p lanes per segment
};

// theta: the member's [16][S] tile in LDS; q: its [16][3] rows of qv.  wv of the member's nw waves.
template <int S>
__device__ __forceinline__ void sort_tails(const float* theta, int M, int log2p, int k_r, int k_c, float* q, int wv, int nw) {
  const int lane = threadIdx.x & 63;
  const int P = 1 << log2p, G = 64 >> log2p;  // lanes per segment, segments per wave
  const int seg = lane >> log2p, i = lane & (P - 1), first = seg << log2p;
  const int sg = wv * G + seg, n_seg = nw * G;
  const unsigned long long seg_mask = (P == 64 ? ~0ull : (1ull << P) - 1ull) << first;
  for (int r0 = 0; r0 < kTile; r0 += n_seg) {  // (the same trip count in every lane: the shuffles see whole waves)
    const int r = r0 + sg;
    const bool valid = r < kTile;
    float v = (valid && i < M) ? theta[r * S + i] : INFINITY;
    const bool bad = (__ballot(v != v) & seg_mask) != 0ull;  // (uniform over the segment)
    v = v != v ? INFINITY : v;
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
      for (int j = k2 >> 1; j > 0; j >>= 1) {
        const float o = __shfl_xor(v, j);
        const bool keep_min = ((i & j) == 0) == ((i & k2) == 0);  // the lower lane of a pair in an ascending run
        v = keep_min ? fminf(v, o) : fmaxf(v, o);
      }
    }
    double all = 0.0, lo = 0.0, hi = 0.0;
    for (int k = 0; k < M; ++k) {  // ascending ranks
      const double x = (double)__shfl(v, first + k);
      all += x;
      if (k < k_r) lo += x;
      if (k >= M - k_c) hi += x;
    }
    if (valid && i == 0) {
      const float nan = __builtin_nanf("");
      q[r * 3] = bad ? nan : (float)(all / (double)M);
      q[r * 3 + 1] = bad ? nan : (float)(lo / (double)k_r);
      q[r * 3 + 2] = bad ? nan : (float)(hi / (double)k_c);
    }
  }
}

// W: widest layer of the policy and the critics; XW: widest critic input od + ad; MP: members side by side.
template <int W, int XW, int MP>
__global__ __launch_bounds__(kThreads) void plan_terminal_quantile_kernel(const QTermArgs qa) {
  constexpr int S = W + kPad, XS = XW + kPad, GW = kWaves / MP;
  static_assert(sizeof(float) * (kTile * XS + MP * 2 * kTile * S + kMaxCritics * kTile * 3) <= 160 * 1024,
                "plan_terminal_quantile_kernel: LDS per workgroup");
  static_assert(OSRL_FQE_MAX_QUANTILES <= 64 && OSRL_FQE_MAX_QUANTILES <= W, "a row's quantiles: one wave, one buffer row");
  __shared__ __attribute__((aligned(16))) float xin[kTile * XS];        // [obs | pi(obs) | 0]: every critic's input
  __shared__ __attribute__((aligned(16))) float buf[MP][2][kTile * S];  // a member's ping-pong activations, then theta
  __shared__ float qv[kMaxCritics * kTile * 3];                         // [member][row]: mean, lower tail, upper tail
  const TermArgs& a = qa.t;
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int e0 = blockIdx.x * kTile;  // the tile's first candidate

  // ---- 1. the observation rows, the policy, its action into xin
  policy_stage<XS, S>(a, e0, w, xin, buf[0][0], buf[0][1]);

  // ---- 2. the critics, member n0 + g on the GW waves of group g: every layer on MFMA, theta ends in buf[g][c]
  const int g = w / GW, wv = w - g * GW;
  const int nets = 2 * a.num_q, L = a.q[0].n_layers;
  for (int n0 = 0; n0 < nets; n0 += MP) {
    const int net = n0 + g;
    const bool on = net < nets;  // (wave-uniform; an idle group still meets the barriers)
    const osrl_gemv_net_t& qn = a.q[on ? net : 0];
    int c = 0;
    for (int l = 0; l < L; ++l) {
      if (on) {
        const float sc = l == L - 1 ? qn.out_scale : 1.0f;
        if (l == 0) {
          wave_layer<XS, S>(qn.Wf[0], qn.b[0], qn.dims[0], qn.dims[1], qn.acts[0], sc, xin, buf[g][0], wv, GW);
        } else {
          wave_layer<S, S>(qn.Wf[l], qn.b[l], qn.dims[l], qn.dims[l + 1], qn.acts[l], sc, buf[g][c], buf[g][c ^ 1], wv,
                           GW);
        }
      }
      if (l > 0) c ^= 1;
      __syncthreads();
    }
    // ---- 3. the rows' quantiles sorted across lanes, the three tail means into qv
    if (on) sort_tails<S>(buf[g][c], qa.M, qa.log2p, qa.k_r, qa.k_c, qv + net * kTile * 3, wv, GW);
    __syncthreads();  // (the next round's first layer overwrites theta)
  }

  // ---- 4. members in ascending order, then one fmaf per sum
  const int e = e0 + tid;
  if (tid >= kTile || e >= a.episodes) return;
  const int nq = a.num_q;
  const float* qt = qv + tid * 3;  // member m, value j: qt[m * kTile * 3 + j]
  float vr = qt[1], vc = qt[nq * kTile * 3 + 2], mr = qt[0], mc = qt[nq * kTile * 3];
  for (int m = 1; m < nq; ++m) {
    const float* r = qt + m * kTile * 3;
    const float* c = qt + (nq + m) * kTile * 3;
    if (a.reduce == OSRL_PLAN_REDUCE_MEAN) {
      vr += r[1];
      vc += c[2];
      mr += r[0];
      mc += c[0];
    } else {  // pessimistic: the lowest return, the highest cost
      vr = fminf(vr, r[1]);
      vc = fmaxf(vc, c[2]);
      mr = fminf(mr, r[0]);
      mc = fmaxf(mc, c[0]);
    }
  }
  if (a.reduce == OSRL_PLAN_REDUCE_MEAN) {
    vr /= (float)nq;
    vc /= (float)nq;
    mr /= (float)nq;
    mc /= (float)nq;
  }
  qa.last_V_mean[(size_t)e * 2] = mr * a.r_mul;
  qa.last_V_mean[(size_t)e * 2 + 1] = mc * a.c_mul;
  close_sums(a, e, vr * a.r_mul, vc * a.c_mul);
}

}  // namespace

extern "C" int osrl_plan_terminal_quantile(const osrl_policy_t* policy, const osrl_gemv_net_t* critics, int32_t num_q,
                                           int32_t M, int32_t k_r, int32_t k_c, int32_t reduce, const float* obs,
                                           int32_t obs_ld, int32_t episodes, float r_mul, float c_mul, float halt_r,
                                           float halt_c, const int32_t* halt_step, float* disc, float* last_V,
                                           float* last_V_mean, void* stream) {
  QTermArgs qa;
  memset(&qa, 0, sizeof qa);
  bool wide = false;
  if (!last_V_mean || M < 2 || M > OSRL_FQE_MAX_QUANTILES || k_r < 1 || k_r > M || k_c < 1 || k_c > M) return -1;
  if (!term_args(policy, critics, num_q, M, reduce, obs, obs_ld, episodes, r_mul, c_mul, halt_r, halt_c, halt_step, disc,
                 last_V, qa.t, &wide))
    return -1;
  qa.last_V_mean = last_V_mean;
  qa.M = M;
  qa.k_r = k_r;
  qa.k_c = k_c;
  qa.log2p = 1;
  while ((1 << qa.log2p) < M) ++qa.log2p;
  const dim3 grid((unsigned)((episodes + kTile - 1) / kTile));
  if (wide)
    return osrl_argmem::launch(plan_terminal_quantile_kernel<OSRL_MAX_WIDTH, kWideIn, 1>, nullptr, grid, dim3(kThreads), 0,
                               (hipStream_t)stream, qa);
  return osrl_argmem::launch(plan_terminal_quantile_kernel<kNarrowW, kNarrowW, 4>, nullptr, grid, dim3(kThreads), 0,
                             (hipStream_t)stream, qa);
}
