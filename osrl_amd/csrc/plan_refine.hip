// plan_refine.hip -- CEM refinement rounds of the act-time planner (engine/mpc.py ModelPlanner(refine_rounds=R)): between
// two H-step runs on the planner's noise table eps[H, E, ad] (the recording step reads it through osrl_collect_t.eps_in;
// episode e = n K + k is candidate k of slot n), ONE entry refits the table per slot from the candidates' scores.
//
//   plan_refit_kernel   one workgroup of 256 threads per slot, K <= 1024 (at most 4 candidates per thread, in registers).
//       (J, C) and the class of every candidate go to LDS; a candidate's rank is the NUMBER of candidates before it under
//       osrl_plan_select's total order (rank by count: integers only, no reduction tree to depend on); order[rank] = k is
//       the elites' index list, in LDS.  Then one thread per column (t, j) of the slot's [H, ad] plan, looping beyond 256:
//       two fp64 passes over the elites in ascending rank (mean, then the squared deviations from it), the momentum mix in
//       fp64 and ONE rounding to fp32 for mu' and for sd'.  No contraction (the pragma below): every fp64 operation rounds
//       once, so a host restatement with the same order gives the same bits.
//   plan_redraw_kernel  a flat grid over the table: work item w = row * G + g, row = t E + e a table row and g one of its
//       G = ceil(ad / 4) groups of four action columns -- one Philox block per item, its four normals the item's four
//       columns.  Items are contiguous in memory in w, so a wave stores one contiguous run of the table.
//       candidate 0: 0 (its sigma is 0: the row is unread);  candidate 1: mu' exactly;  k >= 2: fmaf(sd', z, mu').
//       z = z_in[...] when injected, else word j & 3 of philox4x32_10({episode_base + e, (round << 16) | t, j >> 2,
//       kRefitStream}, key = *seed): a function of (seed word, episode id, round, t, column) alone.  The step and the round
//       share counter word 1, which bounds H <= 65536 and round <= 65535; the entry refuses larger ones.
// Neither kernel reads blockDim / gridDim; both use plain vector stores only -- no atomics, no scratch.  round == 0 is the
// start of a call: the refit kernel reads no score, writes mu = 0, sd = 1 and the identity into elite_rank, and the redraw
// then leaves z for k >= 2 (fmaf(1, z, 0) is z) and 0 for candidate 1.  DESIGN.md "CEM refinement" keeps the budgets.
#include "argmem.h"
#include "rollout_step.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxK = OSRL_PLAN_MAX_CANDIDATES;
constexpr int kThreads = 256, kPerThread = kMaxK / kThreads;
constexpr uint32_t kRefitStream = 18;  // Philox stream of the refinement draws (13 .. 17: exploration .. bootstrap weights)
constexpr int kBatch = 8;  // elites loaded per batch of the column sums
constexpr int kMaxHorizon =1 << 16, kMaxRound = (1 << 16) - 1;

struct RefitArgs {
  const float *disc, *budget;  // [E, 4], [slots]
  const float* eps;            // [H, E, ad]: the table the scores were earned on
  float *mu, *sd;              // [slots, H, ad]
  int32_t* elite_rank;         // [slots, K]
  int32_t candidates, episodes, horizon, ad, n_elite, round;
  float momentum, min_std;
};

// the class of a candidate: 0 feasible, 1 infeasible, 2 a NaN in J or C (after all others, never an elite)
__device__ __forceinline__ int cand_class(float j, float c, float budget) {
  return (j != j || c != c) ? 2 : (c <= budget ? 0 : 1);
}
// whether candidate a comes before candidate b: feasible before infeasible before NaN; among feasible J descending; among
// infeasible C ascending, then J descending; k ascending last (osrl_plan_select's order, continued past its best element)
__device__ __forceinline__ bool before(int cla, float ja, float ca, int ka, int clb, float jb, float cb, int kb) {
  if (cla != clb) return cla < clb;
  if (cla == 2) return ka < kb;
  if (cla == 1 && ca != cb) return ca < cb;
  if (ja != jb) return ja > jb;
  return ka < kb;
}

__global__ __launch_bounds__(kThreads) void plan_refit_kernel(const RefitArgs a) {
  __shared__ float sj[kMaxK], sc[kMaxK];
  __shared__ int32_t order[kMaxK];  // order[rank] = k: the first n_e entries are the elites
  __shared__ uint8_t scl[kMaxK];
  const int tid = threadIdx.x, n = blockIdx.x, K = a.candidates, H = a.horizon, ad = a.ad, cols = H * ad;
  const size_t e0 = (size_t)n * K;
  float* mu = a.mu + (size_t)n * cols;
  float* sd = a.sd + (size_t)n * cols;
  if (a.round == 0) {  // the start of a call: N(0, 1) around the policy, no score is read
    for (int k = tid; k < K; k += kThreads) a.elite_rank[e0 + k] = k;
    for (int c = tid; c < cols; c += kThreads) {
      mu[c] = 0.f;
      sd[c] = 1.f;
    }
    return;
  }
  const float budget = a.budget[n];
  float mj[kPerThread], mc[kPerThread];
  int mcl[kPerThread], rank[kPerThread];
  int n_valid = 0;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {  // (a uniform trip count: the barrier inside is reached by every thread)
    const int k = tid + i * kThreads;
    mj[i] = mc[i] = 0.f;
    mcl[i] = 2;
    rank[i] = 0;
    if (k < K) {
      mj[i] = a.disc[(e0 + k) * 4];
      mc[i] = a.disc[(e0 + k) * 4 + 1];
      mcl[i] = cand_class(mj[i], mc[i], budget);
      sj[k] = mj[i];
      sc[k] = mc[i];
      scl[k] = (uint8_t)mcl[i];
    }
    n_valid += __syncthreads_count(k < K && mcl[i] != 2);
  }
  for (int o = 0; o < K; ++o) {  // every thread reads the same word: an LDS broadcast
    const float oj = sj[o], oc = sc[o];
    const int ocl = scl[o];
#pragma unroll
    for (int i = 0; i < kPerThread; ++i)
      if (i * kThreads < K)  // (uniform: K <= 256 compares one candidate per thread, not four)
        rank[i] += before(ocl, oj, oc, o, mcl[i], mj[i], mc[i], tid + i * kThreads) ? 1 : 0;
  }
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int k = tid + i * kThreads;
    if (k < K) {  // (a total order: the ranks are a permutation of 0 .. K - 1)
      order[rank[i]] = k;
      a.elite_rank[e0 + k] = rank[i];
    }
  }
  __syncthreads();
  const int n_e = a.n_elite < n_valid ? a.n_elite : n_valid;
  if (n_e == 0) return;  // nothing to learn from: mu and sd stay
  const double mom = (double)a.momentum, keep = 1.0 - mom, inv = (double)n_e;
  const size_t E = (size_t)a.episodes;
  for (int c = tid; c < cols; c += kThreads) {
    const int t = c / ad, j = c - t * ad;
    const float* col = a.eps + ((size_t)t * E + e0) * ad + j;  // candidate k's offset: col[k * ad]
    // the elites' offsets come kBatch at a time: the loads of a batch are independent and in flight together, the
    // additions stay one chain in ascending rank (a thread alone walks its column: latency, not bandwidth, is the cost)
    double sum = 0.0, sq = 0.0, m_el = 0.0;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
      for (int r0 = 0; r0 < n_e; r0 += kBatch) {
        float u[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
          const int k = r0 + i < n_e ? order[r0 + i] : 0;
          u[i] = k == 0 ? 0.f : col[(size_t)k * ad];  // (candidate 0 has sigma 0: its offset is 0)
        }
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
          if (r0 + i >= n_e) break;
          if (pass == 0) {
            sum += (double)u[i];
          } else {
            const double d = (double)u[i] - m_el;
            sq += d * d;
          }
        }
      }
      if (pass == 0) m_el = sum / inv;
    }
    const double s_el = sqrt(sq / inv);
    const double m_new = mom * (double)mu[c] + keep * m_el;
    const double s_new = mom * (double)sd[c] + keep * s_el;
    mu[c] = (float)m_new;
    sd[c] = (float)(s_new > (double)a.min_std ? s_new : (double)a.min_std);
  }
}

struct RedrawArgs {
  float* eps;           // [H, E, ad], rewritten
  const float *mu, *sd;  // [slots, H, ad]
  const float* z_in;    // [H, E, ad] or nullptr
  const uint64_t* seed;
  uint32_t episode_base;
  int32_t candidates, episodes, horizon, ad, groups, round;
  int64_t items;  // H * E * groups
};

__global__ __launch_bounds__(kThreads) void plan_redraw_kernel(const RedrawArgs a) {
  const int64_t w = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (w >= a.items) return;
  const int64_t row = w / a.groups;  // t * E + e
  const int g = (int)(w - row * a.groups), ad = a.ad;
  const int t = (int)(row / a.episodes), e = (int)(row - (int64_t)t * a.episodes);
  const int n = e / a.candidates, k = e - n * a.candidates;
  const int j0 = g * 4, nj = ad - j0 < 4 ? ad - j0 : 4;  // this item's columns j0 .. j0 + nj - 1 < ad
  float* out = a.eps + (size_t)row * ad + j0;
  if (k == 0) {
    for (int i = 0; i < nj; ++i) out[i] = 0.f;
    return;
  }
  const size_t plan = ((size_t)n * a.horizon + t) * ad + j0;
  if (k == 1) {  // the refitted mean plan is always evaluated
    for (int i = 0; i < nj; ++i) out[i] = a.mu[plan + i];
    return;
  }
  float z[4];
  if (a.z_in) {
    for (int i = 0; i < 4; ++i) z[i] = i < nj ? a.z_in[(size_t)row * ad + j0 + i] : 0.f;
  } else {
    const uint64_t s = *a.seed;
    const osrl_rng::U4 r = osrl_rng::philox4x32_10(
        osrl_rng::U4{a.episode_base + (uint32_t)e, ((uint32_t)a.round << 16) | (uint32_t)t, (uint32_t)g, kRefitStream},
        (uint32_t)s, (uint32_t)(s >> 32));
    osrl_rng::normal4(r, z);  // z[i] = normal_word(r, i)
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nj) out[i] = fmaf(a.sd[plan + i], z[i], a.mu[plan + i]);
}

}  // namespace

extern "C" int osrl_plan_refit(const float* disc, const float* budget, float* eps, float* mu, float* sd, int32_t slots,
                               int32_t candidates, int32_t horizon, int32_t action_dim, int32_t n_elite, float momentum,
                               float min_std, int32_t round, const uint64_t* seed, uint32_t episode_base,
                               const float* z_in, int32_t* elite_rank, void* stream) {
  if (!disc || !budget || !eps || !mu || !sd || !elite_rank || (!seed && !z_in) || slots < 1 || candidates < 1 ||
      candidates > OSRL_PLAN_MAX_CANDIDATES || horizon < 1 || horizon > kMaxHorizon || action_dim < 1 || n_elite < 1 ||
      round < 0 || round > kMaxRound || !(momentum >= 0.f && momentum < 1.f) || !(min_std >= 0.f && min_std < INFINITY))
    return -1;
  const int64_t episodes = (int64_t)slots * candidates, groups = (action_dim + 3) / 4;
  const int64_t items = (int64_t)horizon * episodes * groups;
  if (episodes > INT32_MAX || (int64_t)horizon * action_dim > INT32_MAX || (int64_t)horizon * episodes * action_dim > INT32_MAX)
    return -1;
  const RefitArgs ra{disc, budget, eps, mu, sd, elite_rank, candidates, (int32_t)episodes, horizon, action_dim, n_elite,
                     round, momentum, min_std};
  const int rc = osrl_argmem::launch(plan_refit_kernel, nullptr, dim3((unsigned)slots), dim3(kThreads), 0,
                                     (hipStream_t)stream, ra);
  if (rc != 0) return rc;
  const RedrawArgs da{eps, mu, sd, z_in, seed, episode_base, candidates, (int32_t)episodes, horizon, action_dim,
                      (int32_t)groups, round, items};
  return osrl_argmem::launch(plan_redraw_kernel, nullptr, dim3((unsigned)((items + kThreads - 1) / kThreads)),
                             dim3(kThreads), 0, (hipStream_t)stream, da);
}
