// cdt_act.hip -- the act latency path of the Constrained Decision Transformer's episode loop on gfx950: one episode
// per handle (B = 1), or N episodes advanced by the same launches, in lockstep or each slot at its own timestep.
//
// CDTTrainer.rollout (cdt.py:436-518) asks the model for one action per env step over a sliding window of the last
// seq_len timesteps.  Run as a training-shaped forward that is ~30 launches over a window padded to seq_len plus a
// host round trip per step.  A policy handle here keeps the window ON THE DEVICE together with every token's hidden
// state, and per env step runs only the work that changed ("B = 1 act()"):
//   * growth (t < seq_len): attention is causal, so no earlier token changes at any layer: only the previous
//     step's action token (a zero dummy until now) and the new [return] [cost] state tokens go through the layers;
//   * sliding (t >= seq_len): the blocks are pre-norm, so a token's layer-0 q / k / v depend on its own embedding
//     (value + absolute timestep) alone and stay cached; layer-0 attention onward is recomputed for the window
//     (every token lost the dropped keys), and the last layer runs past its q / k / v for the newest state token
//     only;
//   * the cost-prefix token attends to itself alone: its hidden states are computed once at reset.
// One env step = one ingest/embed launch, five launches per layer (LN1+QKV, attention, out-proj+residual,
// LN2+MLP-up+GELU, MLP-down+residual) and one head launch, which writes the action into pinned, device-mapped memory
// and publishes a sequence number (system-scope release) the host spins on, as act.hip does.  No launch waits on
// another workgroup.  The projections are fp32 MFMA (v_mfma_f32_16x16x4f32) over 16-row tiles of the packed forward
// weights PF[k/4][n][k%4] (the copies the fused AdamW step and repack() keep current), split-K over the four waves
// of a workgroup and summed in LDS in a fixed order: results do not depend on scheduling.
// A handle of N episodes (osrl_cdt_policy_create_n) keeps N such windows, one per-episode block of `es` floats each in
// the handle's device allocation.  A step is the SAME 2 + 5 * layers launches: ingest and head run one workgroup per
// episode, attention one wave per (row, head, episode), and a projection's row list is the concatenation over the
// episodes, so that its 16-row tiles fill up with rows of several episodes.  No arithmetic crosses rows: an episode's
// results do not depend on N, on its slot or on what the other slots are doing.
// While the episodes share the timestep (lockstep: _reset_n / _step_n on slots that all stand at the same t) they share
// the phase and every row set, and the launches take one (first, count, ring) per stage from their arguments.  When they
// do not (osrl_cdt_policy_step_slots: a slot restarts or idles while the others step) every episode contributes the rows
// of ITS phase -- restart: R - 1 rows + the prefix row; growth: the previous action token + the new tokens; sliding:
// layer-0 q / k / v of the new rows, the whole window from there on; idle: nothing -- and the launches take them from a
// per-call TABLE the host derives (it knows every slot's timestep): per episode its mode, timestep, window start and
// newest state row, and per row-set class (new rows / rows past layer-0 q k v / newest state token) the episode's
// (first, count, ring) and the exclusive prefix sum of the counts.  The host writes the table into a segment of the
// pinned block, the ingest launch copies each episode's entries to device memory, the later launches read that copy;
// a call returns only after publication, so the host never rewrites the table under a running chain.  A projection maps
// entry g of its row list to (episode, local row) by one ballot + popcount over the prefix sums; attention's grid x is
// the largest count and workgroups past their episode's count exit at once.  Grids are sized by the totals: an idle
// slot costs no rows.
// The head launch can end in the recording collectors' exploration tail (osrl_cdt_policy_step_slots_explore): a = clip(mu
// + s * eps) with rollout_step.h's arithmetic and noise keys, s a per-slot sigma or exp(log_std) of the head row; the
// action taken is what the window records at the next step.  The calls without it read none of its arguments.
#include <math.h>

#include <new>
#include <vector>

#include "dev_util.h"
#include "gelu.h"
#include "policy_common.h"
#include "rollout_step.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kMaxE = 512, kMaxD = 128, kMaxTok = 256, kMaxHead = 1024;
constexpr float kLnEps = 1e-5f;

// the per-call table of a call whose episodes are at different timesteps: int32 [kTabFields][kTabStride], entry
// [field][episode].  Row-set class c (0: the rows whose embedding is new; 1: the rows through the layers past layer-0
// q / k / v; 2: the newest state token) has its first / count / ring / exclusive count prefix at kTabSet + 4 c ...
constexpr int kTabStride = OSRL_CDT_POLICY_MAX_ENVS;
constexpr int kTabMode = 0, kTabT = 1, kTabWs = 2, kTabSrow = 3, kTabSet = 4, kTabFields = 16;
constexpr int kIdle = 0, kStep = 1, kRestart = 2;


// mean / rstd of one row of E <= 512 floats, by one wave (two passes, as the training LayerNorm)
__device__ __forceinline__ void row_stats(const float* __restrict__ x, int E, int lane, float* mean_o, float* rstd_o) {
  float v[kMaxE / 64];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxE / 64; ++j) {
    const int f = lane + 64 * j;
    v[j] = f < E ? x[f] : 0.f;
    s += v[j];
  }
  const float mean = wave_sum(s) / (float)E;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxE / 64; ++j)
    if (lane + 64 * j < E) q += (v[j] - mean) * (v[j] - mean);
  *mean_o = mean;
  *rstd_o = 1.0f / sqrtf(wave_sum(q) / (float)E + kLnEps);
}

// ring row of entry i of a row set: (first + i) mod ring
__device__ __forceinline__ int ring_row(int first, int i, int ring) {
  const int r = first + i;
  return r < ring ? r : r - ring;
}

struct Dev {  // device view of a handle's buffers
  float *win_s, *win_a, *win_r, *win_c;  // ring [T, od] / [T, ad] / [T] / [T]: slot = timestep mod T
  int32_t* win_t;                        // [T] absolute timestep
  float* last_act;                       // [ad] the action the head returned last
  float* raw;                            // [NR, ldE] pre-LayerNorm embeddings (cost features read the cost token's)
};

// episode e's view: every per-episode buffer sits at the same offset of its episode's block of `es` floats
__device__ __forceinline__ Dev dev_at(const Dev& d, size_t off) {
  return Dev{d.win_s + off, d.win_a + off, d.win_r + off, d.win_c + off, d.win_t + off, d.last_act + off, d.raw + off};
}

struct Io {  // pinned + device-mapped; one row per episode
  float *obs, *act_in, *act_out, *scalars;  // scalars: reward, cost, target_return, target_cost
  uint64_t* seq;
};

// ---------------------------------------------------------------------------------------------------------------
// ingest + embedding: update the device window from the I/O block, then embed + LayerNorm the listed token rows.
struct IngestArgs {
  osrl_cdt_policy_t p;
  Dev d;
  Io io;
  float* x0;  // [NR, ldE] emb LayerNorm output
  int32_t ldE, R, TR, t, reset, host_action;
  int32_t first, count, ring;  // token rows to embed
  int64_t es;                  // floats per episode block (grid: one workgroup per episode)
  const int32_t* htab;         // the call's table in the pinned block, or null: t / reset / rows above serve every episode
  int32_t* dtab;               // its device copy, for the later launches
};

__global__ __launch_bounds__(256) void cdt_act_ingest_kernel(const IngestArgs a) {
  const osrl_cdt_policy_t& p = a.p;
  const int tid = threadIdx.x, T = p.seq_len, od = p.state_dim, ad = p.action_dim;
  int t = a.t, reset = a.reset, first = a.first, count = a.count, ring = a.ring;
  if (a.htab) {  // this episode's own timestep, mode and rows
    const int32_t* __restrict__ ht = a.htab + blockIdx.x;
    if (tid < kTabFields) a.dtab[tid * kTabStride + blockIdx.x] = ht[tid * kTabStride];
    const int mode = ht[kTabMode * kTabStride];
    if (mode == kIdle) return;
    t = ht[kTabT * kTabStride];
    reset = mode == kRestart;
    first = ht[kTabSet * kTabStride];
    count = ht[(kTabSet + 1) * kTabStride];
    ring = ht[(kTabSet + 2) * kTabStride];
  }
  const int cur = t % T;
  const size_t eoff = (size_t)blockIdx.x * (size_t)a.es;
  const Dev d = dev_at(a.d, eoff);
  const Io io{a.io.obs + (size_t)blockIdx.x * od, a.io.act_in + (size_t)blockIdx.x * ad, nullptr,
              a.io.scalars + (size_t)blockIdx.x * 4, nullptr};
  float* __restrict__ x0 = a.x0 + eoff;
  if (reset) {
    for (int i = tid; i < od; i += blockDim.x) d.win_s[i] = io.obs[i];
    if (tid == 0) {
      d.win_r[0] = io.scalars[2];
      d.win_c[0] = io.scalars[3];
      d.win_t[0] = 0;
    }
  } else {
    const int prv = (t - 1) % T;
    for (int i = tid; i < ad && T > 1; i += blockDim.x)  // (seq_len 1: the previous timestep left the window)
      d.win_a[prv * ad + i] = a.host_action ? io.act_in[i] : d.last_act[i];
    for (int i = tid; i < od; i += blockDim.x) d.win_s[cur * od + i] = io.obs[i];
    if (tid == 0) {  // returns[t+1] = returns[t] - float(reward); costs[t+1] = costs[t] - cost  (fp32, cdt.py:506-507)
      d.win_r[cur] = d.win_r[prv] - io.scalars[0];
      d.win_c[cur] = d.win_c[prv] - io.scalars[1];
      d.win_t[cur] = t;
    }
  }
  for (int i = tid; i < ad; i += blockDim.x) d.win_a[cur * ad + i] = 0.f;  // the newest action slot: zero dummy
  __syncthreads();
  const int lane = tid & 63, E = p.embedding_dim;
  for (int i = tid >> 6; i < count; i += blockDim.x >> 6) {
    const int row = ring_row(first, i, ring);
    const bool is_prefix = row == a.TR;
    const int ts = is_prefix ? 0 : row / a.R, slot = is_prefix ? 0 : row - ts * a.R;
    int which = slot + (4 - a.R);  // 0 return, 1 cost, 2 state, 3 action (cdt.py:185-200)
    if (a.R == 3 && p.use_rew) which = slot == 0 ? 0 : slot + 1;
    const float* te = (p.te && !is_prefix) ? p.te + (size_t)d.win_t[ts] * E : nullptr;
    const float ret = d.win_r[ts];
    const float ctg = p.cost_transform ? 50.0f - d.win_c[ts] : d.win_c[ts];
    const float ec = io.scalars[3];
    float v[kMaxE / 64];
#pragma unroll
    for (int j = 0; j < kMaxE / 64; ++j) {
      const int f = lane + 64 * j;
      float x = 0.f;
      if (f < E) {
        if (is_prefix) {
          x = ec * p.prefix_w[f] + p.prefix_b[f];
        } else if (which == 0) {
          x = ret * p.return_w[f] + p.return_b[f];
        } else if (which == 1) {
          x = ctg * p.cost_w[f] + p.cost_b[f];
        } else if (which == 2) {
          x = p.state_b[f];
#pragma unroll 4
          for (int k = 0; k < od; ++k) x += d.win_s[ts * od + k] * p.state_w[(size_t)f * od + k];
        } else {
          x = p.action_b[f];
          for (int k = 0; k < ad; ++k) x += d.win_a[ts * ad + k] * p.action_w[(size_t)f * ad + k];
        }
        if (te) x += te[f];
        d.raw[(size_t)row * a.ldE + f] = x;
      }
      v[j] = x;
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxE / 64; ++j) s += v[j];
    const float mean = wave_sum(s) / (float)E;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxE / 64; ++j)
      if (lane + 64 * j < E) q += (v[j] - mean) * (v[j] - mean);
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)E + kLnEps);
#pragma unroll
    for (int j = 0; j < kMaxE / 64; ++j) {
      const int f = lane + 64 * j;
      if (f < E) x0[(size_t)row * a.ldE + f] = (v[j] - mean) * rstd * p.emb_g[f] + p.emb_b[f];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Y[r] = epi(LN?(X[r]) W^T + b) for the rows of a row set: one workgroup = one 16-row x 16-column tile, four waves
// split K and meet in LDS.  epi: optional exact GELU, then an optional residual add.  With nenv episodes the launch's
// row list is the row set of episode 0, then of episode 1, ...: entry g is local row g % count of episode g / count;
// with a table (tab: the class's first / count / ring / prefix entries) the episodes' counts differ and entry g belongs
// to the last episode whose prefix is <= g.
struct LinArgs {
  const float* X;
  const float *ln_g, *ln_b;  // LayerNorm of the input rows (K = E) or null
  const float* W;            // packed PF[k/4][n][k%4], Np = round16(N) columns
  const float* bias;
  const float* res;  // residual rows (same row index) or null
  float* Y;
  int32_t ldx, ldr, ldy, K, N, gelu;
  int32_t first, count, ring;
  int32_t nenv;
  int64_t es;    // floats per episode block (X, res and Y are episode 0's)
  uint64_t rcp;  // ceil(2^32 / count): g / count = (g * rcp) >> 32, exact for g < 2^16 and count <= 2^8
  const int32_t* tab;  // or null.  With a table `count` is the total over the episodes; first / ring / rcp are unused
};

__global__ __launch_bounds__(256) void cdt_act_linear_kernel(const LinArgs a) {
  __shared__ float red[4][64][4];
  __shared__ float st[16][2];
  __shared__ int rows[16];
  __shared__ long long xo[16], ro[16], yo[16];  // float offsets of the tile's rows in X, res and Y
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r0 = blockIdx.y * 16, n0 = blockIdx.x * 16;
  if (a.tab) {
    if (tid < 64) {  // wave 0: lane e holds episode e's prefix, lane i < 16 resolves tile row i
      const int pv = tid < a.nenv ? a.tab[3 * kTabStride + tid] : 0x7fffffff;
      int e = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const unsigned long long m = __ballot(pv <= r0 + i);  // (prefix[0] = 0: never empty)
        if (tid == i) e = __popcll(m) - 1;
      }
      const int pe = __shfl(pv, e);
      if (tid < 16) {
        const int g = r0 + tid;
        int r = -1;
        long long eo = 0;
        if (g < a.count) {
          r = ring_row(a.tab[e], g - pe, a.tab[2 * kTabStride + e]);
          eo = (long long)e * a.es;
        }
        rows[tid] = r;
        xo[tid] = eo + (long long)r * a.ldx;
        ro[tid] = eo + (long long)r * a.ldr;
        yo[tid] = eo + (long long)r * a.ldy;
      }
    }
  } else if (tid < 16) {
    const int g = r0 + tid;
    int r = -1;
    long long eo = 0;
    if (g < a.count * a.nenv) {
      const int e = (int)(((uint64_t)(uint32_t)g * a.rcp) >> 32);
      r = ring_row(a.first, g - e * a.count, a.ring);
      eo = (long long)e * a.es;
    }
    rows[tid] = r;
    xo[tid] = eo + (long long)r * a.ldx;
    ro[tid] = eo + (long long)r * a.ldr;
    yo[tid] = eo + (long long)r * a.ldy;
  }
  __syncthreads();
  if (a.ln_g) {
    for (int i = w; i < 16; i += 4) {
      float mean = 0.f, rstd = 0.f;
      if (rows[i] >= 0) row_stats(a.X + xo[i], a.K, lane, &mean, &rstd);
      if (lane == 0) {
        st[i][0] = mean;
        st[i][1] = rstd;
      }
    }
    __syncthreads();
  }
  const int ar = lane & 15, kq = lane >> 4;
  const int row = rows[ar];
  const float* __restrict__ xr = row >= 0 ? a.X + xo[ar] : nullptr;
  const float mean = a.ln_g ? st[ar][0] : 0.f, rstd = a.ln_g ? st[ar][1] : 1.f;
  const int Np = round16(a.N), nkb = round16(a.K) >> 4;
  const int kb0 = (nkb * w) >> 2, kb1 = (nkb * (w + 1)) >> 2;
  const f32x4* __restrict__ W4 = reinterpret_cast<const f32x4*>(a.W);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // kC k-blocks per round: every load of the round is issued before the first MFMA (the loop is latency-bound:
  // a few k-blocks per wave at these row counts).  Rows' padding columns are zero (never written, zeroed at create).
  constexpr int kC = 8;
  for (int kc = kb0; kc < kb1; kc += kC) {
    f32x4 bv[kC], av[kC], gv[kC], be[kC];
#pragma unroll
    for (int u = 0; u < kC; ++u) {
      const int kb = kc + u, k0 = 16 * kb + 4 * kq;
      bv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      av[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      gv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      be[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (kb < kb1) {
        bv[u] = W4[(size_t)(4 * kb + kq) * Np + n0 + ar];
        if (xr) av[u] = *reinterpret_cast<const f32x4*>(xr + k0);
        if (a.ln_g) {
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (k0 + t < a.K) {
              gv[u][t] = a.ln_g[k0 + t];
              be[u][t] = a.ln_b[k0 + t];
            }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kC; ++u) {
      if (a.ln_g && xr) {
#pragma unroll
        for (int t = 0; t < 4; ++t) av[u][t] = (av[u][t] - mean) * rstd * gv[u][t] + be[u][t];  // (0 past K: g = b = 0)
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][t], bv[u][t], acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[w][lane][i] = acc[i];
  __syncthreads();
  if (w == 0) {
    const int col = n0 + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = (lane >> 4) * 4 + i;
      const int orow = rows[rr];
      if (orow < 0 || col >= a.N) continue;
      float v = ((red[0][lane][i] + red[1][lane][i]) + red[2][lane][i]) + red[3][lane][i];
      v += a.bias[col];
      if (a.gelu) v = gelu_f(v);
      if (a.res) v += a.res[ro[rr] + col];
      a.Y[yo[rr] + col] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// causal softmax attention of the listed query rows over the window (+ the prefix token): one wave per (row, head,
// episode); keys and values are the query's own episode's.
struct AttnArgs {
  const float* qkv;  // [NR, ldq]: q | k | v
  float* o;          // [NR, ldo]
  const int32_t* tab;  // the call's table or null.  With a table `first` is the row-set class; ring and ws are unused
  int32_t ldq, E, d, P, TR, ws;  // ws: ring row of the window's first token.  (o's row stride is round16(E))
  float scale;
  int32_t first, ring;  // query rows: grid x entries from `first` (mod ring)
  int32_t es;           // floats per episode block (grid z: episode).  (The struct stays within the 16 dwords a
                        // launch hands over in registers.)
};

__global__ __launch_bounds__(64) void cdt_act_attn_kernel(const AttnArgs a) {
  __shared__ float pr[kMaxTok];
  const int lane = threadIdx.x, h = blockIdx.y, ldo = round16(a.E);
  int first = a.first, ring = a.ring, ws = a.ws;
  if (a.tab) {  // the query's episode's rows and window start; grid x covers the largest count
    const int32_t* __restrict__ st = a.tab + (kTabSet + 4 * a.first) * kTabStride + blockIdx.z;
    if ((int)blockIdx.x >= st[kTabStride]) return;
    first = st[0];
    ring = st[2 * kTabStride];
    ws = a.tab[kTabWs * kTabStride + blockIdx.z];
  }
  const int row = ring_row(first, blockIdx.x, ring);
  // keys: the prefix (ring row TR) first, then the window's tokens up to and including the query
  const int nk = row == a.TR ? 1 : a.P + (row - ws + a.TR) % a.TR + 1;
  const float* __restrict__ qkv = a.qkv + (size_t)blockIdx.z * (size_t)a.es;
  float* __restrict__ o = a.o + (size_t)blockIdx.z * (size_t)a.es;
  const float* __restrict__ q = qkv + (size_t)row * a.ldq + h * a.d;
  float s[kMaxTok / 64];
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < kMaxTok / 64; ++c) {
    const int j = lane + 64 * c;
    s[c] = -INFINITY;
    if (j < nk) {
      const int kr = j < a.P ? a.TR : (ws + j - a.P) % a.TR;
      const float* __restrict__ k = qkv + (size_t)kr * a.ldq + a.E + h * a.d;
      float acc = 0.f;
#pragma unroll 8
      for (int i = 0; i < a.d; ++i) acc = fmaf(q[i], k[i], acc);
      s[c] = acc * a.scale;
      mx = fmaxf(mx, s[c]);
    }
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < kMaxTok / 64; ++c) {
    const int j = lane + 64 * c;
    if (j < nk) {
      const float e = expf(s[c] - mx);
      pr[j] = e;
      sum += e;
    }
  }
  const float inv = 1.0f / wave_sum(sum);
  __syncthreads();
  for (int i = lane; i < a.d; i += 64) {
    float acc = 0.f;
#pragma unroll 4
    for (int j = 0; j < nk; ++j) {
      const int kr = j < a.P ? a.TR : (ws + j - a.P) % a.TR;
      acc = fmaf(pr[j], qkv[(size_t)kr * a.ldq + 2 * a.E + h * a.d + i], acc);
    }
    o[(size_t)row * ldo + h * a.d + i] = acc * inv;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// head: out LayerNorm of the newest state token, cost features, the action head's Linear (+ GELU) layers as GEMVs
// (lanes own outputs over the packed weights, as act.hip), clamp, publish.  One workgroup per episode; the sequence
// number is published once, by the last workgroup to arrive at the handle's device counter: every workgroup makes its
// act_out stores visible at system scope and then increments the counter; the one that sees nenv - 1 re-arms it and
// does the release store.  Nobody waits for anybody.  With a table an idle episode's workgroup writes no action and
// only arrives, so the sequence number is still published once.
struct HeadArgs {
  osrl_cdt_policy_t p;
  Dev d;
  Io io;
  const float* x;  // [NR, ldE] the last block's output
  int32_t ldE, srow, crow;  // newest state token row, its cost token row (-1: none)
  uint64_t seq;
  int64_t es;         // floats per episode block (grid: one workgroup per episode)
  uint32_t* arrived;  // device counter of the workgroups that have stored their action (0 between launches)
  int32_t nenv;
  const int32_t* tab;  // the call's table or null.  With a table srow is the episode's own and crow < 0 means "none"
  // the exploration tail (osrl_cdt_policy_step_slots_explore; explore = 0: none of this is read): a = clip(mu + s * eps),
  // rollout_step.h's arithmetic and noise keys (cdt_collect.hip's).  s = sigma[episode], or with `sample` exp(log_std) of
  // the head row
  const float* sigma;         // [nenv] (pinned)
  const float* eps;           // [nenv, action_dim] injected noise (pinned), read when host_eps
  const int32_t* episode_id;  // [nenv] (pinned) the episode word of the noise key; the step word is the timestep
  float* head_out;            // [nenv, 2 * action_dim] (pinned) the head row (mu | log_std), written when sampling
  int32_t explore, sample, host_eps, t;  // t: every episode's timestep when there is no table
  uint32_t x0, x1;                       // the exploration seed
};

__device__ __forceinline__ void head_arrive(const HeadArgs& a) {  // by one thread, after the workgroup's stores
  __threadfence_system();
  bool last = a.nenv == 1;
  if (!last) {
    last = __hip_atomic_fetch_add(a.arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)(a.nenv - 1);
    if (last) {
      __hip_atomic_store(a.arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence_system();
    }
  }
  if (last) __hip_atomic_store(a.io.seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

constexpr int kHeadThreads = 1024;

__global__ __launch_bounds__(kHeadThreads) void cdt_act_head_kernel(const HeadArgs a) {
  __shared__ __attribute__((aligned(16))) float buf[2][kMaxHead];
  __shared__ float red[kHeadThreads];
  __shared__ float st[2];
  __shared__ float lstd[kMaxHead / 2];  // the head row's log_std columns (a sampling call's second pass)
  const osrl_cdt_policy_t& p = a.p;
  const int tid = threadIdx.x, E = p.embedding_dim;
  const size_t eoff = (size_t)blockIdx.x * (size_t)a.es;
  const float* __restrict__ x = a.x + eoff;
  const float* __restrict__ raw = a.d.raw + eoff;
  int srow = a.srow, crow = a.crow;
  if (a.tab) {
    if (a.tab[kTabMode * kTabStride + blockIdx.x] == kIdle) {
      if (tid == 0) head_arrive(a);
      return;
    }
    srow = a.tab[kTabSrow * kTabStride + blockIdx.x];
    crow = a.crow >= 0 ? srow - 1 : -1;  // the cost token precedes the state token (the cost features imply use_cost)
  }
  if (tid < 64) {
    float mean, rstd;
    row_stats(x + (size_t)srow * a.ldE, E, tid, &mean, &rstd);
    if (tid == 0) {
      st[0] = mean;
      st[1] = rstd;
    }
  }
  __syncthreads();
  const int Eh = p.cat_cost_feat ? 2 * E : E;
  for (int f = tid; f < kMaxHead; f += kHeadThreads) {
    float v = 0.f;
    if (f < E) {
      v = (x[(size_t)srow * a.ldE + f] - st[0]) * st[1] * p.out_g[f] + p.out_b[f];
      if (crow >= 0) {  // cdt.py:243-250, the detached (pre-LayerNorm) cost embedding
        const float ce = raw[(size_t)crow * a.ldE + f];
        if (p.add_cost_feat) {
          v = v + ce;
          if (p.mul_cost_feat) v = v * ce;
        } else if (p.mul_cost_feat) {
          v = v * ce;
        }
      }
    } else if (f < Eh) {
      v = raw[(size_t)crow * a.ldE + (f - E)];
    }
    buf[0][f] = v;
  }
  __syncthreads();
  int cur = 0, in = Eh;
  const int nl = p.head_layers;
  for (int l = 0; l < nl; ++l) {
    const bool last = l == nl - 1;
    const int out = last ? p.action_dim : Eh;
    const int Np = last ? round16(p.head_out_width) : round16(Eh);
    const int nq = round16(in) >> 2;
    const f32x4* __restrict__ W4 = reinterpret_cast<const f32x4*>(p.head_w[l]);
    // 1024 threads = KS k-splits x NL neuron lanes
    int NL = 16;
    while (NL < round16(out) && NL < 256) NL <<= 1;
    const int KS = kHeadThreads / NL, ks = tid / NL, nl_ = tid - ks * NL;
    const int q0 = (nq * ks) / KS, q1 = (nq * (ks + 1)) / KS;
    float* nxt = buf[cur ^ 1];
    // A sampling call runs the last layer twice: pass 0 is the evaluating call's (the mean keeps its bits), pass 1 the
    // log_std columns action_dim .. 2 * action_dim - 1 with the SAME k-split, into lstd.  (One pass over 2 * action_dim
    // columns would derive NL / KS from another width and sum the mean in another order.)
    const int npass = last && a.explore && a.sample ? 2 : 1;
    for (int pass = 0; pass < npass; ++pass) {
      const int c0 = pass * out;  // first weight row / bias of the pass
      const int live = pass ? out : round16(out);  // (pass 1 reads no column past the ones it keeps: c0 + n < Np)
      float acc[4] = {0.f, 0.f, 0.f, 0.f};  // neurons nl_ + 256 j (out <= 1024)
      for (int q = q0; q < q1; ++q) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(&buf[cur][4 * q]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n = nl_ + 256 * j;
          if (n < NL * (j + 1) && n < live) {
            const f32x4 wv = W4[(size_t)q * Np + c0 + n];
            acc[j] = fmaf(wv[0], xv[0], fmaf(wv[1], xv[1], fmaf(wv[2], xv[2], fmaf(wv[3], xv[3], acc[j]))));
          }
        }
      }
      // partials [KS][NL] per 256-neuron chunk, summed in k-split order
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (256 * j >= round16(out)) break;
        __syncthreads();
        red[tid] = acc[j];
        __syncthreads();
        for (int n = 256 * j + tid; n < 256 * (j + 1) && n < round16(out) && tid < NL; n += kHeadThreads) {
          float s = 0.f;
          for (int k = 0; k < KS; ++k) s += red[k * NL + (n - 256 * j)];
          float v = 0.f;
          if (n < out) {
            v = s + p.head_b[l][c0 + n];
            if (!last) v = gelu_f(v);
          }
          if (pass == 0)
            nxt[n] = v;
          else if (n < out)
            lstd[n] = v;
        }
      }
    }
    __syncthreads();
    for (int f = round16(out) + tid; f < kMaxHead; f += kHeadThreads) nxt[f] = 0.f;  // the next layer's k padding
    __syncthreads();
    cur ^= 1;
    in = out;
  }
  if (tid < p.action_dim) {
    const int ad = p.action_dim;
    float v = buf[cur][tid];
    if (a.explore) {
      float sg;
      if (a.sample) {  // the head row goes out as it is: behaviour log-probabilities are the caller's
        const float ls = lstd[tid];
        a.head_out[(size_t)blockIdx.x * 2 * ad + tid] = v;
        a.head_out[(size_t)blockIdx.x * 2 * ad + ad + tid] = ls;
        sg = expf(ls);  // no log-std bounds, as osrl_cdt_collect
      } else {
        sg = a.sigma[blockIdx.x];
      }
      v = osrl_rollout::explore(v, sg, [&] {  // (s == 0: clip(mu) exactly)
        const int t = a.tab ? a.tab[kTabT * kTabStride + blockIdx.x] : a.t;
        return osrl_rollout::explore_eps((uint32_t)a.episode_id[blockIdx.x], (uint32_t)t, tid, a.x0, a.x1,
                                         a.host_eps ? a.eps : nullptr, (size_t)blockIdx.x * ad + tid);
      });
    }
    v = fminf(fmaxf(v, -p.max_action), p.max_action);
    a.io.act_out[(size_t)blockIdx.x * ad + tid] = v;
    a.d.last_act[eoff + tid] = v;  // the action taken: the next ingest records it in the window
  }
  __syncthreads();
  if (tid == 0) head_arrive(a);
}

// ---------------------------------------------------------------------------------------------------------------
struct Handle {
  osrl_cdt_policy_t p;
  std::vector<osrl_cdt_layer_t> layers;
  int R, P, TR, NR, ldE, ld3, ld4;
  int nenv;            // episodes per call
  int64_t es;          // floats per episode block of dmem
  std::vector<int> t;  // [nenv] timestep of each episode's newest window entry; -1 before its first (re)start
  PinnedBlock blk;
  Io host, dev;
  struct Xio {  // the exploration tail's segments of the pinned block
    float *sigma, *eps;
    int32_t* episode_id;
    float* head;
  } xhost, xdev;
  int32_t *htab, *htab_dev;  // the per-call table in the pinned block (host / device address) ...
  int32_t* dtab;             // ... and the copy the ingest launch makes of it in device memory
  Dev d;
  void* dmem;
  float *x, *qkv, *o, *xmid, *h;  // episode 0's; x: [NL + 1][NR, ldE], qkv: [NL][NR, ld3]
  uint32_t* arrived;              // the head workgroups' arrival counter (past the episode blocks)
  uint64_t seq;
};

struct Rows {
  int first, count, ring;
};

// what an episode at timestep t runs: the row-set classes of the table (kTabSet), the window start and the newest
// state token's row
struct Plan {
  Rows set[3];
  int ws, srow;
};

Plan plan_of(const Handle* h, int t, bool restart) {
  const int T = h->p.seq_len, R = h->R, TR = h->TR;
  const int cur = (t % T) * R;
  Plan pl;
  // rows whose embedding (and, in growth, every layer) is new: the previous action token + this step's tokens
  if (t == 0) {
    const int pre = h->P && restart ? 1 : 0;  // the prefix row joins the embedded rows
    pl.set[0] = Rows{pre ? TR : 0, R - 1 + pre, TR + 1};
  } else {
    pl.set[0] = Rows{(cur - 1 + TR) % TR, R, TR};
  }
  const int n = t + 1 < T ? t + 1 : T;  // timesteps in the window
  pl.ws = ((t + 1 - n) % T) * R;        // ring row of its first token
  pl.srow = cur + R - 2;                // the newest state token
  // sliding: layer-0 attention onward (and q / k / v past layer 0) run over the window's tokens, without the newest
  // (dummy) action token
  pl.set[1] = t >= T ? Rows{pl.ws, n * R - 1, TR} : pl.set[0];
  pl.set[2] = Rows{pl.srow, 1, TR};
  return pl;
}

// one call's launches: either one plan for every episode (lockstep), or the table (tot / mx: the classes' total and
// largest counts over the episodes)
struct Call {
  bool table;
  Plan pl;
  int t, reset;
  int tot[3], mx[3];
};

int launch_linear(const Handle* h, const Call& c, int cls, const float* X, int ldx, const float* g, const float* b,
                  const float* W, const float* bias, const float* res, int ldr, float* Y, int ldy, int K, int N,
                  int gelu, hipStream_t s) {
  if (c.table) {
    const int total = c.tot[cls];
    if (total <= 0) return 0;
    LinArgs a{X, g, b, W, bias, res, Y, ldx, ldr, ldy, K, N, gelu, 0, total, 1, h->nenv, h->es, 0,
              h->dtab + (kTabSet + 4 * cls) * kTabStride};
    hipLaunchKernelGGL(cdt_act_linear_kernel, dim3((N + 15) / 16, (total + 15) / 16), dim3(256), 0, s, a);
    return 0;
  }
  const Rows& r = c.pl.set[cls];
  if (r.count <= 0) return 0;
  LinArgs a{X, g, b, W, bias, res, Y, ldx, ldr, ldy, K, N, gelu, r.first, r.count, r.ring, h->nenv, h->es,
            (((uint64_t)1 << 32) + (uint64_t)r.count - 1) / (uint64_t)r.count, nullptr};
  hipLaunchKernelGGL(cdt_act_linear_kernel, dim3((N + 15) / 16, (r.count * h->nenv + 15) / 16), dim3(256), 0, s, a);
  return 0;
}

// one block: the rows of class `qc` through LN1 + q / k / v, the rows of class `oc` through attention .. MLP
void run_layer(const Handle* h, const Call& c, int l, int qc, int oc, hipStream_t s) {
  const osrl_cdt_policy_t& p = h->p;
  const osrl_cdt_layer_t& L = h->layers[l];
  const int E = p.embedding_dim;
  const size_t xs = (size_t)h->NR * h->ldE;
  const float* xin = h->x + l * xs;
  float* xout = h->x + (l + 1) * xs;
  float* qkv = h->qkv + (size_t)l * h->NR * h->ld3;
  launch_linear(h, c, qc, xin, h->ldE, L.ln1_g, L.ln1_b, L.w_qkv, L.b_qkv, nullptr, 0, qkv, h->ld3, E, 3 * E, 0, s);
  const Rows& r = c.pl.set[oc];
  const int gx = c.table ? c.mx[oc] : r.count;
  if (gx <= 0) return;
  const int d = E / p.num_heads;
  AttnArgs at{qkv, h->o, c.table ? h->dtab : nullptr, h->ld3, E, d, h->P, h->TR, c.table ? 0 : c.pl.ws,
              1.0f / sqrtf((float)d), c.table ? oc : r.first, c.table ? 1 : r.ring, (int32_t)h->es};
  hipLaunchKernelGGL(cdt_act_attn_kernel, dim3(gx, p.num_heads, h->nenv), dim3(64), 0, s, at);
  launch_linear(h, c, oc, h->o, h->ldE, nullptr, nullptr, L.w_o, L.b_o, xin, h->ldE, h->xmid, h->ldE, E, E, 0, s);
  launch_linear(h, c, oc, h->xmid, h->ldE, L.ln2_g, L.ln2_b, L.w_1, L.b_1, nullptr, 0, h->h, h->ld4, E, 4 * E, 1, s);
  launch_linear(h, c, oc, h->h, h->ld4, nullptr, nullptr, L.w_2, L.b_2, h->xmid, h->ldE, xout, h->ldE, 4 * E, E, 0, s);
}

// an exploring call's arguments (null: the calls without the tail)
struct Explore {
  int sample, host_eps;
  uint64_t seed;
};

// the chain of one call (h->t already advanced)
int run_step(Handle* h, const Call& c, int host_action, const Explore* x, hipStream_t s) {
  const osrl_cdt_policy_t& p = h->p;
  const int NL = p.num_layers;
  const Rows& emb = c.pl.set[0];
  IngestArgs ia{p,         h->d,      h->dev,   h->x,  h->ldE, h->R, h->TR, c.t, c.reset, host_action, emb.first,
                emb.count, emb.ring,  h->es,    c.table ? h->htab_dev : nullptr, h->dtab};
  (void)hipGetLastError();
  hipLaunchKernelGGL(cdt_act_ingest_kernel, dim3(h->nenv), dim3(256), 0, s, ia);
  // layer 0 keeps its cached q / k / v in the sliding phase (class 0: the new rows only); the last layer runs past
  // its q / k / v for the newest state token only
  for (int l = 0; l < NL; ++l) run_layer(h, c, l, l == 0 ? 0 : 1, l == NL - 1 ? 2 : 1, s);
  const bool feat = p.add_cost_feat || p.mul_cost_feat || p.cat_cost_feat;
  HeadArgs ha{p,     h->d,       h->dev,  h->x + (size_t)NL * h->NR * h->ldE,
              h->ldE, c.pl.srow, feat ? c.pl.srow - h->R + 2 + (p.use_rew ? 1 : 0) : -1,
              ++h->seq, h->es,   h->arrived, h->nenv, c.table ? h->dtab : nullptr,
              h->xdev.sigma, h->xdev.eps, h->xdev.episode_id, h->xdev.head,
              x ? 1 : 0, x ? x->sample : 0, x ? x->host_eps : 0, c.t,
              x ? (uint32_t)x->seed : 0u, x ? (uint32_t)(x->seed >> 32) : 0u};
  hipLaunchKernelGGL(cdt_act_head_kernel, dim3(h->nenv), dim3(kHeadThreads), 0, s, ha);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return wait_published(h->host.seq, 1, 1, h->seq, s);
}

bool valid(const osrl_cdt_policy_t& p, const osrl_cdt_layer_t* layers) {
  if (p.state_dim < 1 || p.action_dim < 1 || p.seq_len < 1 || p.num_layers < 1 || p.num_heads < 1) return false;
  const int E = p.embedding_dim, R = 2 + (p.use_rew ? 1 : 0) + (p.use_cost ? 1 : 0);
  if (E < 1 || E > kMaxE || E % p.num_heads || E / p.num_heads > kMaxD) return false;
  if (R * p.seq_len + (p.cost_prefix ? 1 : 0) > kMaxTok) return false;
  if (p.head_layers < 1 || p.head_layers > OSRL_MAX_LAYERS || p.head_out_width < p.action_dim) return false;
  if ((p.cat_cost_feat ? 2 * E : E) > kMaxHead || p.head_out_width > kMaxHead) return false;
  if ((p.add_cost_feat || p.mul_cost_feat || p.cat_cost_feat) && !p.use_cost) return false;
  if (!layers || !p.state_w || !p.state_b || !p.action_w || !p.action_b || !p.emb_g || !p.emb_b || !p.out_g ||
      !p.out_b)
    return false;
  if ((p.use_rew && (!p.return_w || !p.return_b)) || (p.use_cost && (!p.cost_w || !p.cost_b)) ||
      (p.cost_prefix && (!p.prefix_w || !p.prefix_b)))
    return false;
  for (int l = 0; l < p.head_layers; ++l)
    if (!p.head_w[l] || !p.head_b[l]) return false;
  for (int l = 0; l < p.num_layers; ++l) {
    const osrl_cdt_layer_t& L = layers[l];
    if (!L.ln1_g || !L.ln1_b || !L.w_qkv || !L.b_qkv || !L.w_o || !L.b_o || !L.ln2_g || !L.ln2_b || !L.w_1 || !L.b_1 ||
        !L.w_2 || !L.b_2)
      return false;
  }
  return true;
}

int create(const osrl_cdt_policy_t* desc, const osrl_cdt_layer_t* layers, int n_env, void** handle) {
  if (!desc || !handle || n_env < 1 || n_env > OSRL_CDT_POLICY_MAX_ENVS || !valid(*desc, layers)) return -1;
  const osrl_cdt_policy_t& p = *desc;
  Handle* h = new (std::nothrow) Handle;
  if (!h) return -1;
  h->p = p;
  h->layers.assign(layers, layers + p.num_layers);
  h->R = 2 + (p.use_rew ? 1 : 0) + (p.use_cost ? 1 : 0);
  h->P = p.cost_prefix ? 1 : 0;
  h->TR = h->R * p.seq_len;
  h->NR = h->TR + 1;
  h->nenv = n_env;
  auto up16 = [](int x) { return (x + 15) & ~15; };
  const int E = p.embedding_dim, T = p.seq_len, od = p.state_dim, ad = p.action_dim, NL = p.num_layers;
  const size_t NE = (size_t)n_env;
  h->ldE = up16(E), h->ld3 = up16(3 * E), h->ld4 = up16(4 * E);
  h->t.assign(n_env, -1);
  h->seq = 0;
  h->dmem = nullptr;
  // pinned block: obs [N, od], act_in [N, ad], act_out [N, ad], scalars [N, 4], seq, the per-call table
  constexpr size_t kTabBytes = 4 * (size_t)kTabFields * kTabStride;
  // ... and the exploration tail's: sigma [N], eps [N, ad], episode id [N], the head row [N, 2 ad]
  const size_t pbytes[] = {4 * NE * od, 4 * NE * ad, 4 * NE * ad, 16 * NE, sizeof(uint64_t), kTabBytes,
                           4 * NE,      4 * NE * ad, 4 * NE,      8 * NE * ad};
  hipError_t e = h->blk.alloc(pbytes, 10);
  if (e != hipSuccess) {
    delete h;
    return (int)e;
  }
  auto io = [&](bool dev) {
    const PinnedBlock& b = h->blk;
    return Io{b.seg<float>(0, dev), b.seg<float>(1, dev), b.seg<float>(2, dev), b.seg<float>(3, dev),
              b.seg<uint64_t>(4, dev)};
  };
  h->host = io(false);
  h->dev = io(true);
  auto xio = [&](bool dev) {
    const PinnedBlock& b = h->blk;
    return Handle::Xio{b.seg<float>(6, dev), b.seg<float>(7, dev), b.seg<int32_t>(8, dev), b.seg<float>(9, dev)};
  };
  h->xhost = xio(false);
  h->xdev = xio(true);
  h->htab = h->blk.seg<int32_t>(5, false);
  h->htab_dev = h->blk.seg<int32_t>(5, true);
  // device block, one per episode: window ring, last action, raw embeddings, activations (zeroed: the row strides'
  // padding stays 0); then the head's arrival counter and the device copy of the per-call table
  const size_t NR = h->NR;
  size_t off = 0;
  auto take = [&](size_t floats) {
    const size_t o = off;
    off += (4 * floats + 255) & ~(size_t)255;
    return o;
  };
  const size_t o_s = take((size_t)T * od), o_a = take((size_t)T * ad), o_r = take(T), o_c = take(T), o_t = take(T),
               o_la = take(ad), o_raw = take(NR * h->ldE), o_x = take((size_t)(NL + 1) * NR * h->ldE),
               o_q = take((size_t)NL * NR * h->ld3), o_o = take(NR * h->ldE), o_m = take(NR * h->ldE),
               o_h = take(NR * h->ld4);
  if (off / 4 > (size_t)INT32_MAX) {  // (the attention launch passes the episode stride as 32 bits)
    delete h;
    return -1;
  }
  h->es = (int64_t)(off / 4);
  const size_t total = off * NE + 256 + kTabBytes;
  e = hipMalloc(&h->dmem, total);
  if (e == hipSuccess) e = hipMemset(h->dmem, 0, total);
  if (e != hipSuccess) {
    if (h->dmem) (void)hipFree(h->dmem);
    delete h;
    return (int)e;
  }
  char* base = (char*)h->dmem;
  h->d = Dev{(float*)(base + o_s), (float*)(base + o_a), (float*)(base + o_r), (float*)(base + o_c),
             (int32_t*)(base + o_t), (float*)(base + o_la), (float*)(base + o_raw)};
  h->x = (float*)(base + o_x);
  h->qkv = (float*)(base + o_q);
  h->o = (float*)(base + o_o);
  h->xmid = (float*)(base + o_m);
  h->h = (float*)(base + o_h);
  h->arrived = (uint32_t*)(base + off * NE);
  h->dtab = (int32_t*)(base + off * NE + 256);
  *handle = h;
  return 0;
}

// one call: every episode idles, steps or restarts (mode[e]).  -1, and nothing changed, if a stepping episode was never
// started or would leave the timestep embedding table.
int step_modes(Handle* h, const int32_t* mode, int host_action, const Explore* x, hipStream_t s) {
  const int N = h->nenv;
  if (x && x->sample && h->p.head_out_width < 2 * h->p.action_dim) return -1;  // no log_std columns to sample from
  int nt[OSRL_CDT_POLICY_MAX_ENVS];
  int lead = -1;  // the first episode that runs
  bool same = true;
  for (int e = 0; e < N; ++e) {
    nt[e] = h->t[e];
    if (mode[e] == kIdle) {
      same = false;
      continue;
    }
    if (mode[e] == kStep) {
      if (h->t[e] < 0) return -1;                                 // no episode started
      if (h->p.te && h->t[e] + 1 >= h->p.te_rows) return -1;  // past the timestep embedding table
      nt[e] = h->t[e] + 1;
    } else if (mode[e] == kRestart) {
      nt[e] = 0;
    } else {
      return -1;
    }
    if (lead < 0) lead = e;
    if (mode[e] != mode[lead] || nt[e] != nt[lead]) same = false;
  }
  if (lead < 0) return 0;  // nothing to run
  h->t.assign(nt, nt + N);
  Call c;
  c.table = !same;
  c.pl = plan_of(h, nt[lead], mode[lead] == kRestart);
  c.t = nt[lead];
  c.reset = mode[lead] == kRestart;
  if (c.table) {
    int32_t* tb = h->htab;
    for (int k = 0; k < 3; ++k) c.tot[k] = c.mx[k] = 0;
    for (int e = 0; e < N; ++e) {
      const bool run = mode[e] != kIdle;
      Plan pl = plan_of(h, run ? nt[e] : 0, mode[e] == kRestart);
      tb[kTabMode * kTabStride + e] = mode[e];
      tb[kTabT * kTabStride + e] = run ? nt[e] : 0;
      tb[kTabWs * kTabStride + e] = pl.ws;
      tb[kTabSrow * kTabStride + e] = pl.srow;
      for (int k = 0; k < 3; ++k) {
        const int cnt = run ? pl.set[k].count : 0;
        int32_t* f = tb + (kTabSet + 4 * k) * kTabStride + e;
        f[0] = pl.set[k].first;
        f[kTabStride] = cnt;
        f[2 * kTabStride] = pl.set[k].ring;
        f[3 * kTabStride] = c.tot[k];  // exclusive prefix sum
        c.tot[k] += cnt;
        if (cnt > c.mx[k]) c.mx[k] = cnt;
      }
    }
  }
  return run_step(h, c, host_action ? 1 : 0, x, s);
}

int all_modes(Handle* h, int mode, int host_action, hipStream_t s) {
  int32_t m[OSRL_CDT_POLICY_MAX_ENVS];
  for (int e = 0; e < h->nenv; ++e) m[e] = mode;
  return step_modes(h, m, host_action, nullptr, s);
}

int reset_all(Handle* h, hipStream_t s) { return all_modes(h, kRestart, 0, s); }

int step_all(Handle* h, int host_action, hipStream_t s) { return all_modes(h, kStep, host_action, s); }

int window_of(Handle* h, int env, float* states, float* actions, float* returns, float* costs, int64_t* time_steps,
              int32_t* n_out, hipStream_t st) {
  if (env < 0 || env >= h->nenv) return -1;
  const osrl_cdt_policy_t& p = h->p;
  const int T = p.seq_len, od = p.state_dim, ad = p.action_dim;
  const int t = h->t[env];
  if (t < 0) {
    if (n_out) *n_out = 0;
    return 0;
  }
  const size_t eoff = (size_t)env * (size_t)h->es;
  std::vector<float> s((size_t)T * od), a((size_t)T * ad), r(T), c(T);
  std::vector<int32_t> ts(T);
  hipError_t e = hipMemcpyAsync(s.data(), h->d.win_s + eoff, 4 * s.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(a.data(), h->d.win_a + eoff, 4 * a.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(r.data(), h->d.win_r + eoff, 4 * T, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(c.data(), h->d.win_c + eoff, 4 * T, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(ts.data(), h->d.win_t + eoff, 4 * T, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  const int n = t + 1 < T ? t + 1 : T, t0 = t + 1 - n;
  for (int i = 0; i < n; ++i) {
    const int k = (t0 + i) % T;
    if (states) memcpy(states + (size_t)i * od, &s[(size_t)k * od], 4 * od);
    if (actions) memcpy(actions + (size_t)i * ad, &a[(size_t)k * ad], 4 * ad);
    if (returns) returns[i] = r[k];
    if (costs) costs[i] = c[k];
    if (time_steps) time_steps[i] = ts[k];
  }
  if (n_out) *n_out = n;
  return 0;
}

}  // namespace

extern "C" int osrl_cdt_policy_create(const osrl_cdt_policy_t* desc, const osrl_cdt_layer_t* layers, void** handle) {
  return create(desc, layers, 1, handle);
}

extern "C" int osrl_cdt_policy_create_n(const osrl_cdt_policy_t* desc, const osrl_cdt_layer_t* layers, int32_t n_env,
                                        void** handle) {
  return create(desc, layers, n_env, handle);
}

extern "C" int osrl_cdt_policy_io(void* handle, float** obs, float** act_in, float** act_out) {
  return osrl_cdt_policy_io_n(handle, obs, act_in, act_out, nullptr);
}

extern "C" int osrl_cdt_policy_io_n(void* handle, float** obs, float** act_in, float** act_out, float** scalars) {
  if (!handle) return -1;
  Handle* h = static_cast<Handle*>(handle);
  if (obs) *obs = h->host.obs;
  if (act_in) *act_in = h->host.act_in;
  if (act_out) *act_out = h->host.act_out;
  if (scalars) *scalars = h->host.scalars;
  return 0;
}

// the one-episode calls pass their scalars as arguments: they serve handles of one episode only
extern "C" int osrl_cdt_policy_reset(void* handle, float target_return, float target_cost, void* stream) {
  if (!handle) return -1;
  Handle* h = static_cast<Handle*>(handle);
  if (h->nenv != 1) return -1;
  h->host.scalars[2] = target_return;
  h->host.scalars[3] = target_cost;
  return reset_all(h, (hipStream_t)stream);
}

extern "C" int osrl_cdt_policy_step(void* handle, float reward, float cost, int32_t host_action, void* stream) {
  if (!handle) return -1;
  Handle* h = static_cast<Handle*>(handle);
  if (h->nenv != 1 || h->t[0] < 0) return -1;
  h->host.scalars[0] = reward;
  h->host.scalars[1] = cost;
  return step_all(h, host_action, (hipStream_t)stream);
}

extern "C" int osrl_cdt_policy_reset_n(void* handle, void* stream) {
  if (!handle) return -1;
  return reset_all(static_cast<Handle*>(handle), (hipStream_t)stream);
}

extern "C" int osrl_cdt_policy_step_n(void* handle, int32_t host_action, void* stream) {
  if (!handle) return -1;
  return step_all(static_cast<Handle*>(handle), host_action, (hipStream_t)stream);
}

extern "C" int osrl_cdt_policy_step_slots(void* handle, const int32_t* mode, int32_t host_action, void* stream) {
  if (!handle || !mode) return -1;
  return step_modes(static_cast<Handle*>(handle), mode, host_action, nullptr, (hipStream_t)stream);
}

extern "C" int osrl_cdt_policy_explore_io(void* handle, float** sigma, float** eps, int32_t** episode_id,
                                          float** head) {
  if (!handle) return -1;
  Handle* h = static_cast<Handle*>(handle);
  if (sigma) *sigma = h->xhost.sigma;
  if (eps) *eps = h->xhost.eps;
  if (episode_id) *episode_id = h->xhost.episode_id;
  if (head) *head = h->xhost.head;
  return 0;
}

extern "C" int osrl_cdt_policy_step_slots_explore(void* handle, const int32_t* mode, int32_t host_action,
                                                  int32_t sample, uint64_t explore_seed, int32_t host_eps,
                                                  void* stream) {
  if (!handle || !mode) return -1;
  const Explore x{sample ? 1 : 0, host_eps ? 1 : 0, explore_seed};
  return step_modes(static_cast<Handle*>(handle), mode, host_action, &x, (hipStream_t)stream);
}

extern "C" int osrl_cdt_policy_timesteps(void* handle, int32_t* t) {
  if (!handle || !t) return -1;
  Handle* h = static_cast<Handle*>(handle);
  for (int e = 0; e < h->nenv; ++e) t[e] = h->t[e];
  return 0;
}

extern "C" int osrl_cdt_policy_window(void* handle, float* states, float* actions, float* returns, float* costs,
                                      int64_t* time_steps, int32_t* n_out, void* stream) {
  if (!handle) return -1;
  return window_of(static_cast<Handle*>(handle), 0, states, actions, returns, costs, time_steps, n_out,
                   (hipStream_t)stream);
}

extern "C" int osrl_cdt_policy_window_n(void* handle, int32_t env, float* states, float* actions, float* returns,
                                        float* costs, int64_t* time_steps, int32_t* n_out, void* stream) {
  if (!handle) return -1;
  return window_of(static_cast<Handle*>(handle), env, states, actions, returns, costs, time_steps, n_out,
                   (hipStream_t)stream);
}

extern "C" int osrl_cdt_policy_destroy(void* handle) {
  if (!handle) return -1;
  Handle* h = static_cast<Handle*>(handle);
  (void)hipDeviceSynchronize();  // no launch of this handle may still be running
  hipError_t e = hipFree(h->dmem);
  const hipError_t e2 = h->blk.release();
  delete h;
  return (int)(e != hipSuccess ? e : e2);
}
