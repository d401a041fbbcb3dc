// act_vec.hip -- the lockstep act() path of the MLP policies for gfx950 (MI355X): N <= OSRL_POLICY_MAX_ENVS episodes on
// as many host environments, one C call per environment step for all of them.
//
// act.hip answers one `model.act(obs)` of the reference's episode loop with one launch of a GEMV kernel (<= 4 rows:
// a 16-row MFMA tile would be mostly padding there).  With N environments stepped side by side the same weight stream
// serves N rows, so the layers become fp32 MFMA (v_mfma_f32_16x16x4_f32) over 16-row tiles:
//   * ONE launch per step, one workgroup per 16-row tile of slots; a workgroup runs the whole policy (1-2 chained MLPs
//     + the distribution head) with its activations in LDS -- no dependency between workgroups, nothing to chain;
//   * a layer's 16-column output tiles are dealt to the 8 waves, two per wave and pass; a wave walks ALL of K for its
//     tiles, so a dot product's k-order is fixed by the layer shape alone (no split-K, no reduction): a slot's action
//     is the same bits whatever N is, whichever slot it sits in and whatever its neighbours do;
//   * the weights are the packed forward copies PF[k/4][n][k%4] and the canonical biases of the flat optimizer groups
//     (what act.hip reads): a lane's B operand for four consecutive k is one 16-byte word, 16 lanes = 256 B contiguous;
//   * observations / noise / active mask / (episode id, step) are read from a pinned, device-mapped block, actions and
//     log-probs are written to it, and each workgroup publishes a sequence number of its own that the host spins on;
//   * noise drawn on the device is Philox keyed by (seed, the slot's episode id, the slot's step, element): an episode
//     replays identically in any wave and slot;
//   * the exploration tail (osrl_policy_act_explore_n): a = clip(a_pi + sigma[slot] * eps) on the action the kernel would
//     publish, rollout_step.h's arithmetic with the collectors' noise keys -- a run on host environments records what the
//     device collector would have drawn for the same (seed, episode id, step, column).
#include <new>

#include "policy_common.h"
#include "rollout_step.h"

using osrl_rng::philox4x32_10;
using osrl_rng::U4;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 512, kWaves = 8;
constexpr int kMaxEnvs = OSRL_POLICY_MAX_ENVS, kTile = 16, kMaxTiles = (kMaxEnvs + kTile - 1) / kTile;
constexpr int kPad = 4;  // floats: rows 16 bytes apart in the banks, a tile's 16 A reads of one k-quad do not collide

struct Io {  // pinned + device-mapped; the host writes obs / noise / active / meta, the kernel writes act / logp / seq
  float* obs;       // [n_env, obs_dim]
  float* noise;     // [n_env, noise_dim] explicit standard-normal noise -- else drawn in the kernel
  float* act;       // [n_env, act_dim]
  float* logp;      // [n_env]
  int32_t* active;  // [n_env] 0: the slot idles (its act / logp words are left alone)
  int32_t* meta;    // [n_env, 2] (episode id, step): the key of the slot's device-drawn noise
  uint64_t* seq;    // [kMaxTiles] (64 bytes apart) completion counter of each workgroup
  float* sigma;     // [n_env] exploration scale of the slot (read by exploring calls only)
  float* eps;       // [n_env, act_dim] injected exploration noise -- else drawn in the kernel
};
constexpr int kSeqStride = 8;  // uint64 words between two tiles' counters

struct VecArgs {
  osrl_policy_t p;
  Io io;
  int32_t n_env, deterministic, host_noise, pad_;
  uint32_t k0, k1;
  uint64_t seq;
  int32_t explore, host_eps;  // explore = 0: the calls without the tail (sigma / eps are not read)
  uint32_t x0, x1;            // the exploration seed
};

// y[r][n] = act(b[n] + sum_k W[n][k] x[r][k]) * scale for the tile's 16 rows; x, y in LDS (row stride W + kPad).
// Lane (ar = lane & 15, kq = lane >> 4) holds A = x[ar][16 kb + 4 kq + t] and B = W[n0 + ar][16 kb + 4 kq + t] for MFMA t
// of k-block kb; the accumulator's element i is y[4 kq + i][n0 + ar].  Columns out .. round16(out) are written as zero:
// they are the next layer's k padding.
template <int W>
__device__ __forceinline__ void mfma_layer(const float* __restrict__ PF, const float* __restrict__ b, int in, int out,
                                           int act, float scale, const float* x, float* y) {
  constexpr int S = W + kPad, kC = 8;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ar = lane & 15, kq = lane >> 4;
  const int Np = round16(out), nkb = round16(in) >> 4, nct = Np >> 4;
  const f32x4* __restrict__ W4 = reinterpret_cast<const f32x4*>(PF);
  const float* xr = x + ar * S + 4 * kq;
  for (int c0 = w; c0 < nct; c0 += 2 * kWaves) {
    const int c1 = c0 + kWaves;
    const bool two = c1 < nct;  // (wave-uniform)
    const f32x4* __restrict__ p0 = W4 + (size_t)kq * Np + 16 * c0 + ar;
    const f32x4* __restrict__ p1 = W4 + (size_t)kq * Np + 16 * (two ? c1 : c0) + ar;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    // kC k-blocks per round: every load of the round is issued before its first MFMA
    for (int kc = 0; kc < nkb; kc += kC) {
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
      for (int i = 0; i < 4; ++i) y[(4 * kq + i) * S + col] = col < out ? act_fwd(act, acc0[i] + bb) * scale : 0.f;
    }
    if (two) {
      const int col = 16 * c1 + ar;
      const float bb = col < out ? b[col] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) y[(4 * kq + i) * S + col] = col < out ? act_fwd(act, acc1[i] + bb) * scale : 0.f;
    }
  }
  __syncthreads();
}

// one MLP: input (zero padded to a multiple of 16 columns) in buf[cur]; returns the index of the buffer with the output
template <int W>
__device__ __forceinline__ int run_net(const osrl_gemv_net_t& n, float (*buf)[kTile * (W + kPad)], int cur) {
  for (int l = 0; l < n.n_layers; ++l) {
    const float sc = l == n.n_layers - 1 ? n.out_scale : 1.0f;
    mfma_layer<W>(n.Wf[l], n.b[l], n.dims[l], n.dims[l + 1], n.acts[l], sc, buf[cur], buf[cur ^ 1]);
    cur ^= 1;
  }
  return cur;
}

// element idx of the standard-normal draws of (episode id, step): Philox4x32-10 with counter = (idx / 4, episode id,
// step, stream 0xAC8) and the seed as key, Box-Muller on the word pair idx selects.  Nothing of the handle, of n_env or
// of the slot enters.
__device__ __forceinline__ float draw_normal(const VecArgs& a, int32_t episode, int32_t step, int idx) {
  return normal_from_words(
      philox4x32_10(U4{(uint32_t)(idx >> 2), (uint32_t)episode, (uint32_t)step, 0xAC8u}, a.k0, a.k1), idx);
}

// The exploration tail on element j of slot s, whose scale is sg: csrc/rollout_step.h's draw (eps is the pinned row's, or
// drawn with the explore seed as key) and, under noise only, the clip.  sg == 0 returns v as it is.
__device__ __forceinline__ float explore_tail(const VecArgs& a, float sg, int s, int j, float v) {
  if (sg == 0.f) return v;
  v = osrl_rollout::explore(v, sg, [&] {
    return osrl_rollout::explore_eps((uint32_t)a.io.meta[2 * s], (uint32_t)a.io.meta[2 * s + 1], j, a.x0, a.x1,
                                     a.host_eps ? a.io.eps : nullptr, (size_t)s * a.p.act_dim + j);
  });
  return fminf(fmaxf(v, -a.p.max_action), a.p.max_action);
}

template <int W>
__global__ __launch_bounds__(kThreads) void policy_vec_kernel(const VecArgs a) {
  constexpr int S = W + kPad;
  static_assert(sizeof(float) * 2 * kTile * S <= 160 * 1024, "policy_vec_kernel: LDS per workgroup");
  __shared__ __attribute__((aligned(16))) float buf[2][kTile * S];
  __shared__ int live[kTile];  // 1: the row's slot exists and is active
  __shared__ float sig[kTile];  // the row's exploration scale; 0: the action is published as it is
  const int tid = threadIdx.x;
  const osrl_policy_t& p = a.p;
  const int od = p.obs_dim, ad = p.act_dim, ld = p.latent_dim;
  const int s0 = blockIdx.x * kTile;  // the tile's first slot
  if (tid < kTile) {
    live[tid] = s0 + tid < a.n_env && a.io.active[s0 + tid] != 0;
    sig[tid] = a.explore && live[tid] ? a.io.sigma[s0 + tid] : 0.f;
  }
  __syncthreads();
  // ---- stage the observation rows (host-mapped memory) + the second input segment of stage 0; idle rows are zero
  const int in0 = round16(p.net[0].dims[0]);
  for (int i = tid; i < kTile * in0; i += kThreads) {
    const int r = i / in0, c = i - r * in0, s = s0 + r;
    float v = 0.f;
    if (live[r]) {
      if (c < od) {
        v = a.io.obs[(size_t)s * od + c];
      } else if (p.kind == OSRL_POLICY_BCQ && c < od + ld) {
        // vae.decode(obs) draws z ~ clamp(N(0,1), +-0.5) (net.py:331-334); deterministic callers sample there too
        const int j = c - od;
        const float z = a.host_noise ? a.io.noise[(size_t)s * ld + j]
                                     : draw_normal(a, a.io.meta[2 * s], a.io.meta[2 * s + 1], j);
        v = fminf(fmaxf(z, -0.5f), 0.5f);
      }
    }
    buf[0][r * S + c] = v;
  }
  __syncthreads();
  int cur = run_net<W>(p.net[0], buf, 0);
  if (p.kind == OSRL_POLICY_MLP) {  // BC: act_limit * tanh(mlp(obs)) -- tanh + scale are the net's last layer
    for (int i = tid; i < kTile * ad; i += kThreads) {
      const int r = i / ad, j = i - r * ad;
      if (live[r]) a.io.act[(size_t)(s0 + r) * ad + j] = explore_tail(a, sig[r], s0 + r, j, buf[cur][r * S + j]);
    }
  } else if (p.kind == OSRL_POLICY_GAUSS) {
    // SquashedGaussianMLPActor tail (net.py:176-201): head = (mu | log_std); one thread per row, j ascending
    if (tid < kTile && live[tid]) {
      const int s = s0 + tid;
      const float* h = buf[cur] + tid * S;
      const int32_t episode = a.io.meta[2 * s], step = a.io.meta[2 * s + 1];
      float lp = 0.f;
      for (int j = 0; j < ad; ++j) {
        const float mu = h[j], raw_ls = h[ad + j];
        float e = 0.f;
        if (!a.deterministic) e = a.host_noise ? a.io.noise[(size_t)s * ad + j] : draw_normal(a, episode, step, j);
        float act;
        squashed_gauss(mu, raw_ls, e, p.max_action, &act, lp);
        a.io.act[(size_t)s * ad + j] = explore_tail(a, sig[tid], s, j, act);
      }
      a.io.logp[s] = lp;
    }
  } else {  // OSRL_POLICY_BCQ: a0 = decoder([obs, z]); t = pi([obs, a0]); a = clamp(a0 + phi*max_a*t)  (net.py:58-62)
    float* nxt = buf[cur ^ 1];
    const float* dec = buf[cur];
    // a0 (16 x ad) stays in registers across the second net: element tid + kThreads * q
    constexpr int kKeep = kTile * W / kThreads;
    float a0[kKeep];
#pragma unroll
    for (int q = 0; q < kKeep; ++q) {
      const int i = tid + kThreads * q;
      a0[q] = i < kTile * ad ? dec[(i / ad) * S + (i % ad)] : 0.f;
    }
    const int in1 = round16(p.net[1].dims[0]);
    for (int i = tid; i < kTile * in1; i += kThreads) {
      const int r = i / in1, c = i - r * in1;
      float v = 0.f;
      if (live[r]) v = c < od ? a.io.obs[(size_t)(s0 + r) * od + c] : (c < od + ad ? dec[r * S + (c - od)] : 0.f);
      nxt[r * S + c] = v;
    }
    __syncthreads();
    const int c2 = run_net<W>(p.net[1], buf, cur ^ 1);
#pragma unroll
    for (int q = 0; q < kKeep; ++q) {
      const int i = tid + kThreads * q;
      if (i < kTile * ad) {
        const int r = i / ad, j = i - r * ad;
        const float t = buf[c2][r * S + j];
        if (live[r])
          a.io.act[(size_t)(s0 + r) * ad + j] =
              explore_tail(a, sig[r], s0 + r, j, bcq_clamp(a0[q], p.phi, p.max_action, t));
      }
    }
  }
  // ---- publish: results must be visible to the host before the sequence number
  __syncthreads();
  if (tid == 0) {
    __threadfence_system();
    __hip_atomic_store(a.io.seq + kSeqStride * blockIdx.x, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

struct Handle {
  osrl_policy_t p;
  PinnedBlock blk;
  Io host, dev;
  uint64_t seq;
  int n_env, noise_dim;
  bool wide;
};

}  // namespace

extern "C" int osrl_policy_create_n(const osrl_policy_t* desc, int32_t n_env, void** handle) {
  int noise_dim = 0;
  if (!desc || !handle || n_env < 1 || n_env > kMaxEnvs || !valid_policy(*desc, &noise_dim)) return -1;
  const osrl_policy_t& p = *desc;
  Handle* h = new (std::nothrow) Handle;
  if (!h) return -1;
  h->p = p;
  h->n_env = n_env;
  h->noise_dim = noise_dim;
  h->seq = 0;
  h->wide = needs_wide(p);
  const size_t N = (size_t)n_env, F = sizeof(float) * N, I = sizeof(int32_t) * N;
  const size_t bytes[] = {F * p.obs_dim, F * (noise_dim > 0 ? noise_dim : 1), F * p.act_dim, F, I, 2 * I,
                          sizeof(uint64_t) * kSeqStride * kMaxTiles, F, F * p.act_dim};
  const hipError_t e = h->blk.alloc(bytes, 9);
  if (e != hipSuccess) {
    delete h;
    return (int)e;
  }
  auto io = [&](bool dev) {
    const PinnedBlock& b = h->blk;
    return Io{b.seg<float>(0, dev),   b.seg<float>(1, dev),   b.seg<float>(2, dev),   b.seg<float>(3, dev),
              b.seg<int32_t>(4, dev), b.seg<int32_t>(5, dev), b.seg<uint64_t>(6, dev),
              b.seg<float>(7, dev),   b.seg<float>(8, dev)};
  };
  h->host = io(false);
  h->dev = io(true);
  for (int i = 0; i < n_env; ++i) h->host.active[i] = 1;
  *handle = h;
  return 0;
}

extern "C" int osrl_policy_io_n(void* handle, float** obs, float** noise, float** act, float** logp, int32_t** active,
                                int32_t** meta) {
  if (!handle) return -1;
  Handle* h = static_cast<Handle*>(handle);
  if (obs) *obs = h->host.obs;
  if (noise) *noise = h->host.noise;
  if (act) *act = h->host.act;
  if (logp) *logp = h->host.logp;
  if (active) *active = h->host.active;
  if (meta) *meta = h->host.meta;
  return 0;
}

extern "C" int osrl_policy_explore_io_n(void* handle, float** sigma, float** eps) {
  if (!handle) return -1;
  Handle* h = static_cast<Handle*>(handle);
  if (sigma) *sigma = h->host.sigma;
  if (eps) *eps = h->host.eps;
  return 0;
}

namespace {

// one call; explore = 0: without the tail
int act_n(Handle* h, int32_t deterministic, int32_t host_noise, uint64_t seed, int32_t explore, uint64_t explore_seed,
          int32_t host_eps, void* stream) {
  VecArgs a;
  a.p = h->p;
  a.io = h->dev;
  a.n_env = h->n_env;
  a.deterministic = deterministic;
  a.host_noise = host_noise;
  a.pad_ = 0;
  a.k0 = (uint32_t)seed;
  a.k1 = (uint32_t)(seed >> 32);
  a.seq = ++h->seq;
  a.explore = explore;
  a.host_eps = host_eps;
  a.x0 = (uint32_t)explore_seed;
  a.x1 = (uint32_t)(explore_seed >> 32);
  const int tiles = (h->n_env + kTile - 1) / kTile;
  (void)hipGetLastError();
  if (h->wide)
    hipLaunchKernelGGL(policy_vec_kernel<kWideW>, dim3(tiles), dim3(kThreads), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(policy_vec_kernel<kW>, dim3(tiles), dim3(kThreads), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return wait_published(h->host.seq, kSeqStride, tiles, a.seq, (hipStream_t)stream);
}

}  // namespace

extern "C" int osrl_policy_act_n(void* handle, int32_t deterministic, int32_t host_noise, uint64_t seed, void* stream) {
  if (!handle) return -1;
  return act_n(static_cast<Handle*>(handle), deterministic, host_noise, seed, 0, 0, 0, stream);
}

extern "C" int osrl_policy_act_explore_n(void* handle, int32_t deterministic, int32_t host_noise, uint64_t seed,
                                         uint64_t explore_seed, int32_t host_eps, void* stream) {
  if (!handle) return -1;
  return act_n(static_cast<Handle*>(handle), deterministic, host_noise, seed, 1, explore_seed, host_eps ? 1 : 0, stream);
}

extern "C" int osrl_policy_destroy_n(void* handle) {
  if (!handle) return -1;
  Handle* h = static_cast<Handle*>(handle);
  (void)hipDeviceSynchronize();  // no launch of this handle may still be writing the pinned block
  const hipError_t e = h->blk.release();
  delete h;
  return (int)e;
}
