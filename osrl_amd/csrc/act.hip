// act.hip -- the B = 1 (.. 4) act() latency path for gfx950 (MI355X).
//
// Replaces, for the reference's episode-by-episode evaluation loop (XTrainer.rollout: osrl/algorithms/cpq.py:330-347,
// bcql.py:322-340, bc.py:130-149), what one `model.act(obs)` call costs there: `torch.tensor(obs[None]).to(device)`
// (H2D), 3-6 aten kernels (Linear / ReLU / tanh / clamp ...), two `.cpu().numpy()` syncs (D2H) -- cpq.py:240-252,
// bcql.py:236-243, bc.py:66-76 -- with ONE kernel launch and no copy calls:
//   * the observation is written by the host straight into a pinned, device-mapped buffer; the kernel reads it over the
//     host link, runs the whole policy (1-2 chained MLPs + the distribution head) in one workgroup and writes the
//     action (+ log-prob) back into pinned memory, then publishes a sequence number the host spins on (system-scope
//     release / acquire) -- no hipMemcpy, no stream synchronise on the fast path;
//   * the layers are GEMVs: at 1-4 rows a 16-row MFMA tile would be >= 75 % padding and the work is a pure weight
//     stream (86 K parameters = 344 KB for the CPQ actor): LANES own output neurons and read the packed forward
//     weights PF[k/4][n][k%4] -- the copies the optimizer kernel keeps fresh -- so every wave load is 1 KB contiguous
//     and no dot product needs a cross-lane reduction; the 1024 threads split k as well, partials meet in LDS;
// HBM/L2-bound on one CU by design (latency, not throughput): ~345 KB at the per-CU L2 rate is ~3 us.
#include <new>

#include "policy_common.h"

using osrl_rng::U4;
using osrl_rng::philox4x32_10;

namespace {

constexpr int kThreads = 1024;
constexpr int kMaxRows = OSRL_POLICY_MAX_ROWS;  // (the LDS row stride kW / kWideW >= the widest layer and obs+act inputs)

struct Io {  // pinned + device-mapped; the host writes obs / noise, the kernel writes act / logp / seq
  float* obs;     // [kMaxRows, obs_dim]
  float* noise;   // [kMaxRows, noise_dim] explicit standard-normal noise (tests) -- else drawn in the kernel
  float* act;     // [kMaxRows, act_dim]
  float* logp;    // [kMaxRows]
  uint64_t* seq;  // completion counter
};

constexpr int kInline = 128;  // floats of observation carried in the kernel arguments themselves

struct ActArgs {
  osrl_policy_t p;
  Io io;
  int32_t rows, deterministic, host_noise, obs_inline;
  uint32_t k0, k1;
  uint64_t counter, seq;
  // rows * obs_dim <= kInline: the observation travels in the kernarg segment (written by the host with the launch
  // packet, read by scalar loads) instead of being fetched from pinned host memory by the kernel -- one host-link
  // round trip less on the critical path
  float obs[kInline];
};

// y[r][n] = act(b[n] + sum_k W[n][k] x[r][k]) * scale for r < R rows; x, y in LDS (stride W), `red` = LDS scratch.
// The weights are read from the PACKED forward copy PF[k/4][n][k%4] (osrl_pack_weights: zero padded to multiples of 16
// in both dims) with LANES OWNING OUTPUT NEURONS: for a fixed k-quad consecutive n are consecutive 16-byte words, so
// every wave load is 1 KB contiguous and a dot product needs NO cross-lane reduction (a per-neuron wave reduction is a
// chain of six ds_bpermute: measured 5 us per layer).  The 1024 threads = KS k-splits x NL neuron lanes
// (NL = min(256, Np rounded up to a power of two)); each thread issues all its loads back to back; the KS partials meet
// in LDS.
template <int R, int W>
__device__ __forceinline__ void gemv_layer(const float* __restrict__ PF, const float* __restrict__ b, int in, int out,
                                           int act, float scale, const float* x, float* y, float* red) {
  const int tid = threadIdx.x;
  const int Np = round16(out), nq = round16(in) >> 2;
  int NL = 16;
  while (NL < Np && NL < 256) NL <<= 1;
  const int KS = kThreads / NL;
  const int ks = tid / NL, nl = tid - ks * NL;
  const int q0 = (nq * ks) / KS, q1 = (nq * (ks + 1)) / KS;
  const int rs = Np > 256 ? W : NL;  // row stride of `red`: KS * R * rs <= 4 * W * R floats
  const float4* __restrict__ P4 = reinterpret_cast<const float4*>(PF);
  for (int n = nl; n < Np; n += 256) {
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    // (unrolled 8-deep at W = 512; the W = 1024 form spills there at 4 rows, and 4-deep keeps it in registers)
    constexpr int kUnroll = W > 512 ? 4 : 8;
#pragma unroll kUnroll
    for (int q = q0; q < q1; ++q) {
      const float4 w = P4[(size_t)q * Np + n];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float4 xv = *reinterpret_cast<const float4*>(x + r * W + 4 * q);  // same address across the wave
        acc[r] = fmaf(w.x, xv.x, fmaf(w.y, xv.y, fmaf(w.z, xv.z, fmaf(w.w, xv.w, acc[r]))));
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) red[(ks * R + r) * rs + n] = acc[r];
  }
  __syncthreads();
  for (int i = tid; i < R * Np; i += kThreads) {
    const int r = i / Np, n = i - r * Np;
    float s = 0.f;
    for (int k = 0; k < KS; ++k) s += red[(k * R + r) * rs + n];
    y[r * W + n] = n < out ? act_fwd(act, s + b[n]) * scale : 0.f;  // zero = the next layer's k padding
  }
  __syncthreads();
}

// one MLP: input (zero padded to a multiple of 16 columns) in buf[0]; returns the index of the buffer with the output
template <int R, int W>
__device__ __forceinline__ int run_net(const osrl_gemv_net_t& n, float (*buf)[kMaxRows * W], float* red) {
  int cur = 0;
  for (int l = 0; l < n.n_layers; ++l) {
    const float sc = l == n.n_layers - 1 ? n.out_scale : 1.0f;
    gemv_layer<R, W>(n.Wf[l], n.b[l], n.dims[l], n.dims[l + 1], n.acts[l], sc, buf[cur], buf[cur ^ 1], red);
    cur ^= 1;
  }
  return cur;
}

__device__ __forceinline__ float draw_normal(const ActArgs& a, int idx) {
  // Philox4x32-10 keyed like csrc/rng.hip (counter = (element/4, call counter lo, hi, stream 0xAC7)), Box-Muller
  return normal_from_words(
      philox4x32_10(U4{(uint32_t)(idx >> 2), (uint32_t)a.counter, (uint32_t)(a.counter >> 32), 0xAC7u}, a.k0, a.k1), idx);
}

#ifdef OSRL_ACT_STAMPS  // debug: 100 MHz wall-clock stamps of thread 0 into logp[1..7] (rows = 1 runs only)
#define ACT_STAMP(i) if (threadIdx.x == 0) stamp_[i] = wall_clock64();
#else
#define ACT_STAMP(i)
#endif

template <int R, int W = kW>
__global__ __launch_bounds__(kThreads) void policy_act_kernel(const ActArgs a) {
  static_assert(sizeof(float) * (2 * kMaxRows * W + 4 * W * R) <= 160 * 1024, "policy_act_kernel: LDS per workgroup");
  __shared__ __attribute__((aligned(16))) float buf[2][kMaxRows * W];
  __shared__ __attribute__((aligned(16))) float red[4 * W * R];  // [KS][R][stride] partial sums of a layer
#ifdef OSRL_ACT_STAMPS
  long long stamp_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  ACT_STAMP(0);
  const int tid = threadIdx.x;
  const osrl_policy_t& p = a.p;
  const int od = p.obs_dim, ad = p.act_dim, rows = a.rows;
  // ---- stage the observation rows (host-mapped memory) + the second input segment of stage 0
  for (int i = tid; i < R * W; i += kThreads) {
    const int r = i / W, c = i - r * W;
    float v = 0.f;
    if (r < rows) {
      if (c < od) {
        v = a.obs_inline ? a.obs[r * od + c] : a.io.obs[r * od + c];
      } else if (p.kind == OSRL_POLICY_BCQ && c < od + p.latent_dim) {
        // vae.decode(obs) draws z ~ clamp(N(0,1), +-0.5) (net.py:331-334); deterministic callers still sample there,
        // like the reference does
        const int j = r * p.latent_dim + (c - od);
        const float z = a.host_noise ? a.io.noise[j] : draw_normal(a, j);
        v = fminf(fmaxf(z, -0.5f), 0.5f);
      }
    }
    buf[0][i] = v;
  }
  __syncthreads();
  ACT_STAMP(1);
  int cur = run_net<R, W>(p.net[0], buf, red);
  ACT_STAMP(2);
  if (p.kind == OSRL_POLICY_MLP) {  // BC: act_limit * tanh(mlp(obs)) -- tanh + scale are the net's last layer
    for (int i = tid; i < rows * ad; i += kThreads) a.io.act[i] = buf[cur][(i / ad) * W + (i % ad)];
  } else if (p.kind == OSRL_POLICY_GAUSS) {
    // SquashedGaussianMLPActor tail (net.py:176-201): head = (mu | log_std)
    if (tid < rows) {
      const float* h = buf[cur] + tid * W;
      float lp = 0.f;
      for (int j = 0; j < ad; ++j) {
        const float mu = h[j], raw_ls = h[ad + j];
        float e = 0.f;
        if (!a.deterministic) e = a.host_noise ? a.io.noise[tid * ad + j] : draw_normal(a, tid * ad + j);
        squashed_gauss(mu, raw_ls, e, p.max_action, &a.io.act[tid * ad + j], lp);
      }
      a.io.logp[tid] = lp;
    }
  } else {  // OSRL_POLICY_BCQ: a0 = decoder([obs, z]); t = pi([obs, a0]); a = clamp(a0 + phi*max_a*t)  (net.py:58-62)
    float* nxt = buf[cur ^ 1];
    const float* dec = buf[cur];
    for (int i = tid; i < R * W; i += kThreads) {
      const int r = i / W, c = i - r * W;
      float v = 0.f;
      if (r < rows)
        v = c < od ? (a.obs_inline ? a.obs[r * od + c] : a.io.obs[r * od + c]) : (c < od + ad ? dec[r * W + (c - od)] : 0.f);
      nxt[i] = v;
    }
    __syncthreads();
    // keep a0 (rows x ad) in registers of the first threads across the second net
    float a0 = 0.f;
    if (tid < rows * ad) a0 = dec[(tid / ad) * W + (tid % ad)];
    __syncthreads();
    if (cur == 0) {  // run_net expects its input in buf[0]
      for (int i = tid; i < R * W; i += kThreads) buf[0][i] = buf[1][i];
      __syncthreads();
    }
    const int c2 = run_net<R, W>(p.net[1], buf, red);
    if (tid < rows * ad) {
      const float t = buf[c2][(tid / ad) * W + (tid % ad)];
      a.io.act[tid] = bcq_clamp(a0, p.phi, p.max_action, t);
    }
  }
  // ---- publish: results must be visible to the host before the sequence number
  __syncthreads();
  ACT_STAMP(3);
  if (tid == 0) {
    __threadfence_system();
#ifdef OSRL_ACT_STAMPS
    stamp_[4] = wall_clock64();
    a.io.logp[1] = (float)(stamp_[1] - stamp_[0]) * 0.01f;  // us: stage-in
    a.io.logp[2] = (float)(stamp_[2] - stamp_[1]) * 0.01f;  // the network(s)
    a.io.logp[3] = (float)(stamp_[4] - stamp_[2]) * 0.01f;  // head + fence
#endif
    __hip_atomic_store(a.io.seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

struct Handle {
  osrl_policy_t p;
  PinnedBlock blk;
  Io host, dev;
  uint64_t seq, calls;
  int noise_dim;
};

}  // namespace

extern "C" int osrl_policy_create(const osrl_policy_t* desc, void** handle) {
  int noise_dim = 0;
  if (!desc || !handle || !valid_policy(*desc, &noise_dim)) return -1;
  const osrl_policy_t& p = *desc;
  Handle* h = new (std::nothrow) Handle;
  if (!h) return -1;
  h->p = p;
  h->noise_dim = noise_dim;
  h->seq = h->calls = 0;
  const size_t R = sizeof(float) * kMaxRows;
  const size_t bytes[] = {R * p.obs_dim, R * (noise_dim > 0 ? noise_dim : 1), R * p.act_dim, R, sizeof(uint64_t)};
  const hipError_t e = h->blk.alloc(bytes, 5);
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
  *handle = h;
  return 0;
}

extern "C" int osrl_policy_io(void* handle, float** obs, float** noise, float** act, float** logp) {
  if (!handle) return -1;
  Handle* h = static_cast<Handle*>(handle);
  if (obs) *obs = h->host.obs;
  if (noise) *noise = h->host.noise;
  if (act) *act = h->host.act;
  if (logp) *logp = h->host.logp;
  return 0;
}

extern "C" int osrl_policy_act(void* handle, int32_t rows, int32_t deterministic, int32_t host_noise, uint64_t seed,
                               void* stream) {
  if (!handle || rows < 1 || rows > kMaxRows) return -1;
  Handle* h = static_cast<Handle*>(handle);
  ActArgs a;
  a.p = h->p;
  a.io = h->dev;
  a.rows = rows;
  a.deterministic = deterministic;
  a.host_noise = host_noise;
  a.k0 = (uint32_t)seed;
  a.k1 = (uint32_t)(seed >> 32);
  a.counter = ++h->calls;
  a.seq = ++h->seq;
  a.obs_inline = rows * h->p.obs_dim <= kInline;
  if (a.obs_inline) memcpy(a.obs, h->host.obs, sizeof(float) * rows * h->p.obs_dim);
  (void)hipGetLastError();
  if (needs_wide(h->p)) {
    if (rows == 1)
      hipLaunchKernelGGL((policy_act_kernel<1, kWideW>), dim3(1), dim3(kThreads), 0, (hipStream_t)stream, a);
    else
      hipLaunchKernelGGL((policy_act_kernel<kMaxRows, kWideW>), dim3(1), dim3(kThreads), 0, (hipStream_t)stream, a);
  } else if (rows == 1) {
    hipLaunchKernelGGL(policy_act_kernel<1>, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(policy_act_kernel<kMaxRows>, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return wait_published(h->host.seq, 1, 1, a.seq, (hipStream_t)stream);
}

extern "C" int osrl_policy_destroy(void* handle) {
  if (!handle) return -1;
  Handle* h = static_cast<Handle*>(handle);
  (void)hipDeviceSynchronize();  // no launch of this handle may still be writing the pinned block
  const hipError_t e = h->blk.release();
  delete h;
  return (int)e;
}
