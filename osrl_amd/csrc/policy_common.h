// policy_common.h -- what the act paths share: the element arithmetic of the MLP policies' heads (act.hip and
// act_vec.hip: one definition of the formulas of net.py:176-201 and net.py:58-62 in device code), and the host side of a
// policy handle (act.hip, act_vec.hip, cdt_act.hip): the pinned, device-mapped I/O block, the wait on the sequence
// numbers a launch publishes, and the checks of an MLP policy descriptor.
// Nothing here knows its caller: where the kernels differ (row index type, live[] mask, the key of the device-drawn
// noise) each keeps its own loop around these functions.  Everything is internal to the including translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <chrono>

#include "../../include/osrl_amd.h"
#include "loss_terms.h"
#include "philox.h"

namespace {

// LDS row widths (floats) of the MLP act kernels' two instantiations: 512 for nets whose layers are all <= 512 wide
// (every net of the fused-kernel widths), 1024 = OSRL_MAX_WIDTH for the wider ones (twice the LDS)
constexpr int kW = 512, kWideW = OSRL_MAX_WIDTH;

__device__ __forceinline__ float act_fwd(int act, float x) {
  if (act == OSRL_ACT_RELU) return fmaxf(x, 0.0f);
  if (act == OSRL_ACT_TANH) return tanhf(x);
  return x;
}
__device__ __forceinline__ int round16(int x) { return (x + 15) & ~15; }

// standard-normal draw `idx` of the Philox words of counter idx / 4: Box-Muller on the word pair idx selects
__device__ __forceinline__ float normal_from_words(const osrl_rng::U4& r, int idx) {
  const uint32_t u[4] = {r.x, r.y, r.z, r.w};
  const int pair = (idx & 3) >> 1;
  const float u1 = ((float)(u[2 * pair] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = ((float)(u[2 * pair + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float rad = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincosf(6.283185307179586f * u2, &s, &c);
  return (idx & 1) ? rad * s : rad * c;
}

// one element of the SquashedGaussianMLPActor tail (net.py:176-201): stores max_action * tanh(mu + std * e) to *action
// and applies the element's two log-prob terms to `lp`, in the order the kernels have always used (the store first; the
// terms one after the other: two roundings, a single summed increment would not give the same bits)
__device__ __forceinline__ void squashed_gauss(float mu, float raw_log_std, float e, float max_action, float* action,
                                               float& lp) {
  const float ls = fminf(fmaxf(raw_log_std, kLogStdMin), kLogStdMax);
  const float u = mu + expf(ls) * e;
  *action = max_action * tanhf(u);
  lp += -0.5f * e * e - ls - 0.9189385332046727f;
  lp -= 2.0f * (0.6931471805599453f - u - softplus(-2.0f * u));
}

// BCQ's perturbed action (net.py:58-62): clamp(a0 + phi * max_action * t)
__device__ __forceinline__ float bcq_clamp(float a0, float phi, float max_action, float t) {
  return fminf(fmaxf(a0 + phi * max_action * t, -max_action), max_action);
}

// ---- host side ------------------------------------------------------------------------------------------------

// One pinned (mapped + portable), zeroed allocation carved into 256-byte-aligned segments; a segment is handed out as
// its host or its device address.  Freed by release() (a handle's destroy, which reports the error) or with its owner.
struct PinnedBlock {
  static constexpr int kMaxSegs = 12;
  char *host = nullptr, *dev = nullptr;
  size_t off[kMaxSegs + 1] = {0};

  PinnedBlock() = default;
  PinnedBlock(const PinnedBlock&) = delete;
  PinnedBlock& operator=(const PinnedBlock&) = delete;
  ~PinnedBlock() { (void)release(); }

  // n <= kMaxSegs segments of the given byte sizes, in this order (more: hipErrorInvalidValue, nothing allocated)
  hipError_t alloc(const size_t* bytes, int n) {
    if (n < 1 || n > kMaxSegs) return hipErrorInvalidValue;
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + ((bytes[i] + 255) & ~(size_t)255);
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, off[n], hipHostMallocMapped | hipHostMallocPortable);
    if (e != hipSuccess) return e;
    host = static_cast<char*>(p);
    memset(host, 0, off[n]);
    e = hipHostGetDevicePointer(&p, host, 0);
    if (e != hipSuccess) {
      (void)release();
      return e;
    }
    dev = static_cast<char*>(p);
    return hipSuccess;
  }
  template <class T>
  T* seg(int i, bool device) const {
    return reinterpret_cast<T*>((device ? dev : host) + off[i]);
  }
  hipError_t release() {
    const hipError_t e = host ? hipHostFree(host) : hipSuccess;
    host = dev = nullptr;
    return e;
  }
};

// Waits until the `count` counters seq[0], seq[stride], .. have all reached `want`.  Fast path: spin on the numbers
// the kernels publish (system-scope release) -- a stream synchronise costs more than the kernels; after 2 ms fall back
// to it (also surfaces a faulted launch instead of spinning forever).  0, a HIP error, or -2: the launches ran but did
// not publish (should be impossible).
inline int wait_published(const volatile uint64_t* seq, int stride, int count, uint64_t want, hipStream_t stream) {
  const auto t0 = std::chrono::steady_clock::now();
  int t = 0;
  for (uint32_t it = 0; t < count; ++it) {
    if (seq[stride * t] >= want) {
      ++t;
      continue;
    }
    if ((it & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
      const hipError_t e = hipStreamSynchronize(stream);
      if (e != hipSuccess) return (int)e;
      for (int u = t; u < count; ++u)
        if (seq[stride * u] < want) return -2;
      break;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return 0;
}

inline bool valid_net(const osrl_gemv_net_t& n) {
  if (n.n_layers < 1 || n.n_layers > OSRL_MAX_LAYERS || n.out_scale == 0.f) return false;
  for (int l = 0; l <= n.n_layers; ++l)
    if (n.dims[l] < 1 || n.dims[l] > kWideW) return false;
  for (int l = 0; l < n.n_layers; ++l)
    if (!n.Wf[l] || !n.b[l]) return false;
  return true;
}

// an MLP policy descriptor the act kernels can run; *noise_dim = floats of standard-normal noise a row takes.
// (BCQ's staged rows [obs, z] and [obs, a0] are its nets' inputs: dims[0] <= OSRL_MAX_WIDTH bounds them.)
inline bool valid_policy(const osrl_policy_t& p, int* noise_dim) {
  if (p.kind < OSRL_POLICY_MLP || p.kind > OSRL_POLICY_BCQ || p.obs_dim < 1 || p.act_dim < 1 || !valid_net(p.net[0]))
    return false;
  const int in0 = p.net[0].dims[0], out0 = p.net[0].dims[p.net[0].n_layers];
  if (p.kind == OSRL_POLICY_MLP) {
    *noise_dim = 0;
    return in0 == p.obs_dim && out0 == p.act_dim;
  }
  if (p.kind == OSRL_POLICY_GAUSS) {
    *noise_dim = p.act_dim;
    return in0 == p.obs_dim && out0 == 2 * p.act_dim;
  }
  *noise_dim = p.latent_dim;
  return valid_net(p.net[1]) && p.latent_dim >= 1 && in0 == p.obs_dim + p.latent_dim && out0 == p.act_dim &&
         p.net[1].dims[0] == p.obs_dim + p.act_dim && p.net[1].dims[p.net[1].n_layers] == p.act_dim;
}

// a layer or a staged input row wider than kW: the kWideW instantiation
inline bool needs_wide(const osrl_policy_t& p) {
  const int nn = p.kind == OSRL_POLICY_BCQ ? 2 : 1;
  for (int i = 0; i < nn; ++i)
    for (int l = 0; l <= p.net[i].n_layers; ++l)
      if (p.net[i].dims[l] > kW) return true;
  return false;
}

}  // namespace
