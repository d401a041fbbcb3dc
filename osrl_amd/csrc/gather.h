// gather.h -- the device side of the replay sampler (rng.hip osrl_replay_gather / osrl_step_begin), shared with the
// one-launch regression step of mlp.hip: a row's index is a pure function of (seed, step, stream, row), so any kernel
// that knows the step draws the same minibatch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/osrl_amd.h"
#include "philox.h"

#define OSRL_MAX_FIELDS 8

namespace osrl_gather {

struct GatherArgs {
  const float* src[OSRL_MAX_FIELDS];
  float* dst[OSRL_MAX_FIELDS];
  int32_t width[OSRL_MAX_FIELDS];
  float scale[OSRL_MAX_FIELDS];
  int32_t n_fields, batch;
  int64_t n_rows;
  int32_t* idx_out;
  uint32_t k0, k1, stream_id;
  const osrl_step_state_t* st;
  const uint64_t* cum;  // [n_rows] fixed-point inclusive cdf of the sampling weights (include/osrl_amd.h), or NULL = uniform
  // a store that grows (ReplayStore(capacity=)): the device word that holds the live row count -- n_rows is then the
  // tables' capacity and the draw runs over clamp(*n_rows_dev, 1, n_rows); NULL = the draw over n_rows, as always
  const int64_t* n_rows_dev;
};

// The row count the draw runs over.  Whatever the word holds, the result is inside [1, n_rows]: every index stays inside
// the allocation.  One load ahead of the index (the address is uniform; the word only changes between launches).
template <class AR>
__device__ __forceinline__ int64_t live_rows(AR a) {
  const int64_t cap = a.n_rows;
  const int64_t* __restrict__ p = a.n_rows_dev;
  if (!p) return cap;
  const int64_t v = *p;
  return v < 1 ? 1 : v < cap ? v : cap;
}

// The weighted draw: the first i in [0, n) with cum[i] > min(u, 2^64 - 2), found by the L lanes that hold the row (lane id l;
// every one of them returns the index).  cum is non-decreasing, so that index is the number of entries <= the word.  A
// k-ary search: each round the lanes probe L evenly spaced entries of the open range and a ballot counts the ones that do
// not exceed the word, which cuts the range to one of L + 1 segments -- ceil(log_(L+1) n) dependent loads (3 at 2^18 rows
// and 4 at 2^22 with a wave, 4 and 5 with half a wave) where one lane bisecting takes 18 / 22.  Whatever the table
// holds, the result is inside [0, n).  All lanes of the wave may call it with different rows per half (L = 32): the
// loop runs until both halves are done, a finished half probes nothing.
template <int L>
__device__ __forceinline__ int64_t search_cum(const uint64_t* __restrict__ cum, int64_t n, uint64_t u, int l, int half) {
  const uint64_t word = u < ~0ull - 1 ? u : ~0ull - 1;
  int64_t lo = 0, hi = n - 1;  // the index lies in [lo, hi]; entries [lo, hi) are still to be looked at
  while (__any(hi > lo)) {
    const int64_t len = hi - lo;
    const int64_t s = (len + L) / (L + 1);  // segment length: probes at lo + s - 1, lo + 2 s - 1, ...
    const int64_t p = lo + (int64_t)(l + 1) * s - 1;
    const bool below = len > 0 && p < hi && cum[p] <= word;
    const uint64_t m = __ballot(below);
    const int c = L == 64 ? __popcll(m) : __popc((uint32_t)(m >> (32 * half)));
    if (len > 0) {
      const int64_t top = lo + (int64_t)(c + 1) * s - 1;  // the first probe that exceeded the word, if there was one
      hi = (c < L && top < hi) ? top : hi;
      lo += (int64_t)c * s;
    }
  }
  return lo;
}

// One row of every table, index `idx` -> batch row `b`, by L lanes (lane id l): ALL fields' loads are requested before
// the first store.  (As a loop "for each field: load, scale, store" the fields were one dependent round trip each --
// six for the CPQ tables -- and the step prologue, which nothing overlaps, took 10.8 us: profiles/r3_timeline.txt.)
// Columns beyond 2 L of a wide table take the plain loop.
template <int L, class AR>
__device__ __forceinline__ void gather_row(AR a, int64_t idx, int b, int l) {
  float v[OSRL_MAX_FIELDS][2];
  const int nf = a.n_fields;
#pragma unroll
  for (int f = 0; f < OSRL_MAX_FIELDS; ++f) {
    const bool on = f < nf;
    const int w = on ? a.width[f] : 0;
    const float* __restrict__ s = (on ? a.src[f] : a.src[0]) + (on ? (size_t)idx * w : 0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = l + j * L;
      const float x = s[c < w ? c : 0];  // (clamped address + select: no branch around the load)
      v[f][j] = c < w ? x : 0.f;
    }
  }
#pragma unroll
  for (int f = 0; f < OSRL_MAX_FIELDS; ++f) {
    if (f < nf) {
      const int w = a.width[f];
      const float sc = a.scale[f];
      float* __restrict__ d = a.dst[f] + (size_t)b * w;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = l + j * L;
        if (c < w) d[c] = v[f][j] * sc;
      }
      if (w > 2 * L) {
        const float* __restrict__ s = a.src[f] + (size_t)idx * w;
        for (int c = l + 2 * L; c < w; c += L) d[c] = s[c] * sc;
      }
    }
  }
}

// one wave per sampled row; lanes stride over the row's columns (coalesced both sides)
// AR: `const GatherArgs&` (kernel argument by value) or `const OSRL_CAS GatherArgs&` (device-resident block, argmem.h)
// NT: the workgroup size (a compile-time constant: no kernel here reads blockDim)
template <class AR, int NT>
__device__ __forceinline__ void gather_body(AR a, uint32_t step, int block) {
  using namespace osrl_rng;
  const int lane = threadIdx.x & 63;
  const int b = block * (NT / 64) + (threadIdx.x >> 6);
  if (b >= a.batch) return;
  const U4 r = philox4x32_10(U4{(uint32_t)b, 0x5eedu, step, a.stream_id}, a.k0, a.k1);
  // 64-bit multiply-shift maps a 64-bit uniform onto [0, n_rows) (bias < 2^-40 for n_rows < 2^24)
  const uint64_t u = ((uint64_t)r.x << 32) | r.y;
  const uint64_t* __restrict__ cum = a.cum;
  const int64_t n = live_rows<AR>(a);
  const int64_t idx = cum ? search_cum<64>(cum, n, u, lane, 0) : (int64_t)__umul64hi(u, (uint64_t)n);
  if (lane == 0 && a.idx_out) a.idx_out[b] = (int32_t)idx;
  gather_row<64, AR>(a, idx, b, lane);
}

// rows [16 tile, 16 tile + 16) by one 8-wave workgroup in ONE pass: half a wave per row (the same draws, the same rows
// as gather_body; two passes of a wave per row are two dependent index -> row round trips)
template <class AR>
__device__ __forceinline__ void gather_tile16(AR a, uint32_t step, int tile) {
  using namespace osrl_rng;
  const int lane = threadIdx.x & 63, l = lane & 31;
  const int b = tile * 16 + 2 * (int)(threadIdx.x >> 6) + (lane >> 5);
  if (b >= a.batch) return;
  const U4 r = philox4x32_10(U4{(uint32_t)b, 0x5eedu, step, a.stream_id}, a.k0, a.k1);
  const uint64_t u = ((uint64_t)r.x << 32) | r.y;
  const uint64_t* __restrict__ cum = a.cum;
  const int64_t n = live_rows<AR>(a);
  const int64_t idx = cum ? search_cum<32>(cum, n, u, l, lane >> 5) : (int64_t)__umul64hi(u, (uint64_t)n);
  if (l == 0 && a.idx_out) a.idx_out[b] = (int32_t)idx;
  gather_row<32, AR>(a, idx, b, l);
}

// host: the descriptor of osrl_replay_gather's arguments (false: invalid)
inline bool fill(GatherArgs& a, int32_t n_fields, const float* const* src, float* const* dst, const int32_t* width,
                 const float* scale, int64_t n_rows, int32_t batch, uint64_t seed, uint32_t stream_id,
                 const osrl_step_state_t* st, const uint64_t* cum = nullptr, const int64_t* n_rows_dev = nullptr) {
  for (int f = 0; f < OSRL_MAX_FIELDS; ++f) {
    a.src[f] = f < n_fields ? src[f] : nullptr;
    a.dst[f] = f < n_fields ? dst[f] : nullptr;
    a.width[f] = f < n_fields ? width[f] : 0;
    a.scale[f] = (f < n_fields && scale) ? scale[f] : 1.0f;
    if (f < n_fields && (!a.src[f] || !a.dst[f] || a.width[f] < 1)) return false;
  }
  a.n_fields = n_fields;
  a.batch = n_fields > 0 ? batch : 0;
  a.n_rows = n_rows;
  a.idx_out = nullptr;
  a.k0 = (uint32_t)seed;
  a.k1 = (uint32_t)(seed >> 32);
  a.stream_id = stream_id;
  a.st = st;
  a.cum = cum;
  a.n_rows_dev = n_rows_dev;
  return true;
}

}  // namespace osrl_gather
