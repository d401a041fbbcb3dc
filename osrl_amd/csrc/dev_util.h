// dev_util.h -- the small device helpers every translation unit used to restate: the 64-lane butterflies, pin(), the
// device-coherent words of an in-launch exchange, and the sign-in of its last arriver.
// Everything is internal to the including translation unit.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// 64-lane butterflies: the result is valid in every lane, and the order of the additions is fixed
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// A loaded value that is only consumed under a condition gets its load SUNK into that branch by the compiler (and a
// select on it turned into such a branch), where it waits alone: s_waitcnt vmcnt(0) per load, one memory round trip
// after the other.  pin() makes the value unconditionally live at the point of the call, so a group of loads issued
// back to back in front of a group of pin()s stays in flight together.
__device__ __forceinline__ void pin(float& x) { asm volatile("" : "+v"(x)); }

// device-coherent words (relaxed agent-scope atomics = sc1 stores / loads: written through to, and read from, the level
// all XCDs share): what workgroups on different XCDs exchange inside one launch, with no cache touched
__device__ __forceinline__ void coh_put(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float coh_get(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The sign-in of a deterministic in-launch reduction, called by ONE thread of a workgroup whose coh_put()s are its own:
// true for the last of the n workgroups to sign in, which then re-arms the counter for the next launch and goes on to
// add everybody's words with coh_get() in a fixed order.  Wait-free: a workgroup is the last one or leaves.
// arrive_last_acked() takes the caller's stores as already acknowledged (s_waitcnt vmcnt(0) in every wave that stored,
// then a barrier: mlp_dw.hip, where all threads store); arrive_last() waits for the calling thread's own stores first.
// (glue.hip's grid_last_arriver is NOT this protocol: plain stores ordered by __threadfence().)
__device__ __forceinline__ bool arrive_last_acked(unsigned* counter, int n) {
  const unsigned seen = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool last = seen == (unsigned)n - 1;
  if (last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // every one signed in: re-arm
  return last;
}
__device__ __forceinline__ bool arrive_last(unsigned* counter, int n) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's words are acknowledged before the arrival
  return arrive_last_acked(counter, n);
}

}  // namespace
