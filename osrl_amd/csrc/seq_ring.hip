// SequenceStore(evict="oldest") (common/replay.py, DESIGN.md "Stores that grow"): dropping the oldest trajectories of a
// store keeps the live ones dense and in age order in slots [0, n_traj) of traj_start / traj_len (and of the
// set_sample_prob weights), which is what the window sampler and the cdf kernels index.  That is a shift of the tables
// towards slot 0, in place: the captured graphs hold the tables' addresses, so there is no second buffer to shift into.
//
// One launch of ONE workgroup: source [n_drop, n_live) and destination [0, n_live - n_drop) overlap whenever n_drop is
// below the entries of a pass, so the passes run in ascending order and each is "load, barrier, store".  A pass writes
// [b, b + P) and reads [b + n_drop, b + n_drop + P): what it reads has not been written by an earlier pass (those wrote
// below b), and what it writes is read only by itself -- before the barrier -- or by earlier passes, whose loads precede
// their own barrier.  The pass is parked in LDS over the barrier rather than in registers: the LDS write needs the
// loaded value, so every global load of the pass has RETURNED when its wave reaches the barrier (with registers the
// compiler leaves the loads in flight across it and waits only in front of the stores).  One barrier per pass is enough
// for the global tables; a second one keeps a fast wave's next LDS writes off a slow wave's reads.  No workgroup waits
// on another, there is no workspace, and at <= 2^20 entries of 20 bytes the walk is a few hundred microseconds at most.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/osrl_amd.h"

namespace {

constexpr int kEvictThreads = 1024;  // = the entries of a pass
constexpr int kEvictMax = 1 << 20;

__global__ __launch_bounds__(kEvictThreads) void seq_evict_front_kernel(int64_t* traj_start, int32_t* traj_len,
                                                                        double* traj_w, int32_t* n_traj_dev, int n_live,
                                                                        int n_drop) {
  __shared__ int64_t s_start[kEvictThreads];
  __shared__ double s_w[kEvictThreads];
  __shared__ int32_t s_len[kEvictThreads];
  const int t = (int)threadIdx.x;
  for (int b = 0; b < n_live; b += kEvictThreads) {
    const int i = b + t;
    const int s = i + n_drop;  // (<= 2^21: no overflow)
    const bool keep = s < n_live;
    s_start[t] = keep ? traj_start[s] : 0;
    s_len[t] = keep ? traj_len[s] : 0;
    if (traj_w) s_w[t] = keep ? traj_w[s] : 0.0;
    __syncthreads();  // every load of this pass is done before any of its stores
    if (i < n_live) {
      traj_start[i] = s_start[t];
      traj_len[i] = s_len[t];
      if (traj_w) traj_w[i] = s_w[t];
    }
    __syncthreads();
  }
  if (t == 0) *n_traj_dev = n_live - n_drop;
}

}  // namespace

extern "C" int osrl_seq_evict_front(const osrl_seq_evict_t* e, void* stream) {
  if (!e || !e->traj_start || !e->traj_len || !e->n_traj_dev || e->n_drop < 0 || e->n_drop > e->n_live ||
      e->n_live > kEvictMax)
    return -1;
  (void)hipGetLastError();
  hipLaunchKernelGGL(seq_evict_front_kernel, dim3(1), dim3(kEvictThreads), 0, (hipStream_t)stream, e->traj_start,
                     e->traj_len, e->traj_w, e->n_traj_dev, (int)e->n_live, (int)e->n_drop);
  return (int)hipGetLastError();
}
