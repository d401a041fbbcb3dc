// compact.hip -- variable-length recorded rollouts made dense (osrl_collect_compact, engine/collect.py ModelCollector).
//
// A recorder's tables are episode-major with a fixed pitch: episode e owns rows [e L, e L + L) and has written the first
// len_e = (int)acc[e][2] of them (a rollout that halts on uncertainty stops early: csrc/model_env.hip, kPess).  Two launches,
// out of place:
//   compact_scan_kernel  one workgroup: offsets[e] = sum_{i < e} len_i (int64, exclusive; offsets[E] = the total), each
//                        thread summing a run of consecutive episodes between two block-wide scans in LDS;
//   compact_copy_kernel  grid (E, kSplit): episode e's rows are contiguous in source and destination, so each table moves
//                        as ONE span of len_e * width words from src + e L width to dst + offsets[e] width.
// Integer bookkeeping only; the values move as 32-bit words, bit for bit.  Nothing at or beyond row offsets[E] of a
// destination table is written, and offsets[E] <= E L: a destination as large as its source cannot be overrun.
#include "argmem.h"
#include "rollout_step.h"

namespace {

constexpr int kScanThreads = 256, kCopyThreads = 256, kSplit = 4, kTables = 8;

struct CompactArgs {
  const uint32_t* src[kTables];  // the seven DSRL tables in osrl_collect_t's order, then row_unc (or null with its dst)
  uint32_t* dst[kTables];
  int32_t width[kTables];        // words per row
  const float* acc;              // [E, 4]: acc[e][2] is the episode's length
  int64_t* offsets;              // [E + 1]
  int32_t episodes, episode_len;
};

__device__ __forceinline__ int episode_rows(const float* acc, int e, int L) {
  const float f = acc[(size_t)e * 4 + 2];
  return f >= (float)L ? L : (f > 0.f ? (int)f : 0);  // (a NaN is 0 rows)
}

__global__ __launch_bounds__(kScanThreads) void compact_scan_kernel(const CompactArgs a) {
  __shared__ int64_t part[kScanThreads];
  const int tid = threadIdx.x, E = a.episodes;
  const int per = (E + kScanThreads - 1) / kScanThreads;
  const int lo = min(tid * per, E), hi = min(lo + per, E);
  int64_t s = 0;
  for (int e = lo; e < hi; ++e) s += episode_rows(a.acc, e, a.episode_len);
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < kScanThreads; o <<= 1) {  // inclusive scan of the per-thread sums
    const int64_t v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int64_t off = part[tid] - s;
  for (int e = lo; e < hi; ++e) {
    a.offsets[e] = off;
    off += episode_rows(a.acc, e, a.episode_len);
  }
  if (tid == kScanThreads - 1) a.offsets[E] = part[tid];
}

__global__ __launch_bounds__(kCopyThreads) void compact_copy_kernel(const CompactArgs a) {
  const int e = blockIdx.x;
  const int64_t n = a.offsets[e + 1] - a.offsets[e], off = a.offsets[e];  // n = len_e, in [0, L]
  const int64_t first = (int64_t)blockIdx.y * kCopyThreads + threadIdx.x, stride = (int64_t)kSplit * kCopyThreads;
#pragma unroll
  for (int t = 0; t < kTables; ++t) {
    if (!a.src[t]) continue;  // (uniform)
    const int64_t w = a.width[t], words = n * w;
    const uint32_t* __restrict__ s = a.src[t] + (int64_t)e * a.episode_len * w;
    uint32_t* __restrict__ d = a.dst[t] + off * w;
    for (int64_t i = first; i < words; i += stride) d[i] = s[i];
  }
}

}  // namespace

extern "C" int osrl_collect_compact(const osrl_collect_t* src, const float* src_row_unc, const osrl_collect_t* dst,
                                    float* dst_row_unc, const float* acc, int64_t* offsets, int32_t episodes,
                                    int32_t episode_len, int32_t state_dim, int32_t action_dim, void* stream) {
  if (!src || !dst || !acc || !offsets || episodes < 1 || episode_len < 1 || state_dim < 1 || action_dim < 1) return -1;
  if ((src_row_unc == nullptr) != (dst_row_unc == nullptr)) return -1;
  CompactArgs a;
  memset(&a, 0, sizeof a);
  const float* s[kTables] = {src->observations, src->actions, src->next_observations, src->rewards,
                             src->costs,        src->terminals, src->timeouts,        src_row_unc};
  float* d[kTables] = {dst->observations, dst->actions, dst->next_observations, dst->rewards,
                       dst->costs,        dst->terminals, dst->timeouts,        dst_row_unc};
  const int32_t w[kTables] = {state_dim, action_dim, state_dim, 1, 1, 1, 1, 1};
  for (int t = 0; t < kTables; ++t) {
    if (t < kTables - 1 && (!s[t] || !d[t])) return -1;
    if (s[t] && s[t] == d[t]) return -1;  // out of place
    a.src[t] = reinterpret_cast<const uint32_t*>(s[t]);
    a.dst[t] = reinterpret_cast<uint32_t*>(d[t]);
    a.width[t] = w[t];
  }
  a.acc = acc;
  a.offsets = offsets;
  a.episodes = episodes;
  a.episode_len = episode_len;
  const int r = osrl_argmem::launch(compact_scan_kernel, nullptr, dim3(1), dim3(kScanThreads), 0, (hipStream_t)stream, a);
  if (r != 0) return r;
  return osrl_argmem::launch(compact_copy_kernel, nullptr, dim3((unsigned)episodes, kSplit), dim3(kCopyThreads), 0,
                             (hipStream_t)stream, a);
}
