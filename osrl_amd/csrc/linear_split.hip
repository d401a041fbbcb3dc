// fp32-accurate projections on the bf16 matrix cores of gfx950 ("bf16x3"): Y = A W^T (+ bias) (+ resid), A [M,K] fp32,
// W [N,K] given as three bf16 planes.  The opt-in counterpart of osrl_linear (csrc/mlp.hip) for the CDT projections and
// their input gradients; grown from tools/split_gemm_lab.hip (its v1 kernel with XOR-swizzled 64-byte plane rows).
//
// An fp32 number splits EXACTLY into three bf16 pieces by truncation, a = h + m + l (8 + 8 + 8 significant bits, every
// piece carries the sign of a), so a * w = sum_{i,j} a_i w_j with every a_i w_j exact in fp32 (a 16-bit product).  The
// three terms with i + j >= 5 (m l, l m, l l) are at most 2^-23 |a||w| together and are dropped: SIX
// v_mfma_f32_32x32x16_bf16 per 32 x 32 x 16 block, accumulated in fp32 by the matrix unit, smallest terms first.
//
// Kernel: one 128 x 128 output tile per 4-wave workgroup (48 KB of LDS, two workgroups per CU), wave tile 64 x 64 = 2 x 2
// blocks of 32 x 32, two accumulator sets (h h products / the five cross products).  Per 32-deep slab every thread splits its 16 A values in registers and writes the three planes to
// LDS; the W planes arrive pre-split (osrl_split_planes, once per optimizer step).  Plane rows are 64 bytes with the
// 16-byte chunk position XOR-swizzled by (row >> 2) & 3: conflict-free ds_read_b128 without padding.  The order of
// accumulation is a function of (K) alone: two launches give the same bits, and so do different M.
//
// Non-finite inputs: the truncation split of +-Inf is (Inf, NaN, NaN) and that of a NaN keeps a NaN in at least one piece,
// so every output that a non-finite A or W element feeds is NaN (never a finite number; an Inf that fp32 arithmetic would
// give comes out as NaN too).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/osrl_amd.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 128;             // output tile (rows and columns)
constexpr int kSlab = 32;              // k depth of one staged slab
constexpr int kPitch = 64;             // bytes per plane row in LDS: 32 bf16
constexpr int kPlane = kTile * kPitch; // one plane of a 128-row slab
constexpr int kLds = 6 * kPlane;       // A planes 0-2, W planes 3-5: 49152 B
constexpr int kThreads = 256;
constexpr int kWgPerCu = 2;            // what __launch_bounds__ claims: 512 / 2 = 256 registers per lane (two accumulator sets)

// a = h + m + l exactly (h, m, l: fp32 bit patterns whose low 16 bits are zero = bf16 values)
__device__ __forceinline__ void split3(float a, unsigned& h, unsigned& m, unsigned& l) {
  h = __float_as_uint(a) & 0xffff0000u;
  const float r1 = a - __uint_as_float(h);
  m = __float_as_uint(r1) & 0xffff0000u;
  l = __float_as_uint(r1 - __uint_as_float(m));
}
// two bf16 (the high halves of e0, e1) in one dword, e0 in the low half
__device__ __forceinline__ unsigned pack_hi(unsigned e0, unsigned e1) { return __builtin_amdgcn_perm(e1, e0, 0x07060302u); }

struct SplitArgs {
  const float* A;
  const uint16_t* Wp;  // three planes of W [N, K], `pstride` elements apart
  const float* bias;
  const float* resid;
  float* Y;
  int64_t lda, ldr, ldy, pstride;
  int32_t M, K, N;
};

__global__ __launch_bounds__(kThreads, kWgPerCu) void linear_split_kernel(const SplitArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int row0 = blockIdx.x * kTile, col0 = blockIdx.y * kTile;
  const int K = a.K, nk = K >> 5;
  const size_t pstride = (size_t)a.pstride;
  // ---- sources.  Rows past M read row M - 1 again (never stored): no load leaves the matrix
  const int arow = tid >> 1, ahalf = tid & 1;
  const int srow = min(row0 + arow, a.M - 1);
  const float* ap = a.A + (size_t)srow * a.lda + ahalf * 16;
  const uint16_t* bp[6];
  int boff[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int c = tid + kThreads * j, p = c >> 9, rem = c & 511, col = rem >> 2, q = rem & 3;
    bp[j] = a.Wp + p * pstride + (size_t)(col0 + col) * K + q * 8;
    boff[j] = (3 + p) * kPlane + col * kPitch + (q ^ ((col >> 2) & 3)) * 16;
  }
  const int aoff = arow * kPitch;
  const int asw = (arow >> 2) & 3;
  f32x4 pa[4];
  u32x4 pb[6];
  auto fetch = [&](int ks) {
#pragma unroll
    for (int i = 0; i < 4; ++i) pa[i] = *reinterpret_cast<const f32x4*>(ap + ks * kSlab + 4 * i);
#pragma unroll
    for (int j = 0; j < 6; ++j) pb[j] = *reinterpret_cast<const u32x4*>(bp[j] + ks * kSlab);
  };
  // two accumulator sets: the h h products in one, the five cross products (<= 2^-7 of them) in the other -- every MFMA
  // rounds its accumulator once, and six roundings per 16 k at the size of the full sum were 2.4x the error of one (the
  // single-set form measured 1.2e-6 rms at K = 1024 against 6e-7 for fp32 sgemm on the CPU)
  f32x16 acc[2][2], accs[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[r][c][v] = accs[r][c][v] = 0.f;
  // fragment addresses (bytes): plane p, K16 step s: + p * kPlane + s * 32
  const int fra = wr * 64 + (lane & 31), frb = wc * 64 + (lane & 31);  // (+ 32 per block: (row >> 2) & 3 unchanged)
  const int fa = fra * kPitch, fb = 3 * kPlane + frb * kPitch;
  const int swa = (fra >> 2) & 3, swb = (frb >> 2) & 3;
  fetch(0);
  for (int ks = 0; ks < nk; ++ks) {
    // ---- split this thread's 16 A values, write the planes; pass the pre-split W chunks through
#pragma unroll
    for (int h8 = 0; h8 < 2; ++h8) {
      unsigned hh[8], mm[8], ll[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) split3(pa[2 * h8 + (e >> 2)][e & 3], hh[e], mm[e], ll[e]);
      u32x4 vh, vm, vl;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        vh[d] = pack_hi(hh[2 * d], hh[2 * d + 1]);
        vm[d] = pack_hi(mm[2 * d], mm[2 * d + 1]);
        vl[d] = pack_hi(ll[2 * d], ll[2 * d + 1]);
      }
      const int ao = aoff + (((ahalf * 2 + h8) ^ asw) * 16);
      *reinterpret_cast<u32x4*>(lds + 0 * kPlane + ao) = vh;
      *reinterpret_cast<u32x4*>(lds + 1 * kPlane + ao) = vm;
      *reinterpret_cast<u32x4*>(lds + 2 * kPlane + ao) = vl;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) *reinterpret_cast<u32x4*>(lds + boff[j]) = pb[j];
    __syncthreads();
    if (ks + 1 < nk) fetch(ks + 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 af[2][3], bf[2][3];
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int p = 0; p < 3; ++p)
          af[r][p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(
                                                    lds + fa + p * kPlane + r * 32 * kPitch + (((2 * s + (lane >> 5)) ^ swa) * 16)));
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int p = 0; p < 3; ++p)
          bf[c][p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(
                                                    lds + fb + p * kPlane + c * 32 * kPitch + (((2 * s + (lane >> 5)) ^ swb) * 16)));
      // (A piece, W piece) of the six kept products, smallest first (h = 0, m = 1, l = 2); the four blocks of the wave
      // tile sit between two products on the same accumulator
      constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
      for (int t = 0; t < 6; ++t) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            if (t < 5) accs[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[r][PA[t]], bf[c][PB[t]], accs[r][c], 0, 0, 0);
            else acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[r][PA[t]], bf[c][PB[t]], acc[r][c], 0, 0, 0);
          }
      }
    }
    __syncthreads();
  }
  // ---- epilogue: 32 x 32 block layout: register v of lane l = row (v / 4) * 8 + (l / 32) * 4 + v % 4, column l % 32.
  // One lane-dependent base offset; everything else is wave-uniform (scalar) arithmetic.  Rows past M are not stored.
  {
    const unsigned ldy = (unsigned)a.ldy, ldr = (unsigned)a.ldr;
    const unsigned lrow = (unsigned)(wr * 64 + (lane >> 5) * 4), lcol = (unsigned)(wc * 64 + (lane & 31));
    const int left = a.M - row0 - (int)lrow;  // rows of this lane's column that exist, counted from lrow
    float* yb = a.Y + (size_t)row0 * a.ldy + col0;
    const float* rb_ = a.resid ? a.resid + (size_t)row0 * a.ldr + col0 : nullptr;
    const unsigned oy = lrow * ldy + lcol, orr = lrow * ldr + lcol;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float bv = a.bias ? a.bias[col0 + lcol + c * 32] : 0.f;
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int ro = r * 32 + (v >> 2) * 8 + (v & 3);
          if (ro < left) {
            float y = acc[r][c][v] + accs[r][c][v] + bv;
            if (rb_) y += rb_[orr + (unsigned)ro * ldr + c * 32];
            yb[oy + (unsigned)ro * ldy + c * 32] = y;
          }
        }
    }
  }
}

// Canonical fp32 weights -> bf16 planes, 32 x 32 tiles through LDS so that both orientations are written in rows.
// Entry e = blockIdx.y; its tiles are shared out over the `bx` workgroups of the row (bx is an argument: the kernel reads
// no launch dimension).  f_off: planes of W [out, in]; b_off: planes of W^T [in, out]; the planes of one matrix are out * in
// elements apart; a negative offset skips that orientation.
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ src, uint16_t* __restrict__ pw,
                                                           uint16_t* __restrict__ pt,
                                                           const osrl_pack_entry_t* __restrict__ ents, const int bx) {
  __shared__ float tile[32][33];
  const osrl_pack_entry_t e = ents[blockIdx.y];
  const int out = e.out, in = e.in;
  const size_t n = (size_t)out * in;
  const float* w = src + e.src_off;
  const int ti = (in + 31) >> 5, to = (out + 31) >> 5;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const bool do_w = pw != nullptr && e.f_off >= 0, do_t = pt != nullptr && e.b_off >= 0;
  for (int t = blockIdx.x; t < ti * to; t += bx) {
    const int o0 = (t / ti) * 32, i0 = (t % ti) * 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int o = o0 + ty + 8 * k, i = i0 + tx;
      float x = 0.f;
      if (o < out && i < in) {
        x = w[(size_t)o * in + i];
        if (do_w) {
          unsigned h, m, l;
          split3(x, h, m, l);
          uint16_t* d = pw + e.f_off + (size_t)o * in + i;
          d[0] = (uint16_t)(h >> 16);
          d[n] = (uint16_t)(m >> 16);
          d[2 * n] = (uint16_t)(l >> 16);
        }
      }
      tile[ty + 8 * k][tx] = x;
    }
    __syncthreads();
    if (do_t) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + ty + 8 * k, o = o0 + tx;
        if (o < out && i < in) {
          unsigned h, m, l;
          split3(tile[tx][ty + 8 * k], h, m, l);
          uint16_t* d = pt + e.b_off + (size_t)i * out + o;
          d[0] = (uint16_t)(h >> 16);
          d[n] = (uint16_t)(m >> 16);
          d[2 * n] = (uint16_t)(l >> 16);
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int osrl_linear_split_supported(int32_t M, int32_t K, int32_t N) {
  return (M >= 1 && K >= kSlab && (K % kSlab) == 0 && N >= kTile && (N % kTile) == 0 && (long)N / kTile <= 65535) ? 1 : 0;
}

extern "C" int64_t osrl_linear_split_lds_bytes(void) { return (int64_t)kLds; }

extern "C" int osrl_linear_split(const float* A, int64_t lda, int32_t M, int32_t K, const uint16_t* Wp, int64_t plane_stride,
                                 int32_t N, const float* bias, const float* resid, int64_t ldr, float* Y, int64_t ldy,
                                 void* stream) {
  if (!A || !Wp || !Y || !osrl_linear_split_supported(M, K, N)) return -1;
  if (lda < K || (lda & 3) || ldy < N || (resid && ldr < N) || plane_stride < (int64_t)N * K || (plane_stride & 7)) return -1;
  if ((reinterpret_cast<uintptr_t>(A) & 15) || (reinterpret_cast<uintptr_t>(Wp) & 15)) return -1;
  // the epilogue's in-tile offsets are 32-bit
  if (ldy * kTile >= (int64_t(1) << 31) || (resid && ldr * kTile >= (int64_t(1) << 31))) return -1;
  SplitArgs a;
  a.A = A; a.Wp = Wp; a.bias = bias; a.resid = resid; a.Y = Y;
  a.lda = lda; a.ldr = ldr; a.ldy = ldy; a.pstride = plane_stride;
  a.M = M; a.K = K; a.N = N;
  (void)hipGetLastError();
  hipLaunchKernelGGL(linear_split_kernel, dim3((M + kTile - 1) / kTile, N / kTile), dim3(kThreads), kLds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

extern "C" int osrl_split_planes(const float* src_flat, uint16_t* planes_w, uint16_t* planes_t,
                                 const osrl_pack_entry_t* d_entries, int32_t n_entries, int32_t max_elems, void* stream) {
  if (!src_flat || !d_entries || n_entries < 1 || n_entries > 65535 || (!planes_w && !planes_t)) return -1;
  int bx = (max_elems + 1023) / 1024;
  bx = bx < 1 ? 1 : bx > 64 ? 64 : bx;
  (void)hipGetLastError();
  hipLaunchKernelGGL(split_planes_kernel, dim3(bx, n_entries), dim3(256), 0, (hipStream_t)stream, src_flat, planes_w, planes_t,
                     d_entries, bx);
  return (int)hipGetLastError();
}
