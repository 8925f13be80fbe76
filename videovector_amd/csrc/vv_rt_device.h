// vv_rt_device.h -- device code the gallery path's kernel files share (kernels_retrieval.hip, kernels_ivf.hip): the body of the fp32
// similarity tile, and the 64-bit (distance, index) keys with the wave-wide sorted list that keeps the k smallest of them.  One
// definition each, so that a kernel of either file gives the same float for the same (query row, item row) and orders the same
// pairs the same way.  gfx950 (MI355X, CDNA4) only; included by .hip files alone.
#pragma once
#include "vv_internal.h"

namespace vv {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------- similarity tile
// 128 x 128 output tile per 256-thread workgroup, K advanced 32 at a time.  Wave w owns the 64 x 64 sub-tile
// (w >> 1, w & 1) as 2 x 2 accumulators of v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain).  Operand tiles
// travel global -> registers -> LDS; the registers are loaded one K-tile ahead of the MFMAs that consume the LDS image.
// LDS rows are 36 floats (32 + 4 pad): the 16-byte fragment reads of 32 lanes, one row apart, then cover all banks.
// Lane (r = lane & 31, h = lane >> 5) reads k = 8 kk + 4 h .. + 3 of its row for both operands and feeds element j to
// MFMA step j, so one MFMA sums k = 8 kk + j and 8 kk + 4 + j: a fixed permutation of K, the same for every output.
constexpr int RT_LD = RT_BK + 4;

// The tile's accumulation, whatever rows the caller chose: thread t stages float4 (t & 7) of rows (t >> 3) + 32 i, i = 0..3, of both
// tiles -- ga_i / gb_i point at that float4 of K-tile 0 of the thread's i-th row of either operand (named registers: an array indexed
// inside the K loop's `if` would live in scratch memory).  sA: RT_BM x RT_LD floats, sB: RT_BN x RT_LD, 16-byte aligned.  acc[a][b][e]
// is then the dot product of tile row wm 64 + a 32 + (e & 3) + 8 (e >> 2) + 4 h with tile column wn 64 + b 32 + r (the C/D map of the
// 32x32 MFMA).  The first statement of the K loop is a barrier, so a caller that runs the body again needs none for sA / sB.
__device__ __forceinline__ void rt_tile_mma(const float4* ga0, const float4* ga1, const float4* ga2, const float4* ga3,
                                            const float4* gb0, const float4* gb1, const float4* gb2, const float4* gb3, int Dp,
                                            float* sA, float* sB, f32x16 (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int srow = tid >> 3, c4 = tid & 7, lo = srow * RT_LD + c4 * 4;
  float4 ra0 = ga0[0], ra1 = ga1[0], ra2 = ga2[0], ra3 = ga3[0];
  float4 rb0 = gb0[0], rb1 = gb1[0], rb2 = gb2[0], rb3 = gb3[0];

#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  const int kt_n = Dp / RT_BK;
  for (int kt = 0; kt < kt_n; ++kt) {
    __syncthreads();                                   // the previous tile's fragment reads are done
    *(float4*)&sA[lo] = ra0; *(float4*)&sA[lo + 32 * RT_LD] = ra1; *(float4*)&sA[lo + 64 * RT_LD] = ra2; *(float4*)&sA[lo + 96 * RT_LD] = ra3;
    *(float4*)&sB[lo] = rb0; *(float4*)&sB[lo + 32 * RT_LD] = rb1; *(float4*)&sB[lo + 64 * RT_LD] = rb2; *(float4*)&sB[lo + 96 * RT_LD] = rb3;
    __syncthreads();
    if (kt + 1 < kt_n) {
      const int o = (kt + 1) * (RT_BK / 4);
      ra0 = ga0[o]; ra1 = ga1[o]; ra2 = ga2[o]; ra3 = ga3[o];
      rb0 = gb0[o]; rb1 = gb1[o]; rb2 = gb2[o]; rb3 = gb3[o];
    }
#pragma unroll
    for (int kk = 0; kk < RT_BK / 8; ++kk) {
      float4 fa[2], fb[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        fa[t] = *(const float4*)&sA[(wm * 64 + t * 32 + r) * RT_LD + kk * 8 + h * 4];
        fb[t] = *(const float4*)&sB[(wn * 64 + t * 32 + r) * RT_LD + kk * 8 + h * 4];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float a0 = j == 0 ? fa[0].x : j == 1 ? fa[0].y : j == 2 ? fa[0].z : fa[0].w;
        const float a1 = j == 0 ? fa[1].x : j == 1 ? fa[1].y : j == 2 ? fa[1].z : fa[1].w;
        const float b0 = j == 0 ? fb[0].x : j == 1 ? fb[0].y : j == 2 ? fb[0].z : fb[0].w;
        const float b1 = j == 0 ? fb[1].x : j == 1 ? fb[1].y : j == 2 ? fb[1].z : fb[1].w;
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- keys
// the distance's bits as an unsigned integer of the same order: the high word of the key
__device__ inline uint32_t rt_word(float d) {
  const uint32_t u = __float_as_uint(d);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline uint64_t rt_key(float d, uint32_t g) { return ((uint64_t)rt_word(d) << 32) | g; }
__device__ inline float rt_key_dist(uint64_t key) {
  uint32_t u = (uint32_t)(key >> 32);
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return __uint_as_float(u);
}
constexpr uint64_t RT_NOKEY = ~0ull;

// ---------------------------------------------------------------------------------------------- the k smallest keys of a wave
// One wave keeps the k smallest keys it has seen, sorted, ONE PER LANE (lanes >= k hold RT_NOKEY), and offers every new key
// against the k-th.  After the first few thousand elements almost nothing passes, so the scan runs at the rate of its loads.
__device__ inline void rt_insert(uint64_t x, uint64_t& mine, int lane, int k) {
  const int pos = __popcll(__ballot(mine < x));             // sorted: the lanes below x are lanes 0 .. pos-1
  const uint64_t up = __shfl_up(mine, 1);
  if (lane == pos) mine = x; else if (lane > pos) mine = up;
  if (lane >= k) mine = RT_NOKEY;
}
// wave-uniform call; `key` differs per lane, `cand` says whether this lane offers it
__device__ inline void rt_offer(uint64_t key, bool cand, uint64_t& mine, uint64_t& kth, int lane, int k) {
  uint64_t m = __ballot(cand && key < kth);
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    rt_insert(__shfl(key, src), mine, lane, k);
  }
  kth = __shfl(mine, k - 1);
}

}  // namespace vv
