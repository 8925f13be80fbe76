// kernels_elem.hip -- the small element-wise kernels of videovec (gfx950 only).
//
//   k_abs_stats  : debug_info's magnitude statistics (net.cpp:580-636, blob.cpp:138-165).
//   table / conversion helpers: k_table_*, k_patch_rows, k_mean_rows, k_gram, k_map_rows, k_dyh_to_float, k_row_normalize.
// (The score / loss kernels are in kernels_score.hip, the parameter update path in kernels_update.hip.)
#include <algorithm>
#include <type_traits>
#include "../../include/videovec.h"
#include "vv_internal.h"

namespace vv {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------- magnitude statistics ----
// The reference's debug_info (Net::ForwardDebugInfo / BackwardDebugInfo / UpdateDebugInfo, net.cpp:580-636) prints asum / count of blobs;
// Blob::asum_data / asum_diff (blob.cpp:138-165) are caffe_gpu_asum calls.  k_abs_stats is k_grad_sumsq's reduction over |x| instead of
// x^2, for up to STAT_SEGS buffers in one launch: a FIXED grid of STAT_BLOCKS x 256 threads walks the buffers one after the other; in each,
// thread t takes the 16-byte items t, t + grid, ... in that order into four double sums (element j of an item into sum j & 3), folds
// them as (x + y) + (z + w) and adds its scalar element (the elements in front of the first 16-byte boundary and behind the last whole
// item, split as clip_split does: thread j of the grid takes the j-th); the wave folds by halves, the workgroup adds its four waves in
// order, and the workgroup that arrives last adds the STAT_BLOCKS partials of every buffer in index order.  No atomics on the sums: the
// same buffers give the same bits on every run.  A NaN or +-Inf element counts in `nonfinite` and in nothing else.  The kernel reads the
// buffers it measures and writes its own partials, arrival counter and records, nothing else.
struct AbsAcc { double s; float mx; unsigned long long nf; };
__device__ __forceinline__ void abs_add(double& s, float& mx, unsigned long long& nf, float v) {
  const float a = fabsf(v);
  if (a <= 3.402823466e38f) { s += (double)a; mx = fmaxf(mx, a); }      // (false for NaN and Inf)
  else ++nf;
}
// EB: bytes per element (4: fp32, optionally minus a second fp32 buffer; 2: f16 / bf16)
template <typename T16> __device__ __forceinline__ AbsAcc abs_segment(const AbsSeg& g, int64_t tid, int64_t nth) {
  constexpr bool F32 = std::is_same<T16, float>::value;
  constexpr int EB = F32 ? 4 : 2, PER = 16 / EB;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  AbsAcc r; r.mx = 0.f; r.nf = 0;
  const char* p = (const char*)g.p;
  const float* q = F32 ? (const float*)g.q : nullptr;
  auto elem = [&](int64_t i) -> float {
    if constexpr (F32) { const float v = ((const float*)p)[i]; return q ? v - q[i] : v; }
    else return T16::to_float(((const uint16_t*)p)[i]);
  };
  if (q && (((uintptr_t)p ^ (uintptr_t)q) & 15) != 0) {         // no common 16-byte grid: scalars throughout
    for (int64_t i = tid; i < g.n; i += nth) abs_add(s[0], r.mx, r.nf, elem(i));
    r.s = s[0];
    return r;
  }
  const int64_t head = std::min<int64_t>(g.n, (int64_t)(((16 - ((uintptr_t)p & 15)) & 15) / EB));
  const int64_t nv = (g.n - head) / PER, tail0 = head + nv * PER, rest = head + (g.n - tail0);      // rest: at most 2 (PER - 1) scalars
  for (int64_t i = tid; i < nv; i += nth) {
    const int64_t o = head + i * PER;
    if constexpr (F32) {
      float4 v = *(const float4*)(p + o * 4);
      if (q) { const float4 w = *(const float4*)(q + o); v.x -= w.x; v.y -= w.y; v.z -= w.z; v.w -= w.w; }
      abs_add(s[0], r.mx, r.nf, v.x); abs_add(s[1], r.mx, r.nf, v.y); abs_add(s[2], r.mx, r.nf, v.z); abs_add(s[3], r.mx, r.nf, v.w);
    } else {
      const uint4 v = *(const uint4*)(p + o * 2);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) abs_add(s[j & 3], r.mx, r.nf, T16::to_float((uint16_t)(w[j >> 1] >> ((j & 1) * 16))));
    }
  }
  r.s = (s[0] + s[1]) + (s[2] + s[3]);
  if (tid < rest) abs_add(r.s, r.mx, r.nf, elem(tid < head ? tid : tail0 + (tid - head)));
  return r;
}
__global__ __launch_bounds__(256) void k_abs_stats(AbsStatsArgs a) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)STAT_BLOCKS * 256;
  __shared__ double ws[STAT_SEGS][4];
  __shared__ float wm[STAT_SEGS][4];
  __shared__ unsigned long long wn[STAT_SEGS][4];
  __shared__ int last;
  for (int k = 0; k < a.nseg; ++k) {
    const AbsSeg& g = a.seg[k];
    AbsAcc r = g.type == STAT_F32 ? abs_segment<float>(g, tid, nth) : g.type == STAT_F16 ? abs_segment<F16>(g, tid, nth) : abs_segment<BF16>(g, tid, nth);
    for (int o = 32; o > 0; o >>= 1) {
      r.s += __shfl_down(r.s, o, 64);
      r.mx = fmaxf(r.mx, __shfl_down(r.mx, o, 64));
      r.nf += __shfl_down(r.nf, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { ws[k][threadIdx.x >> 6] = r.s; wm[k][threadIdx.x >> 6] = r.mx; wn[k][threadIdx.x >> 6] = r.nf; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 0; k < a.nseg; ++k) {
      const int o = k * STAT_BLOCKS + blockIdx.x;
      __hip_atomic_store(a.part_sum + o, ((ws[k][0] + ws[k][1]) + ws[k][2]) + ws[k][3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(a.part_max + o, fmaxf(fmaxf(wm[k][0], wm[k][1]), fmaxf(wm[k][2], wm[k][3])), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(a.part_nf + o, wn[k][0] + wn[k][1] + wn[k][2] + wn[k][3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // (release: the partials are visible at agent scope before the count; acquire: the last arrival sees every other workgroup's)
    last = __hip_atomic_fetch_add(a.arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)STAT_BLOCKS - 1;
  }
  __syncthreads();
  if (!last) return;
  if ((int)threadIdx.x < a.nseg) {             // one thread per buffer, the partials in index order
    const int k = threadIdx.x;
    double sum = 0.0; float mx = 0.f; unsigned long long nf = 0;
#pragma unroll 8
    for (int i = 0; i < STAT_BLOCKS; ++i) {
      sum += __hip_atomic_load(a.part_sum + k * STAT_BLOCKS + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      mx = fmaxf(mx, __hip_atomic_load(a.part_max + k * STAT_BLOCKS + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      nf += __hip_atomic_load(a.part_nf + k * STAT_BLOCKS + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    AbsRec& r = a.rec[a.seg[k].slot];
    r.asum = sum; r.amax = mx; r.reserved_ = 0; r.count = a.seg[k].n; r.nonfinite = (int64_t)nf;
  }
  if (threadIdx.x == 0) __hip_atomic_store(a.arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // for the next launch
}
void launch_abs_stats(const AbsStatsArgs& a, hipStream_t s) { VV_LAUNCH(k_abs_stats, dim3(STAT_BLOCKS), dim3(256), 0, s, a); }

// ------------------------------------------------------------------------------- table --------
template <typename T>
__global__ __launch_bounds__(256) void k_table_convert(const float* src, uint16_t* dst,
                                                       int64_t n_rows, int F, int Fp, float sx) {
  const int64_t n = n_rows * F;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / F; const int f = (int)(i % F);
    dst[r * Fp + f] = T::from_float(src[i] * sx);
  }
}
void launch_table_convert(int prec, const float* src, uint16_t* dst, int64_t n_rows, int F, int Fp,
                          float sx, hipStream_t s) {
  if (prec == 0) hipLaunchKernelGGL(k_table_convert<F16>, dim3(2048), dim3(256), 0, s, src, dst, n_rows, F, Fp, sx);
  else hipLaunchKernelGGL(k_table_convert<BF16>, dim3(2048), dim3(256), 0, s, src, dst, n_rows, F, Fp, sx);
}

// synthetic features, bit-identical to videovector_amd/synth.py:feature_rows
template <typename T>
__global__ __launch_bounds__(256) void k_table_synth(uint16_t* dst, uint64_t seed, int64_t n_rows,
                                                     int F, int Fp, float sx) {
  const int64_t n = n_rows * F;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / F; const int f = (int)(i % F);
    const uint64_t h = mix64(seed, (1ull << 40) + (uint64_t)i);
    const int s = (int)(h & 15) + (int)((h >> 4) & 15) + (int)((h >> 8) & 15) + (int)((h >> 12) & 15);
    const float x = (float)(s > 30 ? s - 30 : 0) * 0.125f;
    dst[r * Fp + f] = T::from_float(x * sx);
  }
}
void launch_table_synth(int prec, uint16_t* dst, uint64_t seed, int64_t n_rows, int F, int Fp,
                        float sx, hipStream_t s) {
  if (prec == 0) hipLaunchKernelGGL(k_table_synth<F16>, dim3(4096), dim3(256), 0, s, dst, seed, n_rows, F, Fp, sx);
  else hipLaunchKernelGGL(k_table_synth<BF16>, dim3(4096), dim3(256), 0, s, dst, seed, n_rows, F, Fp, sx);
}

template <typename T>
__global__ __launch_bounds__(256) void k_table_read(const uint16_t* table, const int32_t* rows,
                                                    int64_t n, int F, int Fp, float inv_sx,
                                                    float* out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * F; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / F; const int f = (int)(i % F);
    const int64_t src = rows ? rows[r] : r;
    out[i] = T::to_float(table[src * Fp + f]) * inv_sx;
  }
}
void launch_table_read(int prec, const uint16_t* table, const int32_t* rows, int64_t n, int F,
                       int Fp, float inv_sx, float* out, hipStream_t s) {
  if (prec == 0) hipLaunchKernelGGL(k_table_read<F16>, dim3(1024), dim3(256), 0, s, table, rows, n, F, Fp, inv_sx, out);
  else hipLaunchKernelGGL(k_table_read<BF16>, dim3(1024), dim3(256), 0, s, table, rows, n, F, Fp, inv_sx, out);
}

// composite rows for quirk Q1: row first_row+p = features 0..F-2 of desc[2p], feature F-1 of desc[2p+1]
__global__ __launch_bounds__(256) void k_patch_rows(uint16_t* table, const int32_t* desc, int64_t first_row,
                                                    int F, int Fp) {
  const int64_t p = blockIdx.x;
  const uint16_t* src = table + (int64_t)desc[2 * p] * Fp;
  const int32_t ls = desc[2 * p + 1];
  uint16_t* dst = table + (first_row + p) * Fp;
  for (int f = threadIdx.x; f < Fp; f += 256) {
    uint16_t v = src[f];
    if (f == F - 1) v = ls >= 0 ? table[(int64_t)ls * Fp + f] : (uint16_t)0;
    dst[f] = v;
  }
}
void launch_patch_rows(uint16_t* table, const int32_t* desc, int64_t n_patch, int64_t first_row, int F,
                       int Fp, hipStream_t s) {
  hipLaunchKernelGGL(k_patch_rows, dim3((unsigned)n_patch), dim3(256), 0, s, table, desc, first_row, F, Fp);
}

// scratch row first_row+i = sum_j coeff[j] * table[rows[i*k+j]]   (TEST branch: average_for_test)
template <typename T>
__global__ __launch_bounds__(256) void k_mean_rows(uint16_t* table, const int32_t* rows, int k, const float* coeff,
                                                   int64_t first_row, int Fp) {
  const int64_t i = blockIdx.x;
  uint16_t* dst = table + (first_row + i) * Fp;
  for (int f = threadIdx.x; f < Fp; f += 256) {
    float s = 0.f;
    for (int j = 0; j < k; ++j) s += coeff[j] * T::to_float(table[(int64_t)rows[i * k + j] * Fp + f]);
    dst[f] = T::from_float(s);
  }
}
void launch_mean_rows(int prec, uint16_t* table, const int32_t* rows, int64_t n, int k, const float* coeff,
                      int64_t first_row, int Fp, hipStream_t s) {
  if (prec == 0) hipLaunchKernelGGL(k_mean_rows<F16>, dim3((unsigned)n), dim3(256), 0, s, table, rows, k, coeff, first_row, Fp);
  else hipLaunchKernelGGL(k_mean_rows<BF16>, dim3((unsigned)n), dim3(256), 0, s, table, rows, k, coeff, first_row, Fp);
}

// out[i][j] = alpha * sum_d x[i][d] x[j][d]  (fp32; retrieval_stats_layer.cpp:208-209 uses alpha = -2).
// 64x64 tile per 256-thread block, 4x4 outputs per thread; n is a few hundred to a few thousand.
__global__ __launch_bounds__(256) void k_gram(const float* x, int n, int dim, float alpha, float* out) {
  __shared__ float As[16][64 + 1], Bs[16][64 + 1];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < dim; k0 += 16) {
    for (int t = threadIdx.x; t < 64 * 16; t += 256) {
      const int r = t >> 4, c = t & 15;
      As[c][r] = (i0 + r < n && k0 + c < dim) ? x[(int64_t)(i0 + r) * dim + k0 + c] : 0.f;
      Bs[c][r] = (j0 + r < n && k0 + c < dim) ? x[(int64_t)(j0 + r) * dim + k0 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      float a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { a[u] = As[c][ty * 4 + u]; b[u] = Bs[c][tx * 4 + u]; }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] += a[u] * b[v];
    }
    __syncthreads();
  }
  for (int u = 0; u < 4; ++u)
    for (int v = 0; v < 4; ++v) {
      const int i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
      if (i < n && j < n) out[(int64_t)i * n + j] = alpha * acc[u][v];
    }
}
void launch_gram(const float* x, int n, int dim, float alpha, float* out, hipStream_t s) {
  const dim3 grid((n + 63) / 64, (n + 63) / 64);
  hipLaunchKernelGGL(k_gram, grid, dim3(256), 0, s, x, n, dim, alpha, out);
}

// idx (data-layer layout, -1 = empty slot) -> table rows, padded to Rp with the all-zero row
// An index outside [0, row_limit) -- -1 is the documented "empty slot", anything else can only come from a device
// index array the host never saw -- reads the all-zero row instead of memory outside the table.
__global__ void k_map_rows(const int32_t* idx, int32_t* rows, int R, int Rp, int32_t zero_row, int32_t row_limit) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < Rp) rows[i] = (i < R && idx[i] >= 0 && idx[i] < row_limit) ? idx[i] : zero_row;
}
void launch_map_rows(const int32_t* idx, int32_t* rows, int R, int Rp, int32_t zero_row, int32_t row_limit,
                     hipStream_t s) {
  hipLaunchKernelGGL(k_map_rows, dim3((Rp + 255) / 256), dim3(256), 0, s, idx, rows, R, Rp, zero_row, row_limit);
}

template <typename T>
__global__ void k_dyh_to_float(const uint16_t* dYh, int R, int D, int Dp, float inv_sg, float* out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)R * D; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / D; const int d = (int)(i % D);
    out[i] = T::to_float(dYh[r * Dp + d]) * inv_sg;
  }
}
void launch_dyh_to_float(int prec, const uint16_t* dYh, int R, int D, int Dp, float inv_sg,
                         float* out, hipStream_t s) {
  if (prec == 0) hipLaunchKernelGGL(k_dyh_to_float<F16>, dim3(1024), dim3(256), 0, s, dYh, R, D, Dp, inv_sg, out);
  else hipLaunchKernelGGL(k_dyh_to_float<BF16>, dim3(1024), dim3(256), 0, s, dYh, R, D, Dp, inv_sg, out);
}

// NORMALIZATION forward on rows of x in place (normalization_layer.cu:10-45): y = x/(|x|+1e-10)
__global__ __launch_bounds__(256) void k_row_normalize(float* x, int n, int D) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wave;
  if (r >= n) return;
  float* p = x + (int64_t)r * D;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s += p[d] * p[d];
  s = wave_sum(s);
  const float inv = 1.f / (sqrtf(s) + 1e-10f);
  for (int d = lane; d < D; d += 64) p[d] *= inv;
}
void launch_row_normalize(float* x, int n, int D, hipStream_t s) {
  hipLaunchKernelGGL(k_row_normalize, dim3((n + 3) / 4), dim3(256), 0, s, x, n, D);
}


}  // namespace vv
