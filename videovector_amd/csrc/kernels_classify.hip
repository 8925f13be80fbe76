// kernels_classify.hip -- per-class accuracy and average precision of a score matrix, nothing sorted.
// gfx950 (MI355X, CDNA4) only.  Replaces ClassificationStatsLayer::Forward_cpu (src/caffe/layers/classification_stats_layer.cpp:36-95):
// the argmax walk over every row (:49-67), the std::sort of 2 n pairs per class (:72-74) and the walk over the first n sorted
// entries (:79-84).
//
// Form (DESIGN.md 'Classification statistics'): one COLUMN BLOCK of the score matrix at a time.
//   k_cls_rows    the running first maximum of every row over the block's columns (:50-61); behind the last block one integer
//                 atomic per correctly predicted row (:63-66); counts NaNs
//   k_cls_pack    the block's columns as contiguous key arrays col[j][0 .. n) (a tiled transpose)
//   k_cls_count   a tile of CLS_TILE positives of one class in registers, one segment of the class's column streamed through
//                 LDS: for every positive p with score s, G = items above s, P = positives above s, E = positives equal to s of
//                 lower item index -- three integers, added to cnt[position of p][3] by integer atomics
//   k_cls_final   one workgroup per class: term(p) = (P + E + 1) / (G + E + 1) in double for every positive with s >= 0, summed
//                 in a fixed order, divided by the class's count (:85)
// Why these three counts are the sorted walk: the reference sorts n dummies (0, false) with the n real (score, label == c) pairs by
// std::greater<pair> and visits entries 0 .. n-1 (:42-43, :56-57, :72-80).  A positive below zero lies behind the n dummies and is
// never visited; a positive p with s >= 0 (-0.0f included: -0 == 0 and true > false) is preceded by exactly the G items above it and
// the E equal positives taken before it (equal pairs are interchangeable; item order decides here), so it sits at position G + E and
// is the (P + E + 1)-th positive met (:81-82).  The key the counting pass compares and the key a positive carries are the same
// stored float of col[]: nothing is evaluated twice.
#include "vv_internal.h"

namespace vv {

// ---------------------------------------------------------------------------------------------- row pass
// L lanes per row (a power of two, 1 .. 64; consecutive lanes read consecutive columns).  src: the block's first column of row 0,
// `pitch` floats between two rows; the block holds columns c0 .. c0 + cb - 1 of the matrix.  rmax / rarg [n]: the running maximum
// and its column, written by the first block (c0 == 0) and replaced only on strict > afterwards, so the LOWEST column attaining
// the maximum stays (:58-61; -0.0f == 0.0f).  last: labels [n] are read and correct[label] += 1 where rarg == label.
__global__ __launch_bounds__(256) void k_cls_rows(const float* __restrict__ src, int64_t pitch, int n, int c0, int cb, int L,
                                                  int last, const int32_t* __restrict__ labels, float* __restrict__ rmax,
                                                  int32_t* __restrict__ rarg, uint32_t* __restrict__ correct,
                                                  unsigned long long* __restrict__ nan_count) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / L;
  const int sub = (int)(t % L);
  const bool live = row < n;
  float best = -__builtin_inff();
  int arg = 0x7fffffff;
  uint32_t nans = 0;
  if (live) {
    const float* r = src + row * pitch;
    for (int j = sub; j < cb; j += L) {
      const float v = r[j];
      nans += v != v;
      if (arg == 0x7fffffff || v > best) { best = v; arg = c0 + j; }      // the lane's first element, then strict > (ascending j)
    }
  }
  for (int o = 1; o < L; o <<= 1) {                                        // L-lane groups are aligned: lane ^ o stays inside
    const float ob = __shfl_xor(best, o);
    const int oa = __shfl_xor(arg, o);
    if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
  }
  if (nans) atomicAdd(nan_count, (unsigned long long)nans);
  if (live && sub == 0) {
    if (c0 > 0) {
      const float pb = rmax[row];
      if (!(best > pb)) { best = pb; arg = rarg[row]; }
    }
    if (last) {
      const int32_t lab = labels[row];
      if (arg == lab) atomicAdd(&correct[lab], 1u);
    } else {
      rmax[row] = best; rarg[row] = arg;
    }
  }
}
void launch_cls_rows(const float* src, int64_t pitch, int n, int c0, int cb, int last, const int32_t* labels, float* rmax,
                     int32_t* rarg, uint32_t* correct, unsigned long long* nan_count, hipStream_t s) {
  int L = 1;
  while (L < cb && L < 64) L <<= 1;
  const int64_t threads = (int64_t)n * L;
  hipLaunchKernelGGL(k_cls_rows, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, src, pitch, n, c0, cb, L, last, labels,
                     rmax, rarg, correct, nan_count);
}

// ---------------------------------------------------------------------------------------------- column pack
// col[j][i] = src[i][j] for the block's cb columns; npitch floats between two columns.  32 x 32 tiles through LDS (33-float rows).
__global__ __launch_bounds__(256) void k_cls_pack(const float* __restrict__ src, int64_t pitch, int n, int cb,
                                                  float* __restrict__ col, int64_t npitch) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t i0 = (int64_t)blockIdx.x * 32;
  const int j0 = blockIdx.y * 32;
#pragma unroll
  for (int r = 0; r < 32; r += 8) {
    const int64_t i = i0 + ty + r;
    const int j = j0 + tx;
    tile[ty + r][tx] = (i < n && j < cb) ? src[i * pitch + j] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 32; r += 8) {
    const int j = j0 + ty + r;
    const int64_t i = i0 + tx;
    if (i < n && j < cb) col[(int64_t)j * npitch + i] = tile[tx][ty + r];
  }
}
void launch_cls_pack(const float* src, int64_t pitch, int n, int cb, float* col, int64_t npitch, hipStream_t s) {
  hipLaunchKernelGGL(k_cls_pack, dim3((unsigned)((n + 31) / 32), (unsigned)((cb + 31) / 32)), dim3(256), 0, s, src, pitch, n, cb,
                     col, npitch);
}

// ---------------------------------------------------------------------------------------------- counting pass
// grid (S, tiles of this pass).  tiles[t] = {first position in pos_idx, positives in the tile (<= CLS_TILE), class, 0}; the class's
// keys are column class - c0 of the block.  Thread t of the workgroup holds positive pos_idx[first + t].  The segment's keys go
// through LDS CLS_STAGE at a time as two arrays: sk the key, sp the key where the item is a positive of the class and -inf elsewhere (items past n: -inf in both,
// which nothing is above or -- for a visited positive, s >= 0 -- equal to).  Every lane reads the same LDS address: a broadcast.
// labels has npitch entries (the pad reads as no class); seg is a multiple of CLS_STAGE.
__global__ __launch_bounds__(256) void k_cls_count(const float* __restrict__ col, int64_t npitch, int n, int seg, int c0,
                                                   const int32_t* __restrict__ labels, const int32_t* __restrict__ pos_idx,
                                                   const int4* __restrict__ tiles, int tile0, uint32_t* __restrict__ cnt) {
  __shared__ __attribute__((aligned(16))) float sk[CLS_STAGE];
  __shared__ __attribute__((aligned(16))) float sp[CLS_STAGE];
  const int4 tl = tiles[tile0 + blockIdx.y];
  const int tid = threadIdx.x;
  const float* key = col + (int64_t)(tl.z - c0) * npitch;
  const bool have = tid < tl.y;
  int p = -1;
  float s = 0.f;
  if (have) { p = pos_idx[tl.x + tid]; s = key[p]; }
  const float ninf = -__builtin_inff();
  uint32_t G = 0, P = 0, E = 0;
  const int begin = blockIdx.x * seg, end = min(n, begin + seg);
  for (int base = begin; base < end; base += CLS_STAGE) {
    __syncthreads();                                               // the previous stage's reads are done
    {
      const int i = base + tid * 4;                                // CLS_STAGE == 4 * 256; i + 3 < npitch (a multiple of 64)
      float4 v = make_float4(ninf, ninf, ninf, ninf);
      int4 lb = make_int4(-1, -1, -1, -1);
      if (i < end) { v = *(const float4*)(key + i); lb = *(const int4*)(labels + i); }
      if (i + 1 >= end) v.y = ninf;
      if (i + 2 >= end) v.z = ninf;
      if (i + 3 >= end) v.w = ninf;
      *(float4*)&sk[tid * 4] = v;
      *(float4*)&sp[tid * 4] = make_float4(lb.x == tl.z ? v.x : ninf, lb.y == tl.z ? v.y : ninf, lb.z == tl.z ? v.z : ninf,
                                           lb.w == tl.z ? v.w : ninf);
    }
    __syncthreads();
    const int jlim = p - base;                                     // staged entry j is an item of lower index than p iff j < jlim
#pragma unroll 4
    for (int j = 0; j < CLS_STAGE; j += 4) {
      const float4 a = *(const float4*)&sk[j];
      const float4 b = *(const float4*)&sp[j];
      G += (a.x > s) + (a.y > s) + (a.z > s) + (a.w > s);
      P += (b.x > s) + (b.y > s) + (b.z > s) + (b.w > s);
      E += (b.x == s && j < jlim) + (b.y == s && j + 1 < jlim) + (b.z == s && j + 2 < jlim) + (b.w == s && j + 3 < jlim);
    }
  }
  if (have) {
    uint32_t* c = cnt + (int64_t)(tl.x + tid) * 3;
    if (G) atomicAdd(&c[0], G);
    if (P) atomicAdd(&c[1], P);
    if (E) atomicAdd(&c[2], E);
  }
}
void launch_cls_count(const float* col, int64_t npitch, int n, int seg, int S, int c0, const int32_t* labels, const int32_t* pos_idx,
                      const int4* tiles, int tile0, int ntiles, uint32_t* cnt, hipStream_t s) {
  hipLaunchKernelGGL(k_cls_count, dim3((unsigned)S, (unsigned)ntiles), dim3(256), 0, s, col, npitch, n, seg, c0, labels, pos_idx, tiles,
                     tile0, cnt);
}

// ---------------------------------------------------------------------------------------------- final pass
// grid (cb): class c0 + blockIdx.x, its positives pos_idx[cstart[c] .. cstart[c + 1]) in ascending item index.  Thread t sums the
// terms of positives t, t + 256, ... in that order, then a fixed tree over the 256 threads: the same bits on every call.
// apd[c]: the double quotient (vv_classification_report::mean_ap is formed from these); ap[c]: rounded once to float (:85).
__global__ __launch_bounds__(256) void k_cls_final(const float* __restrict__ col, int64_t npitch, int c0,
                                                   const int32_t* __restrict__ pos_idx, const int32_t* __restrict__ cstart,
                                                   const uint32_t* __restrict__ cnt, double* __restrict__ apd,
                                                   float* __restrict__ ap) {
  __shared__ double red[256];
  const int c = c0 + blockIdx.x, tid = threadIdx.x;
  const int b = cstart[c], e = cstart[c + 1];
  const float* key = col + (int64_t)blockIdx.x * npitch;
  double sum = 0.0;
  for (int j = b + tid; j < e; j += 256) {
    const float s = key[pos_idx[j]];
    if (s >= 0.f) {                                                 // below zero: behind the n dummies, never visited (:79)
      const uint32_t* q = cnt + (int64_t)j * 3;
      sum += (double)(q[1] + q[2] + 1u) / (double)(q[0] + q[2] + 1u);    // :81-82
    }
  }
  red[tid] = sum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const double v = e > b ? red[0] / (double)(e - b) : 0.0;        // :85, :88-89
    apd[c] = v; ap[c] = (float)v;
  }
}
void launch_cls_final(const float* col, int64_t npitch, int c0, int cb, const int32_t* pos_idx, const int32_t* cstart,
                      const uint32_t* cnt, double* apd, float* ap, hipStream_t s) {
  hipLaunchKernelGGL(k_cls_final, dim3((unsigned)cb), dim3(256), 0, s, col, npitch, c0, pos_idx, cstart, cnt, apd, ap);
}

// ---------------------------------------------------------------------------------------------- gallery scores
// vv_gallery_scores: out[r][g] = -0.5f * dist[r][g], the fp32 dot product k_sim_f32 accumulated (it stored -2 x that; both
// factors are powers of two, so the product is exact).  dist rows are `pitch` floats apart, out rows ng.
__global__ __launch_bounds__(256) void k_scores_out(const float* __restrict__ dist, int64_t pitch, int ng, float* __restrict__ out) {
  const int row = blockIdx.y;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g < ng) out[(int64_t)row * ng + g] = -0.5f * dist[(int64_t)row * pitch + g];
}
void launch_scores_out(const float* dist, int64_t pitch, int rows, int ng, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_scores_out, dim3((unsigned)((ng + 255) / 256), (unsigned)rows), dim3(256), 0, s, dist, pitch, ng, out);
}

}  // namespace vv
