// kernels_pq.hip -- product-quantised lists of the inverted-file index (include/videovec.h: vv_pq_*, vv_ivfpq_*; the entry points are
// pq.hip, the sizes are vv_pq_plan.h).  gfx950 (MI355X, CDNA4) only.  HAS NO REFERENCE COUNTERPART: the reference quantises nothing.
//
// Building: k_pq_slice cuts a sub-space's columns out of the items' rows for k-means' own assignment pass (kmeans.hip, as it stands),
// k_pq_pack writes that pass's clusters as bytes, k_pq_permute puts the code rows into list order.  Searching, per block of queries:
// the IVF probe as it stands, k_pq_lut, k_pq_scan, and k_ivf_select as it stands behind them.  Every fp32 operation of the arithmetic
// goes through pq_add / pq_mul (contraction off inside them and in this whole file), so each is rounded on its own; no floating-point
// atomic exists here, and every byte that indexes a table was written by k_pq_pack, which cuts it into 0 .. ksub - 1.
#include "vv_internal.h"

#pragma clang fp contract(off)

namespace vv {

__device__ __forceinline__ float pq_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float pq_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// ---------------------------------------------------------------------------------------------- building
// out[g][c] = feat[g][col0 + c] for c < dsub, 0 for dsub <= c < Dps.  One thread per output float.
__global__ __launch_bounds__(256) void k_pq_slice(const float* __restrict__ feat, int64_t n, int Dp, int col0, int dsub, int Dps,
                                                  float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * Dps) return;
  const int64_t g = t / Dps;
  const int c = (int)(t - g * Dps);
  out[t] = c < dsub ? feat[g * Dp + col0 + c] : 0.f;
}
void launch_pq_slice(const float* feat, int64_t n, int Dp, int col0, int dsub, int Dps, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_pq_slice, dim3((unsigned)((n * Dps + 255) / 256)), dim3(256), 0, s, feat, n, Dp, col0, dsub, Dps, out);
}

// codes[g][m] = assign[g], cut into 0 .. ksub - 1 (k-means' assignment lies there already: the cut is what lets k_pq_scan index its
// table without a check).  One thread per item.
__global__ __launch_bounds__(256) void k_pq_pack(const int32_t* __restrict__ assign, int64_t n, int m, int M, int ksub,
                                                 uint8_t* __restrict__ codes) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  codes[g * M + m] = (uint8_t)min(max(assign[g], 0), ksub - 1);
}
void launch_pq_pack(const int32_t* assign, int64_t n, int m, int M, int ksub, uint8_t* codes, hipStream_t s) {
  hipLaunchKernelGGL(k_pq_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, assign, n, m, M, ksub, codes);
}

// slab[p][m] = codes[list[p]][m]: list[] is k_km_scatter's, every entry in 0 .. n - 1.  One thread per byte.
__global__ __launch_bounds__(256) void k_pq_permute(const uint8_t* __restrict__ codes, const int32_t* __restrict__ list, int64_t n, int M,
                                                    int Mrow, uint8_t* __restrict__ slab) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * M) return;
  const int64_t p = t / M;
  const int m = (int)(t - p * M);
  slab[p * Mrow + m] = codes[(int64_t)list[p] * M + m];
}
void launch_pq_permute(const uint8_t* codes, const int32_t* list, int64_t n, int M, int Mrow, uint8_t* slab, hipStream_t s) {
  hipLaunchKernelGGL(k_pq_permute, dim3((unsigned)((n * M + 255) / 256)), dim3(256), 0, s, codes, list, n, M, Mrow, slab);
}

// ---------------------------------------------------------------------------------------------- the table
// One workgroup per PQ_LUT_ROWS = 8 consecutive query rows; thread t takes the entries t, t + 256, .. of their tables, each for all
// the workgroup's rows at once, so a codeword is read once for eight queries.  Entry m ksub + j of row i: s = +0.0f, then
// s = s + q[i][m dsub + col] * cb[m][j][col] for col = 0 .. dsub - 1, product and sum each rounded; stored as -2.0f * s + 0.0f, the
// similarity kernel's store -- a chain of its own per row and entry, whatever rows share the workgroup.  The entries from M ksub up to
// the table's pitch are written zero and never read.
constexpr int PQ_LUT_ROWS = 8;
__global__ __launch_bounds__(256) void k_pq_lut(const float* __restrict__ Q, int rows, int Dp, const float* __restrict__ cb, int M, int ksub,
                                                int dsub, float* __restrict__ lut, int64_t table) {
  const int row0 = (int)blockIdx.x * PQ_LUT_ROWS, nr = min(PQ_LUT_ROWS, rows - row0);     // (uniform over the workgroup)
  const int entries = M * ksub;
  for (int e = threadIdx.x; e < (int)table; e += 256) {
    float s[PQ_LUT_ROWS];
#pragma unroll
    for (int r = 0; r < PQ_LUT_ROWS; ++r) s[r] = 0.f;
    if (e < entries) {
      const float* w = cb + (int64_t)e * dsub;                     // cb[m][j] with e = m ksub + j
      const float* x = Q + (int64_t)row0 * Dp + (e / ksub) * dsub;
      for (int col = 0; col < dsub; ++col) {
        const float wv = w[col];
#pragma unroll
        for (int r = 0; r < PQ_LUT_ROWS; ++r)
          if (r < nr) s[r] = pq_add(s[r], pq_mul(x[(int64_t)r * Dp + col], wv));
      }
    }
#pragma unroll
    for (int r = 0; r < PQ_LUT_ROWS; ++r)
      if (r < nr) lut[(int64_t)(row0 + r) * table + e] = e < entries ? pq_add(pq_mul(-2.0f, s[r]), 0.0f) : 0.f;
  }
}
void launch_pq_lut(const float* Q, int rows, int Dp, const float* cb, int M, int ksub, int dsub, float* lut, int64_t table, hipStream_t s) {
  hipLaunchKernelGGL(k_pq_lut, dim3((unsigned)((rows + PQ_LUT_ROWS - 1) / PQ_LUT_ROWS)), dim3(256), 0, s, Q, rows, Dp, cb, M, ksub, dsub, lut, table);
}

// ---------------------------------------------------------------------------------------------- the scan
// One workgroup of 256 per query row.  Its table goes to LDS once, 16 bytes per load, laid out as it lies in scratch: [M][ksub].  (The
// lanes of a wave read the same m and whatever j their items carry, so which banks meet is the data's choice under any one-to-one
// layout; only a second copy of the table would spread them, and the largest table, 64 KiB, leaves no room for one beside a second
// workgroup on the compute unit.)  Then the probed lists p = 0 .. nprobe - 1 in turn, the lanes across a list's items 256 at a time:
// lane j reads the M code bytes of slab row start[c] + j -- FORM 1: uint4 loads (M % 16 == 0), 2: uint32 loads (M % 4 == 0), 3: bytes;
// the same bytes in the same order, so one result -- and adds the M look-ups in ascending m: acc = lut[0][code 0], then
// acc = acc + lut[m][code m].  It stores acc to cand[i pitch + off[i][p] + j]: k_sim_f32_grouped's layout, so k_ivf_select follows.
template <int FORM>
__global__ __launch_bounds__(256) void k_pq_scan(PqScan a) {
  extern __shared__ float4 slut4[];
  const float* slut = (const float*)slut4;
  const int row = blockIdx.x, tid = threadIdx.x;
  const float4* src = (const float4*)(a.lut + (int64_t)row * a.table);
  for (int i = tid; i < (int)(a.table / 4); i += 256) slut4[i] = src[i];
  __syncthreads();
  float* d = a.cand + (int64_t)row * a.pitch;
  const int M = a.M, ksub = a.ksub;
  for (int p = 0; p < a.nprobe; ++p) {                               // (uniform over the workgroup)
    const int64_t pair = (int64_t)row * a.nprobe + p;
    const int c = a.probe[pair], o = a.off[pair], s0 = a.start[c], size = a.start[c + 1] - s0;
    for (int j = tid; j < size; j += 256) {
      const uint8_t* r = a.slab + (int64_t)(s0 + j) * a.Mrow;
      float acc = 0.f;
      if (FORM == 1) {
        for (int m0 = 0; m0 < M; m0 += 16) {
          const uint4 w = *(const uint4*)(r + m0);
          const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
          for (int b = 0; b < 16; ++b) {
            const float v = slut[(m0 + b) * ksub + (int)((ww[b >> 2] >> (8 * (b & 3))) & 255u)];
            acc = m0 + b == 0 ? v : pq_add(acc, v);
          }
        }
      } else if (FORM == 2) {
        for (int m0 = 0; m0 < M; m0 += 4) {
          const uint32_t w = *(const uint32_t*)(r + m0);
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const float v = slut[(m0 + b) * ksub + (int)((w >> (8 * b)) & 255u)];
            acc = m0 + b == 0 ? v : pq_add(acc, v);
          }
        }
      } else {
        acc = slut[r[0]];
        for (int m = 1; m < M; ++m) acc = pq_add(acc, slut[m * ksub + r[m]]);
      }
      d[o + j] = acc;
    }
  }
}
void launch_pq_scan(const PqScan& a, int form, hipStream_t s) {
  const size_t lds = (size_t)a.table * 4;
  if (form == 1) hipLaunchKernelGGL(k_pq_scan<1>, dim3((unsigned)a.rows), dim3(256), lds, s, a);
  else if (form == 2) hipLaunchKernelGGL(k_pq_scan<2>, dim3((unsigned)a.rows), dim3(256), lds, s, a);
  else hipLaunchKernelGGL(k_pq_scan<3>, dim3((unsigned)a.rows), dim3(256), lds, s, a);
}

}  // namespace vv
