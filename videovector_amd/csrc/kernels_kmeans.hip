// kernels_kmeans.hip -- k-means on a gallery (include/videovec.h: vv_gallery_kmeans; the entry point is kmeans.hip, the sizes are
// vv_kmeans_plan.h).  gfx950 (MI355X, CDNA4) only.  HAS NO REFERENCE COUNTERPART: the reference has no clustering.
//
// One pass = the similarity of a block of items against the centroids (k_sim_f32, kernels_retrieval.hip, as it stands), k_km_assign on
// the block, and after the last block k_km_fold.  One update = the grouping (k_km_hist, k_km_starts, k_km_scan, k_km_scatter: a
// stable counting sort of the items by cluster), k_km_partial and k_km_finish.  Every fp32 operation of the arithmetic goes through
// km_add / km_mul / km_div below (contraction off inside them and in this whole file) or sqrtf, so each is rounded on its own; no
// floating-point atomic exists here, and every sum has ONE order that depends on item indices alone -- never on the block plan, the grid or the dispatch order.
#include "vv_internal.h"

#pragma clang fp contract(off)

namespace vv {

// One rounding each, never fused with a neighbour (the toolchain's __fadd_rn / __fmul_rn are plain operators compiled where contraction
// is allowed, and its __fsqrt_rn is the native instruction: neither is used).  Division and sqrtf are the correctly rounded ones.
__device__ __forceinline__ float km_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float km_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float km_div(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}

// (key, cluster) ascending: the order vv_gallery_topk gives (d, g).  A NaN key is below nothing, so it is never selected.
__device__ inline bool km_less(float k2, int c2, float k, int c) { return k2 < k || (k2 == k && c2 < c); }

// ---------------------------------------------------------------------------------------------- initial centroids
// cent[c] = feat[rows[c]] over all Dp columns (the padding is zero in both).  grid (C).
__global__ __launch_bounds__(256) void k_km_gather(const float* __restrict__ feat, int Dp, const int32_t* __restrict__ rows,
                                                   float* __restrict__ cent) {
  const float4* src = (const float4*)(feat + (int64_t)rows[blockIdx.x] * Dp);
  float4* dst = (float4*)(cent + (int64_t)blockIdx.x * Dp);
  for (int i = threadIdx.x; i < Dp / 4; i += 256) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------------- assignment
// One workgroup per KM_SLOT_ROWS = 64 consecutive items, wave w rows 16 w .. 16 w + 15 one after the other, the lanes across the row's
// C scores: VEC 16 bytes per lane (score base on 16 bytes, C % 4 == 0), else one float per lane.  A lane keeps the smallest (key, c) it
// saw, the wave folds the 64 by km_less: a total order on the keys that are not NaN, so the row's minimum is the same whatever lane saw
// which column -- both forms, one result.  No key selected (every key NaN): cluster 0 with its key.
// score: the block's rows, C floats apart; row0: the block's first item; rows: its items.  assign: in -- the previous pass's cluster
// (-1 before the first), out -- this one's.  counts [C]: integer atomics.  slot [ceil(n / 64)]: the workgroup's 64 selected keys as
// doubles (absent rows +0.0) folded by x[i] += x[i + o], o = 32 .. 1, in item order.  moved / nonfinite: the pass's record.
template <bool VEC, bool EUCLID>
__global__ __launch_bounds__(256) void k_km_assign(const float* __restrict__ score, int C, int64_t row0, int rows,
                                                   const float* __restrict__ nn, int32_t* __restrict__ assign,
                                                   int32_t* __restrict__ counts, double* __restrict__ slot, KmRec* __restrict__ rec) {
  __shared__ __attribute__((aligned(16))) float snn[KM_MAX_CLUSTERS];
  __shared__ int shist[KM_MAX_CLUSTERS];
  __shared__ double skey[KM_SLOT_ROWS];
  __shared__ int smoved, sbad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = tid; c < C; c += 256) { shist[c] = 0; if (EUCLID) snn[c] = nn[c]; }
  if (tid < KM_SLOT_ROWS) skey[tid] = 0.0;
  if (tid == 0) { smoved = 0; sbad = 0; }
  __syncthreads();
  const int r_base = (int)blockIdx.x * KM_SLOT_ROWS + wave * 16;
  for (int rr = 0; rr < 16; ++rr) {
    const int r = r_base + rr;                                   // (uniform in the wave)
    if (r >= rows) break;
    const float* srow = score + (int64_t)r * C;
    float bk = __builtin_inff(); int bc = 0x7fffffff;
    if (VEC) {
      for (int c4 = lane; c4 < C / 4; c4 += 64) {
        const float4 d = *(const float4*)(srow + c4 * 4);
        float k0 = d.x, k1 = d.y, k2 = d.z, k3 = d.w;
        if (EUCLID) {
          const float4 q = *(const float4*)&snn[c4 * 4];
          k0 = km_add(d.x, q.x); k1 = km_add(d.y, q.y); k2 = km_add(d.z, q.z); k3 = km_add(d.w, q.w);
        }
        if (km_less(k0, c4 * 4, bk, bc)) { bk = k0; bc = c4 * 4; }
        if (km_less(k1, c4 * 4 + 1, bk, bc)) { bk = k1; bc = c4 * 4 + 1; }
        if (km_less(k2, c4 * 4 + 2, bk, bc)) { bk = k2; bc = c4 * 4 + 2; }
        if (km_less(k3, c4 * 4 + 3, bk, bc)) { bk = k3; bc = c4 * 4 + 3; }
      }
    } else {
      for (int c = lane; c < C; c += 64) {
        float k = srow[c];
        if (EUCLID) k = km_add(k, snn[c]);
        if (km_less(k, c, bk, bc)) { bk = k; bc = c; }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ok = __shfl_xor(bk, o, 64); const int oc = __shfl_xor(bc, o, 64);
      if (km_less(ok, oc, bk, bc)) { bk = ok; bc = oc; }
    }
    if (lane == 0) {
      if (bc == 0x7fffffff) { bc = 0; bk = EUCLID ? km_add(srow[0], snn[0]) : srow[0]; }
      const int64_t i = row0 + r;
      if (assign[i] != bc) atomicAdd(&smoved, 1);
      assign[i] = bc;
      atomicAdd(&shist[bc], 1);
      if (!(fabsf(bk) < __builtin_inff())) atomicAdd(&sbad, 1);
      skey[r - (int)blockIdx.x * KM_SLOT_ROWS] = (double)bk;
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) { const int h = shist[c]; if (h) atomicAdd(&counts[c], h); }
  if (wave == 0) {
    double v = skey[lane];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) {
      slot[(row0 + (int64_t)blockIdx.x * KM_SLOT_ROWS) / KM_SLOT_ROWS] = v;
      if (smoved) atomicAdd((unsigned long long*)&rec->moved, (unsigned long long)smoved);
      if (sbad) atomicAdd((unsigned long long*)&rec->nonfinite, (unsigned long long)sbad);
    }
  }
}

int launch_km_assign(const float* score, int C, int64_t row0, int rows, int euclid, const float* nn, int32_t* assign, int32_t* counts,
                     double* slot, KmRec* rec, hipStream_t s) {
  const bool vec = ((uintptr_t)score & 15) == 0 && C % 4 == 0;
  const dim3 grid((unsigned)((rows + KM_SLOT_ROWS - 1) / KM_SLOT_ROWS)), wg(256);
#define KM_GO(V, E) hipLaunchKernelGGL((k_km_assign<V, E>), grid, wg, 0, s, score, C, row0, rows, nn, assign, counts, slot, rec)
  if (vec) { if (euclid) KM_GO(true, true); else KM_GO(true, false); }
  else { if (euclid) KM_GO(false, true); else KM_GO(false, false); }
#undef KM_GO
  return vec ? 1 : 2;
}

// the pass's objective: the slots in ascending index, one after the other from +0.0 -- one thread, eight loads ahead of the chain
__global__ void k_km_fold(const double* __restrict__ slot, int64_t slots, KmRec* __restrict__ rec) {
  double acc = 0.0;
  int64_t i = 0;
  for (; i + 8 <= slots; i += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = slot[i + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; i < slots; ++i) acc += slot[i];
  rec->objective = acc;
}
void launch_km_fold(const double* slot, int64_t slots, KmRec* rec, hipStream_t s) {
  hipLaunchKernelGGL(k_km_fold, dim3(1), dim3(1), 0, s, slot, slots, rec);
}

// ---------------------------------------------------------------------------------------------- grouping
// A stable counting sort of the items by cluster: list holds every cluster's items in ascending item index, cluster c's at
// start[c] .. start[c + 1] - 1, whatever order the workgroups run in.
//   k_km_hist     hist[tile][c] = the items of tile `tile` (KM_TILE consecutive items) in cluster c
//   k_km_starts   start = the exclusive sums of counts; the chunk table -- cluster c's list cut into chunks of KM_CHUNK entries
//   k_km_scan     hist[tile][c] <- start[c] + the items of cluster c in the tiles before `tile`: where the tile's first item of c goes
//   k_km_scatter  one wave per tile walks its items 64 at a time in ascending index; an item's place is its cluster's running base plus
//                 the lanes below it that hold the same cluster
__global__ __launch_bounds__(256) void k_km_hist(const int32_t* __restrict__ assign, int64_t n, int C, int32_t* __restrict__ hist) {
  __shared__ int sh[KM_MAX_CLUSTERS];
  const int tid = threadIdx.x;
  for (int c = tid; c < C; c += 256) sh[c] = 0;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * KM_TILE;
  for (int j = tid; j < KM_TILE; j += 256) {
    const int64_t i = i0 + j;
    if (i < n) { const uint32_t c = (uint32_t)assign[i]; if (c < (uint32_t)C) atomicAdd(&sh[c], 1); }
  }
  __syncthreads();
  int32_t* out = hist + (int64_t)blockIdx.x * C;
  for (int c = tid; c < C; c += 256) out[c] = sh[c];
}

// one workgroup.  Thread t owns the clusters t P .. t P + P - 1, P = ceil(C / 256).  start [C + 1]; cbase [C + 1]: the first chunk
// of every cluster; chunks[k] = {cluster, first list position, entries (1 .. KM_CHUNK), 0}; rec->chunks = their number.
__global__ __launch_bounds__(256) void k_km_starts(const int32_t* __restrict__ counts, int C, int32_t* __restrict__ start,
                                                   int32_t* __restrict__ cbase, int4* __restrict__ chunks, int64_t max_chunks,
                                                   int32_t* __restrict__ nchunks, KmRec* __restrict__ rec) {
  __shared__ int s_items[256], s_chunks[256];
  const int tid = threadIdx.x, per = (C + 255) / 256, c0 = min(C, tid * per), c1 = min(C, c0 + per);
  int items = 0, nch = 0;
  for (int c = c0; c < c1; ++c) { const int k = counts[c]; items += k; nch += (k + KM_CHUNK - 1) / KM_CHUNK; }
  s_items[tid] = items; s_chunks[tid] = nch;
  __syncthreads();
  int bi = 0, bc = 0;                                            // (integers: any order)
  for (int t = 0; t < tid; ++t) { bi += s_items[t]; bc += s_chunks[t]; }
  for (int c = c0; c < c1; ++c) {
    const int k = counts[c], m = (k + KM_CHUNK - 1) / KM_CHUNK;
    start[c] = bi; cbase[c] = bc;
    for (int j = 0; j < m; ++j)
      if (bc + j < max_chunks) chunks[bc + j] = make_int4(c, bi + j * KM_CHUNK, min(KM_CHUNK, k - j * KM_CHUNK), 0);
    bi += k; bc += m;
  }
  if (tid == 255) { start[C] = bi; cbase[C] = bc; *nchunks = (int32_t)min((int64_t)bc, max_chunks); rec->chunks = bc; }
}

// thread per cluster, the tiles in ascending order
__global__ __launch_bounds__(64) void k_km_scan(int32_t* __restrict__ hist, int64_t tiles, int C, const int32_t* __restrict__ start) {
  const int c = (int)blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  int run = start[c];
  int64_t t = 0;
  for (; t + 8 <= tiles; t += 8) {
    int h[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) h[u] = hist[(t + u) * C + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) { hist[(t + u) * C + c] = run; run += h[u]; }
  }
  for (; t < tiles; ++t) { const int h = hist[t * C + c]; hist[t * C + c] = run; run += h; }
}

// one wave per tile
__global__ __launch_bounds__(64) void k_km_scatter(const int32_t* __restrict__ assign, int64_t n, int C,
                                                   const int32_t* __restrict__ hist, int32_t* __restrict__ list) {
  __shared__ int sbase[KM_MAX_CLUSTERS];
  const int lane = threadIdx.x;
  const int32_t* base = hist + (int64_t)blockIdx.x * C;
  for (int c = lane; c < C; c += 64) sbase[c] = base[c];
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * KM_TILE;
  for (int j0 = 0; j0 < KM_TILE; j0 += 64) {
    const int64_t i = i0 + j0 + lane;
    if (i0 + j0 >= n) break;                                     // (uniform)
    int c = -1;
    if (i < n) { c = assign[i]; if ((uint32_t)c >= (uint32_t)C) c = -1; }
    unsigned long long todo = __ballot(c >= 0);
    while (todo) {                                               // (uniform: one round per distinct cluster among the 64)
      const int leader = __ffsll((long long)todo) - 1;
      const int cl = __shfl(c, leader, 64);
      const unsigned long long m = __ballot(c == cl);
      const int b = sbase[cl];
      __syncthreads();                                           // (every lane has read the base before the leader moves it)
      if (c == cl) {
        const int64_t pos = (int64_t)b + __popcll(m & ((1ull << lane) - 1ull));
        if (pos < n) list[pos] = (int32_t)i;
      }
      if (lane == leader) sbase[cl] = b + __popcll(m);
      __syncthreads();
      todo &= ~m;
    }
  }
}

void launch_km_group(const int32_t* assign, int64_t n, int C, int64_t tiles, const int32_t* counts, int32_t* hist, int32_t* start,
                     int32_t* cbase, int4* chunks, int64_t max_chunks, int32_t* nchunks, int32_t* list, KmRec* rec, hipStream_t s) {
  hipLaunchKernelGGL(k_km_hist, dim3((unsigned)tiles), dim3(256), 0, s, assign, n, C, hist);
  hipLaunchKernelGGL(k_km_starts, dim3(1), dim3(256), 0, s, counts, C, start, cbase, chunks, max_chunks, nchunks, rec);
  hipLaunchKernelGGL(k_km_scan, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, s, hist, tiles, C, (const int32_t*)start);
  hipLaunchKernelGGL(k_km_scatter, dim3((unsigned)tiles), dim3(64), 0, s, assign, n, C, (const int32_t*)hist, list);
}

// ---------------------------------------------------------------------------------------------- centroid sums
// One workgroup per (chunk, slice of KM_SLICE columns), 16 bytes per thread: the chunk's first row is stored, then acc = acc + x over
// its other rows in list order.  grid (max_chunks, slices); the workgroups past *nchunks leave.  part [max_chunks][Dp].
// (every index read from memory is cut to the arrays' bounds: n items, KM_CHUNK entries)
__global__ __launch_bounds__(128) void k_km_partial(const float* __restrict__ feat, int64_t n, int Dp, const int32_t* __restrict__ list,
                                                    const int4* __restrict__ chunks, const int32_t* __restrict__ nchunks,
                                                    float* __restrict__ part) {
  __shared__ int sidx[KM_CHUNK];
  if ((int)blockIdx.x >= *nchunks) return;
  const int4 ch = chunks[blockIdx.x];
  const int tid = threadIdx.x, len = max(1, min(ch.z, KM_CHUNK));
  for (int j = tid; j < len; j += 128) {
    const int64_t pos = min(max((int64_t)ch.y + j, (int64_t)0), n - 1);
    sidx[j] = (int)min(max((int64_t)list[pos], (int64_t)0), n - 1);
  }
  __syncthreads();
  const int col = (int)blockIdx.y * KM_SLICE + tid * 4;
  if (col >= Dp) return;
  const float* src = feat + col;
  float4 acc = *(const float4*)(src + (int64_t)sidx[0] * Dp);
  int j = 1;
  for (; j + 4 <= len; j += 4) {
    const float4 x0 = *(const float4*)(src + (int64_t)sidx[j] * Dp), x1 = *(const float4*)(src + (int64_t)sidx[j + 1] * Dp),
                 x2 = *(const float4*)(src + (int64_t)sidx[j + 2] * Dp), x3 = *(const float4*)(src + (int64_t)sidx[j + 3] * Dp);
    acc.x = km_add(km_add(km_add(km_add(acc.x, x0.x), x1.x), x2.x), x3.x);
    acc.y = km_add(km_add(km_add(km_add(acc.y, x0.y), x1.y), x2.y), x3.y);
    acc.z = km_add(km_add(km_add(km_add(acc.z, x0.z), x1.z), x2.z), x3.z);
    acc.w = km_add(km_add(km_add(km_add(acc.w, x0.w), x1.w), x2.w), x3.w);
  }
  for (; j < len; ++j) {
    const float4 x = *(const float4*)(src + (int64_t)sidx[j] * Dp);
    acc.x = km_add(acc.x, x.x); acc.y = km_add(acc.y, x.y); acc.z = km_add(acc.z, x.z); acc.w = km_add(acc.w, x.w);
  }
  *(float4*)(part + (int64_t)blockIdx.x * Dp + col) = acc;
}
void launch_km_partial(const float* feat, int64_t n, int Dp, const int32_t* list, const int4* chunks, const int32_t* nchunks, int64_t max_chunks,
                       int slices, float* part, hipStream_t s) {
  hipLaunchKernelGGL(k_km_partial, dim3((unsigned)max_chunks, (unsigned)slices), dim3(128), 0, s, feat, n, Dp, list, chunks, nchunks, part);
}

// One workgroup per cluster.  s = the cluster's partials added in ascending chunk order, starting from the first.  EUCLIDEAN:
// centroid = s * (1.0f / (float)count).  SPHERICAL: q = the chain of s[col]^2 in ascending column from +0, centroid = s / sqrtf(q); q
// zero or not finite: the previous centroid stays (degenerate).  No item: the previous centroid stays (empty).  Then nn = the chain of
// centroid[col]^2 in ascending column from +0 (EUCLIDEAN only; a row that stayed gives the value it had).  init: the rows are the
// initial centroids -- nothing is summed or counted, only nn is written.
__global__ __launch_bounds__(256) void k_km_finish(const float* __restrict__ part, int Dp, int dim, const int32_t* __restrict__ counts,
                                                   const int32_t* __restrict__ cbase, int64_t max_chunks, int euclid, int init,
                                                   float* __restrict__ cent, float* __restrict__ nn, KmRec* __restrict__ rec) {
  __shared__ float srow[8192];                                    // (vv_gallery_create: dim <= 8192, so Dp <= 8192)
  __shared__ float sq;
  const int c = blockIdx.x, tid = threadIdx.x;
  float* crow = cent + (int64_t)c * Dp;
  const int count = init ? 0 : counts[c];
  bool keep = init || count == 0;
  if (!keep) {
    const int k0 = (int)min((int64_t)cbase[c], max_chunks - 1), k1 = (int)min((int64_t)cbase[c + 1], max_chunks);
    for (int col = tid; col < Dp; col += 256) {
      float s = part[(int64_t)k0 * Dp + col];
      for (int k = k0 + 1; k < k1; ++k) s = km_add(s, part[(int64_t)k * Dp + col]);
      srow[col] = s;
    }
    __syncthreads();
    if (euclid) {
      const float inv = km_div(1.0f, (float)count);
      for (int col = tid; col < Dp; col += 256) crow[col] = km_mul(srow[col], inv);
    } else {
      if (tid == 0) {
        float q = 0.f;
        for (int col = 0; col < dim; ++col) q = km_add(q, km_mul(srow[col], srow[col]));
        sq = q;
      }
      __syncthreads();
      const float q = sq;
      if (q == 0.f || !(fabsf(q) < __builtin_inff())) {
        keep = true;                                              // (uniform)
        if (tid == 0) atomicAdd(&rec->degenerate, 1);
      } else {
        const float nrm = sqrtf(q);                                // (the correctly rounded one; __fsqrt_rn is the native instruction here)
        for (int col = tid; col < Dp; col += 256) crow[col] = km_div(srow[col], nrm);
      }
    }
  } else if (!init && tid == 0) {
    atomicAdd(&rec->empty, 1);
  }
  if (!euclid) return;
  if (keep && !init) return;                                      // the row and its nn stay bit for bit
  __syncthreads();                                                // (this workgroup's stores to crow, read back below by thread 0)
  if (tid == 0) {
    float q = 0.f;
    for (int col = 0; col < dim; ++col) { const float v = init ? crow[col] : km_mul(srow[col], km_div(1.0f, (float)count)); q = km_add(q, km_mul(v, v)); }
    nn[c] = q;
  }
}
void launch_km_finish(const float* part, int Dp, int dim, const int32_t* counts, const int32_t* cbase, int64_t max_chunks, int C, int euclid, int init,
                      float* cent, float* nn, KmRec* rec, hipStream_t s) {
  hipLaunchKernelGGL(k_km_finish, dim3((unsigned)C), dim3(256), 0, s, part, Dp, dim, counts, cbase, max_chunks, euclid, init, cent, nn, rec);
}
void launch_km_gather(const float* feat, int Dp, const int32_t* rows, int C, float* cent, hipStream_t s) {
  hipLaunchKernelGGL(k_km_gather, dim3((unsigned)C), dim3(256), 0, s, feat, Dp, rows, cent);
}

}  // namespace vv
