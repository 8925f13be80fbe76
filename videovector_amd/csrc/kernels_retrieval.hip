// kernels_retrieval.hip -- gallery retrieval: fp32 similarity, streaming top-k, sort-free rank statistics and nearest-neighbour
// lists of up to RT_CHUNK items by radix selection.
// gfx950 (MI355X, CDNA4) only.  Replaces the hot path of RetrievalRankStatsFixedRefLayer::Forward_cpu
// (src/caffe/layers/retrieval_rank_stats_fixed_ref_layer.cpp:142-171): the -2 Q R^T product (:142-144), the full
// std::sort of every query's row (:158-162) and the walk over the sorted row in ComputeApStats (:62-118).
//
// Form (DESIGN.md 'Gallery retrieval'): one QUERY BLOCK at a time.  k_sim_f32 writes the block's distances
// d[q][g] = -2 dot(q, r_g) into a scratch buffer of at most 1 GiB; the row kernels below read that buffer.  A positive's
// key and the key the counting pass sees for the same pair are therefore the SAME stored float: no second evaluation
// of a dot product exists whose summation order could differ.
//
// Order: every (distance, gallery index) pair becomes one 64-bit key, ascending in (d, g): the distance's bits mapped
// to an unsigned integer of the same order in the high word, the index in the low word.  Keys of one query are distinct,
// so "the rank of p" is 1 + the number of keys below p's.  -0.0f is folded into +0.0f when the distance is stored
// (operator< of the reference's comparator calls them equal).
#include "vv_internal.h"
#include "vv_rt_device.h"

namespace vv {

// ---------------------------------------------------------------------------------------------- similarity
// The tile (128 x 128 outputs per 256-thread workgroup, K 32 at a time, its fixed K order) is vv_rt_device.h's rt_tile_mma: the kernels
// here choose the rows and store the result.  Q [nq][Dp], G [ng][Dp] row-major, Dp a multiple of 32 with zero padding; out [nq][pitch].

// ROWS: query row i is Q + rowidx[i] * Dp (the linear classifier on a row list, linear.hip) instead of Q + i * Dp; the clamp below is
// then on the LIST POSITION, so no index past rowidx[nq - 1] is read.  Everything after the eight row pointers is the same code, so
// out (i, c) has the bits the contiguous form gives for the same row values.
template <bool ROWS>
__global__ __launch_bounds__(256) void k_sim_f32_t(const float* __restrict__ Q, const float* __restrict__ G,
                                                   float* __restrict__ out, int nq, int ng, int Dp, int64_t pitch,
                                                   int mtiles, const int32_t* __restrict__ rowidx) {
  __shared__ __attribute__((aligned(16))) float sA[RT_BM * RT_LD];
  __shared__ __attribute__((aligned(16))) float sB[RT_BN * RT_LD];
  // query tiles fastest: the workgroups that share a gallery tile run together, so the gallery comes from HBM once per block
  const int m0 = (int)(blockIdx.x % mtiles) * RT_BM, n0 = (int)(blockIdx.x / mtiles) * RT_BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;

  // thread t stages float4 (t & 7) of rows (t >> 3) + 32 i, i = 0..3, of both tiles.  Rows past the end repeat the last one; they are
  // never stored.
  const int srow = tid >> 3, c4 = tid & 7;
#define RT_ROWPTR(M, base, i, n) ((const float4*)((M) + (int64_t)min((base) + srow + 32 * (i), (n)-1) * Dp) + c4)
#define RT_LISTPTR(i) ((const float4*)(Q + (int64_t)rowidx[min(m0 + srow + 32 * (i), nq - 1)] * Dp) + c4)
  const float4 *ga0, *ga1, *ga2, *ga3;
  if constexpr (ROWS) { ga0 = RT_LISTPTR(0); ga1 = RT_LISTPTR(1); ga2 = RT_LISTPTR(2); ga3 = RT_LISTPTR(3); }
  else { ga0 = RT_ROWPTR(Q, m0, 0, nq); ga1 = RT_ROWPTR(Q, m0, 1, nq); ga2 = RT_ROWPTR(Q, m0, 2, nq); ga3 = RT_ROWPTR(Q, m0, 3, nq); }
#undef RT_LISTPTR
  const float4 *gb0 = RT_ROWPTR(G, n0, 0, ng), *gb1 = RT_ROWPTR(G, n0, 1, ng), *gb2 = RT_ROWPTR(G, n0, 2, ng),
               *gb3 = RT_ROWPTR(G, n0, 3, ng);
#undef RT_ROWPTR
  f32x16 acc[2][2];
  rt_tile_mma(ga0, ga1, ga2, ga3, gb0, gb1, gb2, gb3, Dp, sA, sB, acc);
  // C/D map of the 32x32 MFMA: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int g = n0 + wn * 64 + b * 32 + r;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int q = m0 + wm * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (q < nq && g < ng) out[(int64_t)q * pitch + g] = -2.0f * acc[a][b][e] + 0.0f;      // :142-144; -0 -> +0
      }
    }
}

constexpr auto k_sim_f32 = k_sim_f32_t<false>;              // the contiguous form: what every gallery call has always launched (rowidx is never read)
constexpr auto k_sim_f32_rows = k_sim_f32_t<true>;

void launch_sim_f32(const float* Q, const float* G, float* out, int nq, int ng, int Dp, int64_t pitch, hipStream_t s) {
  const int mtiles = (nq + RT_BM - 1) / RT_BM, ntiles = (ng + RT_BN - 1) / RT_BN;
  hipLaunchKernelGGL(k_sim_f32, dim3((unsigned)(mtiles * ntiles)), dim3(256), 0, s, Q, G, out, nq, ng, Dp, pitch, mtiles, (const int32_t*)nullptr);
}
// rowidx: device [nq], every entry a row of Q (checked on the host by the caller: nothing here can test it)
void launch_sim_f32_rows(const float* Q, const int32_t* rowidx, const float* G, float* out, int nq, int ng, int Dp, int64_t pitch, hipStream_t s) {
  const int mtiles = (nq + RT_BM - 1) / RT_BM, ntiles = (ng + RT_BN - 1) / RT_BN;
  hipLaunchKernelGGL(k_sim_f32_rows, dim3((unsigned)(mtiles * ntiles)), dim3(256), 0, s, Q, G, out, nq, ng, Dp, pitch, mtiles, rowidx);
}

// ---------------------------------------------------------------------------------------------- keys
// (rt_word / rt_key / rt_key_dist / RT_NOKEY: vv_rt_device.h)
// sk[0 .. npad), npad a power of two, ascending; a 256-thread workgroup, every thread calls it (after a barrier behind the stores)
__device__ inline void rt_bitonic(uint64_t* sk, int npad) {
  for (int k2 = 2; k2 <= npad; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < npad; i += 256) {
        const int x = i ^ j;
        if (x > i) {
          const uint64_t a = sk[i], b = sk[x];
          if ((a > b) == ((i & k2) == 0)) { sk[i] = b; sk[x] = a; }
        }
      }
      __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------- top-k
// (rt_insert / rt_offer, the wave's sorted list of the k smallest keys: vv_rt_device.h)

// grid (S, rows): workgroup (s, row) scans gallery items [s seg, (s+1) seg) of the row, part[row][s][k] = its k smallest keys.
// OTHER_ID: only items whose id differs from the row's own (own[row]; own = ids + q0 where the rows are gallery items q0 ..) are
// offered: "the nearest items of other videos" of RetrievalStatsLayer (retrieval_stats_layer.cpp:310-316).
// NOT_SELF: the rows are gallery items q0 .., and item q0 + row is not offered to its own row (vv_gallery_nearest_self).
template <bool OTHER_ID, bool NOT_SELF = false>
__global__ __launch_bounds__(256) void k_topk_part(const float* __restrict__ dist, int64_t pitch, int ng, int k, int seg,
                                                   const int32_t* __restrict__ ids, const int32_t* __restrict__ own, int q0,
                                                   uint64_t* __restrict__ part) {
  __shared__ uint64_t sl[4][32];
  const int row = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int begin = s * seg, end = min(ng, begin + seg);
  const float* d = dist + (int64_t)row * pitch;
  int32_t oid = 0;
  if (OTHER_ID) oid = own[row];
  const int self = q0 + row;
  uint64_t mine = RT_NOKEY, kth = RT_NOKEY;
  for (int base = begin; base < end; base += 1024) {               // seg is a multiple of 1024, pitch of 4
    const int i = base + tid * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < end) v = *(const float4*)(d + i);                      // i + 3 < pitch: the row's pad may be read, never ranked
    bool c0 = i < end, c1 = i + 1 < end, c2 = i + 2 < end, c3 = i + 3 < end;
    if (OTHER_ID) {                                                // (ids has ng entries: every read is guarded)
      c0 = c0 && ids[i] != oid; c1 = c1 && ids[i + 1] != oid; c2 = c2 && ids[i + 2] != oid; c3 = c3 && ids[i + 3] != oid;
    }
    if (NOT_SELF) { c0 = c0 && i != self; c1 = c1 && i + 1 != self; c2 = c2 && i + 2 != self; c3 = c3 && i + 3 != self; }
    rt_offer(rt_key(v.x, (uint32_t)i), c0, mine, kth, lane, k);
    rt_offer(rt_key(v.y, (uint32_t)i + 1), c1, mine, kth, lane, k);
    rt_offer(rt_key(v.z, (uint32_t)i + 2), c2, mine, kth, lane, k);
    rt_offer(rt_key(v.w, (uint32_t)i + 3), c3, mine, kth, lane, k);
  }
  if (lane < 32) sl[wave][lane] = mine;
  __syncthreads();
  if (wave == 0) {
    for (int w = 1; w < 4; ++w)
      for (int j = 0; j < k; ++j) rt_insert(sl[w][j], mine, lane, k);
    if (lane < k) part[((int64_t)row * gridDim.x + s) * k + lane] = mine;
  }
}
// one wave per row: the k smallest of the row's S partial lists
__global__ __launch_bounds__(64) void k_topk_merge(const uint64_t* __restrict__ part, int S, int k, int32_t* __restrict__ idx,
                                                   float* __restrict__ dst) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const uint64_t* p = part + (int64_t)row * S * k;
  uint64_t mine = RT_NOKEY, kth = RT_NOKEY;
  for (int base = 0; base < S * k; base += 64) {
    const int i = base + lane;
    const uint64_t key = i < S * k ? p[i] : RT_NOKEY;
    rt_offer(key, key != RT_NOKEY, mine, kth, lane, k);
  }
  if (lane < k) {
    idx[(int64_t)row * k + lane] = mine == RT_NOKEY ? -1 : (int32_t)(uint32_t)mine;
    dst[(int64_t)row * k + lane] = mine == RT_NOKEY ? 0.f : rt_key_dist(mine);
  }
}
void launch_topk(const float* dist, int64_t pitch, int rows, int ng, int k, int seg, int S, uint64_t* part, int32_t* idx,
                 float* dst, hipStream_t s) {
  hipLaunchKernelGGL(k_topk_part<false>, dim3(S, rows), dim3(256), 0, s, dist, pitch, ng, k, seg, (const int32_t*)nullptr,
                     (const int32_t*)nullptr, 0, part);
  hipLaunchKernelGGL(k_topk_merge, dim3(rows), dim3(64), 0, s, part, S, k, idx, dst);
}
void launch_topk_other_id(const float* dist, int64_t pitch, int rows, int ng, int k, int seg, int S, const int32_t* ids, int q0,
                          uint64_t* part, int32_t* idx, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(k_topk_part<true>, dim3(S, rows), dim3(256), 0, s, dist, pitch, ng, k, seg, ids, ids + q0, q0, part);
  hipLaunchKernelGGL(k_topk_merge, dim3(rows), dim3(64), 0, s, part, S, k, idx, dst);
}
// The streaming form of vv_gallery_nearest*: own != NULL: row r is offered only the items whose id differs from own[r];
// self0 >= 0: the rows are gallery items self0 .., none is offered to itself.
void launch_topk_eligible(const float* dist, int64_t pitch, int rows, int ng, int k, int seg, int S, const int32_t* ids,
                          const int32_t* own, int self0, uint64_t* part, int32_t* idx, float* dst, hipStream_t s) {
  const dim3 grid(S, rows), wg(256);
  const int q0 = self0 < 0 ? 0 : self0;
  if (own && self0 >= 0) hipLaunchKernelGGL((k_topk_part<true, true>), grid, wg, 0, s, dist, pitch, ng, k, seg, ids, own, q0, part);
  else if (own) hipLaunchKernelGGL((k_topk_part<true, false>), grid, wg, 0, s, dist, pitch, ng, k, seg, ids, own, q0, part);
  else if (self0 >= 0) hipLaunchKernelGGL((k_topk_part<false, true>), grid, wg, 0, s, dist, pitch, ng, k, seg, ids, own, q0, part);
  else hipLaunchKernelGGL((k_topk_part<false, false>), grid, wg, 0, s, dist, pitch, ng, k, seg, ids, own, q0, part);
  hipLaunchKernelGGL(k_topk_merge, dim3(rows), dim3(64), 0, s, part, S, k, idx, dst);
}

// ---------------------------------------------------------------------------------------------- rank statistics
// The positives of query `row` are pos_idx[pstart[row] .. + pcount[row]) (gallery indices of the query's id).  A pass takes
// RT_CHUNK of them: their keys go to LDS, sorted.  Returns how many this pass holds (0: nothing to do); *npad = the power of
// two the sorted array was padded to with RT_NOKEY.
__device__ inline int rt_load_sorted(uint64_t* sk, const float* d, const int32_t* pos_idx, int pstart, int pcount, int pass,
                                     int* npad_out) {
  const int off = pass * RT_CHUNK;
  if (off >= pcount) return 0;
  const int n = min(RT_CHUNK, pcount - off);
  int npad = 1;
  while (npad < n) npad <<= 1;
  for (int j = threadIdx.x; j < npad; j += 256) {
    uint64_t key = RT_NOKEY;
    if (j < n) { const int g = pos_idx[pstart + off + j]; key = rt_key(d[g], (uint32_t)g); }
    sk[j] = key;
  }
  __syncthreads();
  rt_bitonic(sk, npad);
  *npad_out = npad;
  return n;
}

// grid (S, rows).  Every gallery key of the segment at or below the pass's largest positive key is counted into the bin of
// its slot among the sorted positives (slot = number of positive keys below it).  bins[row][0][slot]: all items;
// bins[row][1][slot]: items that are themselves positives of the query -- needed only when the positives span several
// passes (then a positive's ordinal among ALL positives is not its index in this pass's sorted chunk).
__global__ __launch_bounds__(256) void k_rank_count(const float* __restrict__ dist, int64_t pitch, int ng, int seg,
                                                    const int32_t* __restrict__ pos_idx, const int32_t* __restrict__ pstart,
                                                    const int32_t* __restrict__ pcount, const int32_t* __restrict__ q_ids,
                                                    const int32_t* __restrict__ ref_ids, int pass, uint32_t* __restrict__ bins) {
  __shared__ uint64_t sk[RT_CHUNK];
  __shared__ uint32_t sb[2][RT_CHUNK];
  const int row = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
  const float* d = dist + (int64_t)row * pitch;
  const int P = pcount[row];
  int npad = 0;
  const int n = rt_load_sorted(sk, d, pos_idx, pstart[row], P, pass, &npad);        // uniform over the workgroup
  if (n == 0) return;
  for (int j = tid; j < n; j += 256) { sb[0][j] = 0; sb[1][j] = 0; }
  __syncthreads();
  const bool multi = P > RT_CHUNK;
  const int32_t qid = q_ids[row];
  const uint64_t last = sk[n - 1];
  const int begin = s * seg, end = min(ng, begin + seg);
  for (int base = begin; base < end; base += 1024) {
    const int i = base + tid * 4;
    if (i >= end) continue;
    const float4 v = *(const float4*)(d + i);
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint64_t key = rt_key(e[u], (uint32_t)(i + u));
      if (i + u >= end || key > last) continue;
      int slot = 0;
      for (int step = npad >> 1; step > 0; step >>= 1)
        if (sk[slot + step - 1] < key) slot += step;                // key <= last, so the answer is at most n - 1 < npad
      atomicAdd(&sb[0][slot], 1u);
      if (multi && ref_ids[i + u] == qid) atomicAdd(&sb[1][slot], 1u);
    }
  }
  __syncthreads();
  uint32_t* b = bins + (int64_t)row * 2 * RT_CHUNK;
  for (int j = tid; j < n; j += 256) {
    if (sb[0][j]) atomicAdd(&b[j], sb[0][j]);
    if (sb[1][j]) atomicAdd(&b[RT_CHUNK + j], sb[1][j]);
  }
}

// grid (rows).  The inclusive prefix sum of the bins over the sorted positives IS their full-order rank (the bin of slot j
// holds the keys in (p_{j-1}, p_j], p_j itself included).  ComputeApStats (:62-118) from the ranks, accumulated over passes.
__global__ __launch_bounds__(256) void k_rank_final(const float* __restrict__ dist, int64_t pitch,
                                                    const int32_t* __restrict__ pos_idx, const int32_t* __restrict__ pstart,
                                                    const int32_t* __restrict__ pcount, int pass,
                                                    const uint32_t* __restrict__ bins, RankAcc* __restrict__ acc) {
  __shared__ uint64_t sk[RT_CHUNK];
  __shared__ uint32_t tr[256], tp[256];
  __shared__ double rap[256];
  __shared__ int rbest[256], r1[256], r5[256], r10[256];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int P = pcount[row];
  int npad = 0;
  const int n = rt_load_sorted(sk, dist + (int64_t)row * pitch, pos_idx, pstart[row], P, pass, &npad);
  if (n == 0) return;
  const bool multi = P > RT_CHUNK;
  const uint32_t* b = bins + (int64_t)row * 2 * RT_CHUNK;
  constexpr int PER = RT_CHUNK / 256;
  const int j0 = tid * PER;
  uint32_t cr[PER], cp[PER], sr = 0, sp = 0;
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int j = j0 + u;
    cr[u] = j < n ? b[j] : 0; cp[u] = j < n ? b[RT_CHUNK + j] : 0;
    sr += cr[u]; sp += cp[u];
  }
  tr[tid] = sr; tp[tid] = sp;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {                                 // inclusive scan of the thread totals
    const uint32_t a = tid >= o ? tr[tid - o] : 0, c = tid >= o ? tp[tid - o] : 0;
    __syncthreads();
    tr[tid] += a; tp[tid] += c;
    __syncthreads();
  }
  uint32_t rank = tr[tid] - sr, ord = tp[tid] - sp;
  double ap = 0; int best = 10000, a1 = 0, a5 = 0, a10 = 0;          // :68-70
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int j = j0 + u;
    rank += cr[u]; ord += cp[u];
    if (j < n) {
      const uint32_t ret = multi ? ord : (uint32_t)(j + 1);           // :90 (`ret` after the increment)
      if ((int64_t)rank < best) best = (int)rank;                     // :77-79
      a1 += rank <= 1; a5 += rank <= 5; a10 += rank <= 10;            // :81-89
      ap += (double)ret / (double)rank;                               // :91
    }
  }
  rap[tid] = ap; rbest[tid] = best; r1[tid] = a1; r5[tid] = a5; r10[tid] = a10;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      rap[tid] += rap[tid + o]; rbest[tid] = min(rbest[tid], rbest[tid + o]);
      r1[tid] += r1[tid + o]; r5[tid] += r5[tid + o]; r10[tid] += r10[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {                                                      // one workgroup per row and pass, passes in stream order
    RankAcc a = acc[row];
    a.ap_sum += rap[0]; a.best = min(a.best, rbest[0]); a.acc1 += r1[0]; a.acc5 += r5[0]; a.acc10 += r10[0];
    acc[row] = a;
  }
}

void launch_rank_pass(const float* dist, int64_t pitch, int rows, int ng, int seg, int S, const int32_t* pos_idx,
                      const int32_t* pstart, const int32_t* pcount, const int32_t* q_ids, const int32_t* ref_ids, int pass,
                      uint32_t* bins, RankAcc* acc, hipStream_t s) {
  hipLaunchKernelGGL(k_rank_count, dim3(S, rows), dim3(256), 0, s, dist, pitch, ng, seg, pos_idx, pstart, pcount, q_ids,
                     ref_ids, pass, bins);
  hipLaunchKernelGGL(k_rank_final, dim3(rows), dim3(256), 0, s, dist, pitch, pos_idx, pstart, pcount, pass, bins, acc);
}

// ---------------------------------------------------------------------------------------------- class-level statistics
// RetrievalStatsLayer (retrieval_stats_layer.cpp:104-141, 226-304): every gallery item is a query against all the others, a hit
// is an item of the query's CLASS.  The rows of a block are the gallery items q0 .. q0 + rows - 1.  Positives of row r: the
// class list cpos[pstart[r] .. + pcount[r]) (every item of the query's class, the query and the items of its video among them;
// pcount = 0 for a query of negative class).  Three counts per positive p, all "at or before p in (d, g) order":
//   all[p]   items                    left[p]  left-out items: the query itself, and with `exclude` the items of its video
//   cls[p]   items of the class       (same video => same class, so a left-out item is a class-mate)
// val(p) = all - left, ret(p) = cls - left (:113-125); a positive that is itself left out contributes nothing.
//
// A pass ranks RT_CHUNK positives.  Unlike the fixed-reference case the positives are a constant share of the gallery spread
// over the whole order, so `key > last` discards nothing and every item of the row is searched in every pass; the chunk is
// therefore sorted ONCE per (row, pass) by k_class_sort into `skeys`, not once per segment workgroup.

// grid (rows): skeys[row][0 .. npad) = the pass's positive keys, ascending, padded with RT_NOKEY to a power of two
__global__ __launch_bounds__(256) void k_class_sort(const float* __restrict__ dist, int64_t pitch,
                                                    const int32_t* __restrict__ cpos, const int32_t* __restrict__ pstart,
                                                    const int32_t* __restrict__ pcount, int pass, uint64_t* __restrict__ skeys) {
  __shared__ uint64_t sk[RT_CHUNK];
  const int row = blockIdx.x;
  int npad = 0;
  const int n = rt_load_sorted(sk, dist + (int64_t)row * pitch, cpos, pstart[row], pcount[row], pass, &npad);
  if (n == 0) return;
  for (int j = threadIdx.x; j < npad; j += 256) skeys[(int64_t)row * RT_CHUNK + j] = sk[j];
}

// number of this pass's positives of a row and the padded length of its sorted keys (what rt_load_sorted returned to k_class_sort)
__device__ inline int rt_pass_count(int pcount, int pass, int* npad_out) {
  const int off = pass * RT_CHUNK;
  if (off >= pcount) return 0;
  const int n = min(RT_CHUNK, pcount - off);
  int npad = 1;
  while (npad < n) npad <<= 1;
  *npad_out = npad;
  return n;
}

// grid (S, rows).  bins[row][t][slot], t = 0 all / 1 class / 2 left out: the items of the segment whose key lies in
// (p_{slot-1}, p_slot].  Items beyond the pass's last positive are not counted.
__global__ __launch_bounds__(256) void k_class_count(const float* __restrict__ dist, int64_t pitch, int ng, int seg,
                                                     const uint64_t* __restrict__ skeys, const int32_t* __restrict__ pcount,
                                                     const int32_t* __restrict__ ids, const int32_t* __restrict__ cls, int q0,
                                                     int exclude, int pass, uint32_t* __restrict__ bins) {
  __shared__ uint64_t sk[RT_CHUNK];
  __shared__ uint32_t sb[3][RT_CHUNK];
  const int row = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
  int npad = 0;
  const int n = rt_pass_count(pcount[row], pass, &npad);             // uniform over the workgroup
  if (n == 0) return;
  for (int j = tid; j < npad; j += 256) sk[j] = skeys[(int64_t)row * RT_CHUNK + j];
  for (int j = tid; j < n; j += 256) { sb[0][j] = 0; sb[1][j] = 0; sb[2][j] = 0; }
  __syncthreads();
  const float* d = dist + (int64_t)row * pitch;
  const int self = q0 + row;
  const int32_t qid = ids[self], qcls = cls[self];
  const uint64_t last = sk[n - 1];
  const int begin = s * seg, end = min(ng, begin + seg);
  for (int base = begin; base < end; base += 1024) {
    const int i = base + tid * 4;
    if (i >= end) continue;
    const float4 v = *(const float4*)(d + i);
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int g = i + u;
      const uint64_t key = rt_key(e[u], (uint32_t)g);
      if (g >= end || key > last) continue;
      int slot = 0;
      for (int step = npad >> 1; step > 0; step >>= 1)
        if (sk[slot + step - 1] < key) slot += step;                // key <= last, so the answer is at most n - 1 < npad
      atomicAdd(&sb[0][slot], 1u);
      if (cls[g] == qcls) {
        atomicAdd(&sb[1][slot], 1u);
        if (g == self || (exclude && ids[g] == qid)) atomicAdd(&sb[2][slot], 1u);
      }
    }
  }
  __syncthreads();
  uint32_t* b = bins + (int64_t)row * 3 * RT_CHUNK;
  for (int j = tid; j < n; j += 256)
#pragma unroll
    for (int t = 0; t < 3; ++t)
      if (sb[t][j]) atomicAdd(&b[t * RT_CHUNK + j], sb[t][j]);
}

// grid (rows).  Inclusive prefix sums of the three bin arrays over the sorted positives = the three counts; ComputeStats
// (:113-128) from them.  Integer counts; the AP terms are summed in double in a fixed order (per thread ascending slot, then
// a fixed tree, then pass by pass in stream order).
__global__ __launch_bounds__(256) void k_class_final(const uint64_t* __restrict__ skeys, const int32_t* __restrict__ pcount,
                                                     const int32_t* __restrict__ ids, int q0, int exclude, int pass,
                                                     const uint32_t* __restrict__ bins, ClassAcc* __restrict__ acc) {
  __shared__ uint32_t ta[256], tc[256], tl[256];
  __shared__ double rap[256];
  __shared__ int rn[256], r1[256], r5[256];
  const int row = blockIdx.x, tid = threadIdx.x;
  int npad = 0;
  const int n = rt_pass_count(pcount[row], pass, &npad);
  if (n == 0) return;
  const int self = q0 + row;
  const int32_t qid = ids[self];
  const uint32_t* b = bins + (int64_t)row * 3 * RT_CHUNK;
  const uint64_t* sk = skeys + (int64_t)row * RT_CHUNK;
  constexpr int PER = RT_CHUNK / 256;
  const int j0 = tid * PER;
  uint32_t ca[PER], cc[PER], cl[PER], sa = 0, sc = 0, sl = 0;
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int j = j0 + u;
    ca[u] = j < n ? b[j] : 0; cc[u] = j < n ? b[RT_CHUNK + j] : 0; cl[u] = j < n ? b[2 * RT_CHUNK + j] : 0;
    sa += ca[u]; sc += cc[u]; sl += cl[u];
  }
  ta[tid] = sa; tc[tid] = sc; tl[tid] = sl;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {                                 // inclusive scan of the thread totals
    const uint32_t x = tid >= o ? ta[tid - o] : 0, y = tid >= o ? tc[tid - o] : 0, z = tid >= o ? tl[tid - o] : 0;
    __syncthreads();
    ta[tid] += x; tc[tid] += y; tl[tid] += z;
    __syncthreads();
  }
  uint32_t all = ta[tid] - sa, cmate = tc[tid] - sc, left = tl[tid] - sl;
  double ap = 0; int np = 0, a1 = 0, a5 = 0;
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int j = j0 + u;
    all += ca[u]; cmate += cc[u]; left += cl[u];
    if (j < n) {
      const int p = (int)(uint32_t)sk[j];
      if (p != self && !(exclude && ids[p] == qid)) {                 // :113-115
        const uint32_t val = all - left, ret = cmate - left;          // :116, :124
        np += 1; a1 += val <= 1; a5 += val <= 5;                      // :118-123
        ap += (double)ret / (double)val;                              // :125
      }
    }
  }
  rap[tid] = ap; rn[tid] = np; r1[tid] = a1; r5[tid] = a5;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { rap[tid] += rap[tid + o]; rn[tid] += rn[tid + o]; r1[tid] += r1[tid + o]; r5[tid] += r5[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {                                                      // one workgroup per row and pass, passes in stream order
    ClassAcc a = acc[row];
    a.ap_sum += rap[0]; a.npos += rn[0]; a.acc1 += r1[0]; a.n5 += r5[0];
    acc[row] = a;
  }
}

void launch_class_pass(const float* dist, int64_t pitch, int rows, int ng, int seg, int S, const int32_t* cpos,
                       const int32_t* pstart, const int32_t* pcount, const int32_t* ids, const int32_t* cls, int q0, int exclude,
                       int pass, uint64_t* skeys, uint32_t* bins, ClassAcc* acc, hipStream_t s) {
  hipLaunchKernelGGL(k_class_sort, dim3(rows), dim3(256), 0, s, dist, pitch, cpos, pstart, pcount, pass, skeys);
  hipLaunchKernelGGL(k_class_count, dim3(S, rows), dim3(256), 0, s, dist, pitch, ng, seg, skeys, pcount, ids, cls, q0, exclude,
                     pass, bins);
  hipLaunchKernelGGL(k_class_final, dim3(rows), dim3(256), 0, s, skeys, pcount, ids, q0, exclude, pass, bins, acc);
}

// ---------------------------------------------------------------------------------------------- nearest-neighbour lists
// vv_gallery_nearest*, selection form: the k smallest eligible keys of every scratch row for k up to RT_CHUNK, the row never
// sorted.  Radix select on the key's high word (rt_word), most significant digit first, digits of 12, 12 and 8 bits:
//   k_sel_hist<P>   grid (S, rows): the histogram of digit P over the segment's eligible items whose higher digits equal the
//                   threshold's, in LDS, its non-zero bins added to hist[row][4096]
//   k_sel_scan<P>   grid (rows), one wave: the bin in which the running count reaches the count still wanted becomes digit P of
//                   the threshold T; the wanted count drops by the items in the bins below it; the bins are cleared for P + 1
// After digit 2, T is the word of the k-th eligible key and st[1] = k - #{eligible words < T}: how many of the keys with word
// == T are taken.  Those are the ones of LOWEST GALLERY INDEX, whatever order the workgroups run in: k_sel_hist<2> keeps every
// segment's own histogram (segh[row][s][256]), so k_sel_collect knows how many equal words the segments before its own hold and
// numbers its own by an in-workgroup scan in index order.  Words below T go to the row's candidates at positions drawn from an
// atomic counter -- k_sel_sort orders the at most RT_CHUNK candidates in LDS and writes the lists.
// A row with fewer than k eligible items (st[2] = 1, found by k_sel_scan<0>) skips digits 1 and 2 and takes every eligible item.
// st: uint32 [rows][4] = {T, wanted, take-all, candidates below T}, zero on entry; hist: zero on entry.
// Eligible for row r: every item; with own != NULL those whose id differs from own[r]; with self0 >= 0 not item self0 + r.
constexpr int SEL_BINS = RT_SEL_BINS, SEL_LAST_BINS = RT_SEL_LAST_BINS;        // 12-bit digits 0 and 1, 8-bit digit 2

__device__ inline bool rt_eligible(int g, const int32_t* __restrict__ ids, bool other, int32_t oid, int self) {
  return g != self && (!other || ids[g] != oid);
}

template <int P>
__global__ __launch_bounds__(256) void k_sel_hist(const float* __restrict__ dist, int64_t pitch, int ng, int seg,
                                                  const int32_t* __restrict__ ids, const int32_t* __restrict__ own, int self0,
                                                  const uint32_t* __restrict__ st, uint32_t* __restrict__ hist,
                                                  uint32_t* __restrict__ segh) {
  constexpr int SHIFT = P == 0 ? 20 : P == 1 ? 8 : 0, NB = P == 2 ? SEL_LAST_BINS : SEL_BINS, HI = P == 1 ? 20 : 8;
  __shared__ uint32_t sh[NB];
  const int row = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
  if (P > 0 && st[row * 4 + 2]) return;                              // (uniform) fewer than k eligible items: all are taken
  const uint32_t T = P > 0 ? st[row * 4] : 0;
  for (int j = tid; j < NB; j += 256) sh[j] = 0;
  __syncthreads();
  const float* d = dist + (int64_t)row * pitch;
  const bool other = own != nullptr;
  const int32_t oid = other ? own[row] : 0;
  const int self = self0 < 0 ? -1 : self0 + row;
  const int begin = s * seg, end = min(ng, begin + seg);
  for (int base = begin; base < end; base += 1024) {                 // seg is a multiple of 1024, pitch of 4
    const int i = base + tid * 4;
    if (i >= end) continue;
    const float4 v = *(const float4*)(d + i);                        // i + 3 < pitch: the row's pad may be read, never counted
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int g = i + u;
      if (g >= end || !rt_eligible(g, ids, other, oid, self)) continue;
      const uint32_t w = rt_word(e[u]);
      if (P == 0 || (w >> HI) == (T >> HI)) atomicAdd(&sh[(w >> SHIFT) & (NB - 1)], 1u);
    }
  }
  __syncthreads();
  for (int j = tid; j < NB; j += 256)
    if (sh[j]) atomicAdd(&hist[(int64_t)row * SEL_BINS + j], sh[j]);
  if (P == 2) segh[((int64_t)row * gridDim.x + s) * SEL_LAST_BINS + tid] = sh[tid];
}

template <int P>
__global__ __launch_bounds__(64) void k_sel_scan(uint32_t* __restrict__ hist, uint32_t* __restrict__ st, int k) {
  constexpr int SHIFT = P == 0 ? 20 : P == 1 ? 8 : 0, NB = P == 2 ? SEL_LAST_BINS : SEL_BINS, PER = NB / 64;
  const int row = blockIdx.x, lane = threadIdx.x;
  uint32_t* sr = st + row * 4;
  if (P > 0 && sr[2]) return;
  uint32_t* h = hist + (int64_t)row * SEL_BINS + lane * PER;          // this lane's PER consecutive bins
  const uint32_t want = P == 0 ? (uint32_t)k : sr[1];
  uint32_t sum = 0;
  for (int j = 0; j < PER; j += 4) { const uint4 v = *(const uint4*)(h + j); sum += v.x + v.y + v.z + v.w; }
  uint32_t incl = sum;
  for (int o = 1; o < 64; o <<= 1) { const uint32_t a = __shfl_up(incl, o); if (lane >= o) incl += a; }
  const uint32_t total = __shfl(incl, 63), excl = incl - sum;
  if (total < want) {                                                  // only at P = 0: later digits count >= `want` items
    if (lane == 0) { sr[0] = 0xffffffffu; sr[1] = 0; sr[2] = 1; }
  } else if (excl < want && want <= incl) {                            // exactly one lane
    uint32_t below = excl;
    int bin = 0;
    for (; bin < PER - 1; ++bin) { const uint32_t c = h[bin]; if (below + c >= want) break; below += c; }
    sr[0] = (P == 0 ? 0u : sr[0]) | ((uint32_t)(lane * PER + bin) << SHIFT);
    sr[1] = want - below;
  }
  for (int j = 0; j < PER; j += 4) *(uint4*)(h + j) = make_uint4(0, 0, 0, 0);
}

// grid (S, rows).  cand: uint64 [rows][RT_CHUNK].
__global__ __launch_bounds__(256) void k_sel_collect(const float* __restrict__ dist, int64_t pitch, int ng, int seg, int k,
                                                     const int32_t* __restrict__ ids, const int32_t* __restrict__ own, int self0,
                                                     uint32_t* __restrict__ st, const uint32_t* __restrict__ segh,
                                                     uint64_t* __restrict__ cand) {
  __shared__ uint32_t wtot[4];
  const int row = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t T = st[row * 4], want_eq = st[row * 4 + 1];
  const bool all = st[row * 4 + 2] != 0;
  const uint32_t below = (uint32_t)k - want_eq;                        // (unused with `all`) the candidates' slots for words == T
  uint64_t* c = cand + (int64_t)row * RT_CHUNK;
  // equal words in the segments before this one, and whether this segment has any that are taken
  uint32_t eqbase = 0;
  bool ties = false;
  if (!all) {
    const uint32_t* sg = segh + (int64_t)row * gridDim.x * SEL_LAST_BINS + (T & (SEL_LAST_BINS - 1));
    for (int t = 0; t < s; ++t) eqbase += sg[t * SEL_LAST_BINS];
    ties = eqbase < want_eq && sg[s * SEL_LAST_BINS] != 0;
  }
  const float* d = dist + (int64_t)row * pitch;
  const bool other = own != nullptr;
  const int32_t oid = other ? own[row] : 0;
  const int self = self0 < 0 ? -1 : self0 + row;
  const int begin = s * seg, end = min(ng, begin + seg);
  for (int base = begin; base < end; base += 1024) {
    const int i = base + tid * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < end) v = *(const float4*)(d + i);
    const float e[4] = {v.x, v.y, v.z, v.w};
    uint32_t w[4];
    bool el[4], eq[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int g = i + u;
      el[u] = g < end && rt_eligible(g, ids, other, oid, self);
      w[u] = rt_word(e[u]);
      eq[u] = el[u] && !all && w[u] == T;
      if (el[u] && (all || w[u] < T)) {
        const uint32_t pos = atomicAdd(&st[row * 4 + 3], 1u);          // fewer than k of them
        if (pos < (uint32_t)RT_CHUNK) c[pos] = ((uint64_t)w[u] << 32) | (uint32_t)g;
      }
    }
    if (!ties) continue;                                               // (uniform over the workgroup)
    // ordinal of an equal word among the row's equal words in index order: thread t holds items base + 4 t .. + 3
    const uint64_t lower = ((uint64_t)1 << lane) - 1;
    uint32_t before = 0, wsum = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint64_t m = __ballot(eq[u]);
      before += (uint32_t)__popcll(m & lower);
      wsum += (uint32_t)__popcll(m);
    }
    if (lane == 0) wtot[wave] = wsum;
    __syncthreads();
    uint32_t chunk = 0;
    for (int t = 0; t < 4; ++t) { if (t < wave) before += wtot[t]; chunk += wtot[t]; }
    __syncthreads();                                                   // wtot is written again in the next round
    uint32_t ord = eqbase + before;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (eq[u]) {
        if (ord < want_eq && below + ord < (uint32_t)RT_CHUNK) c[below + ord] = ((uint64_t)T << 32) | (uint32_t)(i + u);
        ++ord;
      }
    eqbase += chunk;
    ties = eqbase < want_eq;
  }
}

// grid (rows).  idx / dst: [rows][k]; slots past the eligible count read -1 / 0.
__global__ __launch_bounds__(256) void k_sel_sort(const uint64_t* __restrict__ cand, const uint32_t* __restrict__ st, int k,
                                                  int32_t* __restrict__ idx, float* __restrict__ dst) {
  __shared__ uint64_t sk[RT_CHUNK];
  const int row = blockIdx.x;
  const int n = st[row * 4 + 2] ? (int)min(st[row * 4 + 3], (uint32_t)k) : k;
  int npad = 1;
  while (npad < n) npad <<= 1;
  for (int j = threadIdx.x; j < npad; j += 256) sk[j] = j < n ? cand[(int64_t)row * RT_CHUNK + j] : RT_NOKEY;
  __syncthreads();
  rt_bitonic(sk, npad);
  for (int j = threadIdx.x; j < k; j += 256) {
    const uint64_t key = j < n ? sk[j] : RT_NOKEY;
    idx[(int64_t)row * k + j] = j < n ? (int32_t)(uint32_t)key : -1;
    dst[(int64_t)row * k + j] = j < n ? rt_key_dist(key) : 0.f;
  }
}

void launch_select(const float* dist, int64_t pitch, int rows, int ng, int k, int seg, int S, const int32_t* ids,
                   const int32_t* own, int self0, uint32_t* st, uint32_t* hist, uint32_t* segh, uint64_t* cand, int32_t* idx,
                   float* dst, hipStream_t s) {
  const dim3 grid(S, rows), wg(256);
  hipLaunchKernelGGL(k_sel_hist<0>, grid, wg, 0, s, dist, pitch, ng, seg, ids, own, self0, st, hist, segh);
  hipLaunchKernelGGL(k_sel_scan<0>, dim3(rows), dim3(64), 0, s, hist, st, k);
  hipLaunchKernelGGL(k_sel_hist<1>, grid, wg, 0, s, dist, pitch, ng, seg, ids, own, self0, st, hist, segh);
  hipLaunchKernelGGL(k_sel_scan<1>, dim3(rows), dim3(64), 0, s, hist, st, k);
  hipLaunchKernelGGL(k_sel_hist<2>, grid, wg, 0, s, dist, pitch, ng, seg, ids, own, self0, st, hist, segh);
  hipLaunchKernelGGL(k_sel_scan<2>, dim3(rows), dim3(64), 0, s, hist, st, k);
  hipLaunchKernelGGL(k_sel_collect, grid, wg, 0, s, dist, pitch, ng, seg, k, ids, own, self0, st, segh, cand);
  hipLaunchKernelGGL(k_sel_sort, dim3(rows), dim3(64 * 4), 0, s, cand, st, k, idx, dst);
}

// ---------------------------------------------------------------------------------------------- k-NN vote
// vv_gallery_knn_scores*: the class votes of the neighbour lists the two forms above left on the device.  grid (rows), one workgroup
// per query row.  idx / dist: the block's lists, `stride` entries between two rows, filled slots first, idx -1 behind them;
// labels: int32 [ng], every entry in [0, C) (checked on the host); out: row r at out + r * C, EVERY element written (a row without
// a filled slot: +0.0f); m_out: int32 [rows], the filled slots.  C <= KNN_MAX_CLASSES, k <= RT_CHUNK.
// VEC: 16-byte stores (out on 16 bytes and C % 4 == 0, the launcher's test); otherwise one float per store, the same values.
constexpr int KNN_MAX_CLASSES = 4096;

// filled slots of this thread's share of the list, added up over the workgroup into *sm (zero and visible before the call)
__device__ inline void knn_count_filled(int mine, int* sm) {
  const int w = (int)__popcll(__ballot(mine != 0));
  if ((threadIdx.x & 63) == 0 && w) atomicAdd(sm, w);
}

// UNIFORM: integer bins in LDS (exact, order-free), score = (float)V_c / (float)m: one rounding.
template <bool VEC>
__global__ __launch_bounds__(256) void k_knn_vote(const int32_t* __restrict__ idx, int64_t stride, int k,
                                                  const int32_t* __restrict__ labels, int C, float* __restrict__ out,
                                                  int32_t* __restrict__ m_out) {
  __shared__ __attribute__((aligned(16))) uint32_t sb[KNN_MAX_CLASSES];
  __shared__ int sm;
  const int row = blockIdx.x, tid = threadIdx.x;
  for (int c = tid; c < C; c += 256) sb[c] = 0;
  if (tid == 0) sm = 0;
  __syncthreads();
  const int32_t* li = idx + (int64_t)row * stride;
  for (int base = 0; base < k; base += 256) {                      // (uniform trip count: the ballot sees whole waves)
    const int j = base + tid;
    const int g = j < k ? li[j] : -1;
    if (g >= 0) {
      const uint32_t c = (uint32_t)labels[g];
      if (c < (uint32_t)C) atomicAdd(&sb[c], 1u);
    }
    knn_count_filled(g >= 0, &sm);
  }
  __syncthreads();
  const int m = sm;
  const float fm = (float)m;
  float* o = out + (int64_t)row * C;
  if (VEC) {
    for (int c4 = tid; c4 < C / 4; c4 += 256) {
      const uint4 v = *(const uint4*)&sb[c4 * 4];
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m) r = make_float4((float)v.x / fm, (float)v.y / fm, (float)v.z / fm, (float)v.w / fm);
      *(float4*)(o + c4 * 4) = r;
    }
  } else {
    for (int c = tid; c < C; c += 256) o[c] = m ? (float)sb[c] / fm : 0.f;
  }
  if (tid == 0) m_out[row] = m;
}

// the weight of list position j under VV_KNN_EXP: s = -0.5f d (exact), the difference and the quotient each rounded once
__device__ inline float knn_exp_weight(float d, float d0, float T) {
#pragma clang fp contract(off)
  const float s = -0.5f * d, s0 = -0.5f * d0;
  const float diff = s - s0;
  const float arg = diff / T;
  return expf(arg);
}

// EXP: fp32 sums in a FIXED order, no floating-point atomics.  The filled positions are sorted by (class, position) with the
// file's bitonic sort; the thread at the head of a class's run adds the run's weights serially, so V_c is the sum of its weights
// in ASCENDING LIST POSITION.  V: thread t adds V_c over its ceil(C / 256) consecutive classes in ascending class, and the 256
// partials are folded by the fixed tree the rank kernels use (t += t + o, o = 128 .. 1).  Classes without a vote add +0.0f, so a
// row whose neighbours share one class has V == V_c and scores exactly 1.0 there.  w_0 = expf(0) = 1: V >= 1 wherever m >= 1.
template <bool VEC>
__global__ __launch_bounds__(256) void k_knn_vote_exp(const int32_t* __restrict__ idx, const float* __restrict__ dist,
                                                      int64_t stride, int k, float T, const int32_t* __restrict__ labels, int C,
                                                      float* __restrict__ out, int32_t* __restrict__ m_out) {
  __shared__ uint64_t sk[RT_CHUNK];                                // (class << 32 | position), ascending; RT_NOKEY behind the filled ones
  __shared__ float sw[RT_CHUNK];                                   // weight by list position
  __shared__ __attribute__((aligned(16))) float sv[KNN_MAX_CLASSES];
  __shared__ float sp[256];
  __shared__ int sm;
  const int row = blockIdx.x, tid = threadIdx.x;
  const int32_t* li = idx + (int64_t)row * stride;
  const float* ld = dist + (int64_t)row * stride;
  int npad = 1;
  while (npad < k) npad <<= 1;                                     // k <= RT_CHUNK, a power of two
  for (int c = tid; c < C; c += 256) sv[c] = 0.f;
  if (tid == 0) sm = 0;
  __syncthreads();
  const float d0 = ld[0];                                          // (slot 0 exists: k >= 1; read as a weight only where m >= 1)
  for (int base = 0; base < npad; base += 256) {                   // npad < 256: one round, the threads past it hold nothing
    const int j = base + tid;
    const int g = j < k ? li[j] : -1;
    uint64_t key = RT_NOKEY;
    float w = 0.f;
    if (g >= 0) {
      const uint32_t c = (uint32_t)labels[g];
      if (c < (uint32_t)C) { key = ((uint64_t)c << 32) | (uint32_t)j; w = knn_exp_weight(ld[j], d0, T); }
    }
    if (j < npad) { sk[j] = key; sw[j] = w; }
    knn_count_filled(key != RT_NOKEY, &sm);
  }
  __syncthreads();
  rt_bitonic(sk, npad);
  const int m = sm;
  for (int p = tid; p < m; p += 256) {
    const uint64_t key = sk[p];
    const uint32_t c = (uint32_t)(key >> 32);
    if (p > 0 && (uint32_t)(sk[p - 1] >> 32) == c) continue;       // not the head of its class's run
    float acc = sw[(uint32_t)key];
    for (int t = p + 1; t < m; ++t) {
      const uint64_t kt = sk[t];
      if ((uint32_t)(kt >> 32) != c) break;
      acc += sw[(uint32_t)kt];
    }
    sv[c] = acc;                                                   // one head per class: no other thread writes sv[c]
  }
  __syncthreads();
  const int per = (C + 255) / 256;
  float part = 0.f;
  for (int c = tid * per; c < min(C, (tid + 1) * per); ++c) part += sv[c];
  sp[tid] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sp[tid] += sp[tid + o];
    __syncthreads();
  }
  const float V = sp[0];
  float* o = out + (int64_t)row * C;
  if (VEC) {
    for (int c4 = tid; c4 < C / 4; c4 += 256) {
      const float4 v = *(const float4*)&sv[c4 * 4];
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m) r = make_float4(v.x / V, v.y / V, v.z / V, v.w / V);
      *(float4*)(o + c4 * 4) = r;
    }
  } else {
    for (int c = tid; c < C; c += 256) o[c] = m ? sv[c] / V : 0.f;
  }
  if (tid == 0) m_out[row] = m;
}

// -> the store form: 1 the 16-byte one, 2 element-wise
int launch_knn_vote(const int32_t* idx, const float* dist, int64_t stride, int rows, int k, int exp_weights, float T,
                    const int32_t* labels, int C, float* out, int32_t* m_out, hipStream_t s) {
  const bool vec = ((uintptr_t)out & 15) == 0 && C % 4 == 0;
  const dim3 grid(rows), wg(256);
  if (exp_weights) {
    if (vec) hipLaunchKernelGGL(k_knn_vote_exp<true>, grid, wg, 0, s, idx, dist, stride, k, T, labels, C, out, m_out);
    else hipLaunchKernelGGL(k_knn_vote_exp<false>, grid, wg, 0, s, idx, dist, stride, k, T, labels, C, out, m_out);
  } else {
    if (vec) hipLaunchKernelGGL(k_knn_vote<true>, grid, wg, 0, s, idx, stride, k, labels, C, out, m_out);
    else hipLaunchKernelGGL(k_knn_vote<false>, grid, wg, 0, s, idx, stride, k, labels, C, out, m_out);
  }
  return vec ? 1 : 2;
}

// ---------------------------------------------------------------------------------------------- pooling by id
// Video-level retrieval (retrieval_stats_layer.cpp:189-198): out[u] = sum over the items of id u of (1 / count_u) x_i, the
// weight multiplied into every term as the reference's weight matrix does, items in ascending index (pos_idx groups them so).
// grid (n_ids); feat [n][Dp], out [n_ids][Dp] (the zero padding of the columns sums to zero).
__global__ __launch_bounds__(256) void k_pool_by_id(const float* __restrict__ feat, int Dp, const int32_t* __restrict__ pos_idx,
                                                    const int32_t* __restrict__ ustart, float* __restrict__ out) {
  const int u = blockIdx.x, b = ustart[u], e = ustart[u + 1];
  const float w = 1.0f / (float)(e - b);                                // :193
  for (int col = threadIdx.x; col < Dp; col += 256) {
    float acc = 0.f;
    for (int j = b; j < e; ++j) acc = fmaf(w, feat[(int64_t)pos_idx[j] * Dp + col], acc);
    out[(int64_t)u * Dp + col] = acc;
  }
}
void launch_pool_by_id(const float* feat, int Dp, const int32_t* pos_idx, const int32_t* ustart, int n_ids, float* out,
                       hipStream_t s) {
  hipLaunchKernelGGL(k_pool_by_id, dim3(n_ids), dim3(256), 0, s, feat, Dp, pos_idx, ustart, out);
}

}  // namespace vv
