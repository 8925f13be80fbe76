// kernels_ivf.hip -- inverted-file search on a gallery (include/videovec.h: vv_ivf_search; the entry points are ivf.hip, the sizes are
// vv_ivf_plan.h).  gfx950 (MI355X, CDNA4) only.  HAS NO REFERENCE COUNTERPART: the reference searches exhaustively.
//
// One block of queries = the similarity of the block against the centroids (k_sim_f32, as it stands), k_ivf_probe, the stable counting
// sort of the block's (query, cluster) pairs by cluster (k_km_hist / k_km_starts / k_km_scan / k_km_scatter, kernels_kmeans.hip, as they
// stand), k_ivf_tiles, k_sim_f32_grouped and k_ivf_select.  A distance is the float k_sim_f32_grouped stores, and it runs the tile body
// k_sim_f32 runs (vv_rt_device.h: rt_tile_mma), so it is the float vv_gallery_topk would rank for the same query and item.  No
// floating-point atomic exists here; every index that addresses memory was written by one of the library's own kernels.
#include "vv_internal.h"
#include "vv_rt_device.h"

namespace vv {

// the probe key's one add, rounded on its own (kernels_kmeans.hip: km_add)
__device__ __forceinline__ float ivf_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// ---------------------------------------------------------------------------------------------- probe
// One wave per query row.  key = d (SPHERICAL) or d + nn_c (EUCLIDEAN: one fp32 add, not contracted), the nprobe smallest (key, c)
// ascending: km_less's order (kernels_kmeans.hip) -- on keys that are not NaN it is the order of rt_key(key, c) once a zero key is
// written +0, which is what the wave's sorted list keeps.  A NaN key is offered by nobody; if fewer than nprobe keys are numbers, all
// of them were selected and the free slots take the NaN clusters in ascending index: the lowest unused ones.
// Then, p ascending: off[p] = the sizes of the lists probed before p, m = their total; counts[c] += 1 for every probed cluster
// (integer atomics).  all: every cluster, in ascending index.
template <bool EUCLID>
__global__ __launch_bounds__(64) void k_ivf_probe(const float* __restrict__ score, int C, int nprobe, int all,
                                                  const float* __restrict__ nn, const int32_t* __restrict__ start,
                                                  int32_t* __restrict__ probe, int32_t* __restrict__ off, int32_t* __restrict__ m,
                                                  int32_t* __restrict__ counts, IvfRec* __restrict__ rec) {
  __shared__ int sp[KM_MAX_CLUSTERS];
  const int row = blockIdx.x, lane = threadIdx.x;
  const float* srow = score + (int64_t)row * C;
  if (all) {
    for (int c = lane; c < C; c += 64) sp[c] = c;
  } else {
    uint64_t mine = RT_NOKEY, kth = RT_NOKEY;
    for (int base = 0; base < C; base += 64) {                     // (uniform trip count: rt_offer is a wave-wide call)
      const int c = base + lane;
      float key = __builtin_nanf("");
      if (c < C) { key = srow[c]; if (EUCLID) key = ivf_add(key, nn[c]); }
      if (key == 0.f) key = 0.f;                                    // -0 and +0 are one key
      rt_offer(rt_key(key, (uint32_t)c), key == key, mine, kth, lane, nprobe);
    }
    const int filled = (int)__popcll(__ballot(mine != RT_NOKEY));
    if (mine != RT_NOKEY) sp[lane] = (int)(uint32_t)mine;          // (lanes >= nprobe hold RT_NOKEY)
    if (filled < nprobe) {
      int f = filled;
      for (int base = 0; base < C && f < nprobe; base += 64) {     // (f is uniform)
        const int c = base + lane;
        bool isnan = false;
        if (c < C) { float key = srow[c]; if (EUCLID) key = ivf_add(key, nn[c]); isnan = key != key; }
        const uint64_t mask = __ballot(isnan);
        const int pos = f + (int)__popcll(mask & (((uint64_t)1 << lane) - 1));
        if (isnan && pos < nprobe) sp[pos] = c;
        f += (int)__popcll(mask);
      }
    }
  }
  __syncthreads();
  int run = 0;
  for (int base = 0; base < nprobe; base += 64) {
    const int p = base + lane;
    const int c = p < nprobe ? sp[p] : -1;
    const int size = c >= 0 ? start[c + 1] - start[c] : 0;
    int incl = size;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int a = __shfl_up(incl, o, 64); if (lane >= o) incl += a; }
    if (c >= 0) {
      const int64_t pair = (int64_t)row * nprobe + p;
      probe[pair] = c; off[pair] = run + incl - size;
      atomicAdd(&counts[c], 1);
    }
    run += __shfl(incl, 63, 64);
  }
  if (lane == 0) {
    m[row] = run;
    if (run) atomicAdd((unsigned long long*)&rec->candidates, (unsigned long long)run);
  }
}

void launch_ivf_probe(const float* score, int rows, int C, int nprobe, int all, int euclid, const float* nn, const int32_t* start,
                      int32_t* probe, int32_t* off, int32_t* m, int32_t* counts, IvfRec* rec, hipStream_t s) {
  if (euclid) hipLaunchKernelGGL(k_ivf_probe<true>, dim3((unsigned)rows), dim3(64), 0, s, score, C, nprobe, all, nn, start, probe, off, m, counts, rec);
  else hipLaunchKernelGGL(k_ivf_probe<false>, dim3((unsigned)rows), dim3(64), 0, s, score, C, nprobe, all, nn, start, probe, off, m, counts, rec);
}

// ---------------------------------------------------------------------------------------------- tile table
// One workgroup.  Cluster c with a queries (qstart) and b items (start) gives ceil(a / 128) x ceil(b / 128) tiles, none if either is
// zero; thread t owns the clusters t P .. t P + P - 1, P = ceil(C / 256), as k_km_starts does.  A cluster's tiles are consecutive, query
// tiles fastest: the workgroups that take them side by side share the cluster's item rows.  *ntiles = their number, cut to the table's
// capacity (vv_ivf_plan.h proves it is never reached); rec->tiles += the uncut number (one thread, stream order: no atomic needed).
__global__ __launch_bounds__(256) void k_ivf_tiles(const int32_t* __restrict__ start, const int32_t* __restrict__ qstart, int C,
                                                   int4* __restrict__ tiles, int tile_cap, int32_t* __restrict__ ntiles,
                                                   IvfRec* __restrict__ rec) {
  __shared__ int s_t[256];
  const int tid = threadIdx.x, per = (C + 255) / 256, c0 = min(C, tid * per), c1 = min(C, c0 + per);
  int mine = 0;
  for (int c = c0; c < c1; ++c) {
    const int a = qstart[c + 1] - qstart[c], b = start[c + 1] - start[c];
    if (a > 0 && b > 0) mine += ((a + IVF_TILE - 1) / IVF_TILE) * ((b + IVF_TILE - 1) / IVF_TILE);
  }
  s_t[tid] = mine;
  __syncthreads();
  int64_t base = 0;                                                // (integers: any order)
  for (int t = 0; t < tid; ++t) base += s_t[t];
  for (int c = c0; c < c1; ++c) {
    const int a = qstart[c + 1] - qstart[c], b = start[c + 1] - start[c];
    if (a <= 0 || b <= 0) continue;
    const int mt_n = (a + IVF_TILE - 1) / IVF_TILE, nt_n = (b + IVF_TILE - 1) / IVF_TILE;
    for (int nt = 0; nt < nt_n; ++nt)
      for (int mt = 0; mt < mt_n; ++mt, ++base)
        if (base < tile_cap) tiles[base] = make_int4(c, mt, nt, 0);
  }
  if (tid == 255) { *ntiles = (int32_t)min(base, (int64_t)tile_cap); rec->tiles += base; }
}
void launch_ivf_tiles(const int32_t* start, const int32_t* qstart, int C, int4* tiles, int tile_cap, int32_t* ntiles, IvfRec* rec, hipStream_t s) {
  hipLaunchKernelGGL(k_ivf_tiles, dim3(1), dim3(256), 0, s, start, qstart, C, tiles, tile_cap, ntiles, rec);
}

// ---------------------------------------------------------------------------------------------- grouped similarity
// k_sim_f32's tile body on tiles that belong to clusters of different sizes.  A FIXED grid: workgroup w takes the table's tiles w,
// w + grid, .. below *ntiles, which it reads from device memory -- no grid depends on data, no host read sits in front of the launch.
// Tile {c, mt, nt}: its query rows are the pairs qlist[qstart[c] + 128 mt ..] (row = pair / nprobe of the block's queries, as the ROWS
// form of k_sim_f32_t reads a list), its item rows the slab rows start[c] + 128 nt ..; rows past either end repeat the last one and are
// never stored.  Item j of the cluster against pair (i, p) goes to cand[i pitch + off[i][p] + j] as -2.0f * acc + 0.0f: k_sim_f32's store.
__global__ __launch_bounds__(256) void k_sim_f32_grouped(IvfBlock a) {
  __shared__ __attribute__((aligned(16))) float sA[RT_BM * RT_LD];
  __shared__ __attribute__((aligned(16))) float sB[RT_BN * RT_LD];
  __shared__ int64_t sdst[RT_BM];                                   // where tile row t's candidates of this item tile begin; -1: no such row
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int srow = tid >> 3, c4 = tid & 7;
  const int nt_all = min(*a.ntiles, a.tile_cap);
  for (int t = blockIdx.x; t < nt_all; t += gridDim.x) {            // (uniform over the workgroup)
    const int4 tl = a.tiles[t];
    const int q0 = a.qstart[tl.x] + tl.y * RT_BM, q1 = a.qstart[tl.x + 1];
    const int i0 = a.start[tl.x] + tl.z * RT_BN, i1 = a.start[tl.x + 1];
#define IVF_QPTR(i) ((const float4*)(a.Q + (int64_t)(a.qlist[min(q0 + srow + 32 * (i), q1 - 1)] / a.nprobe) * a.Dp) + c4)
#define IVF_IPTR(i) ((const float4*)(a.slab + (int64_t)min(i0 + srow + 32 * (i), i1 - 1) * a.Dp) + c4)
    const float4 *ga0 = IVF_QPTR(0), *ga1 = IVF_QPTR(1), *ga2 = IVF_QPTR(2), *ga3 = IVF_QPTR(3);
    const float4 *gb0 = IVF_IPTR(0), *gb1 = IVF_IPTR(1), *gb2 = IVF_IPTR(2), *gb3 = IVF_IPTR(3);
#undef IVF_QPTR
#undef IVF_IPTR
    __syncthreads();                                               // the previous tile's stores have read sdst
    if (tid < RT_BM) {
      int64_t d = -1;
      if (q0 + tid < q1) { const int pair = a.qlist[q0 + tid]; d = (int64_t)(pair / a.nprobe) * a.pitch + a.off[pair] + tl.z * RT_BN; }
      sdst[tid] = d;
    }
    f32x16 acc[2][2];
    rt_tile_mma(ga0, ga1, ga2, ga3, gb0, gb1, gb2, gb3, a.Dp, sA, sB, acc);       // (its first barrier publishes sdst: Dp >= 32)
    // C/D map of the 32x32 MFMA: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        const int col = wn * 64 + y * 32 + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int64_t d = sdst[wm * 64 + x * 32 + (e & 3) + 8 * (e >> 2) + 4 * h];
          if (d >= 0 && i0 + col < i1) a.cand[d + col] = -2.0f * acc[x][y][e] + 0.0f;
        }
      }
  }
}
void launch_sim_f32_grouped(const IvfBlock& b, int grid_wgs, hipStream_t s) {
  hipLaunchKernelGGL(k_sim_f32_grouped, dim3((unsigned)grid_wgs), dim3(256), 0, s, b);
}

// ---------------------------------------------------------------------------------------------- select
// One workgroup per query row: the k <= RT_MAX_K smallest (rt_word(d), g) of its m candidates, g the ORIGINAL item index (list[]), so
// equal distances order by ascending gallery index across clusters -- vv_gallery_topk's order, by its own sorted list (rt_offer).  Wave w
// takes the probes w, w + 4, .., 64 candidates at a time; wave 0 merges the four lists as k_topk_part does.  Slots past m: -1 / 0.
__global__ __launch_bounds__(256) void k_ivf_select(IvfBlock a, int k, int32_t* __restrict__ idx, float* __restrict__ dst) {
  __shared__ uint64_t sl[4][RT_MAX_K];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* d = a.cand + (int64_t)row * a.pitch;
  uint64_t mine = RT_NOKEY, kth = RT_NOKEY;
  for (int p = wave; p < a.nprobe; p += 4) {                       // (everything below is uniform in the wave)
    const int64_t pair = (int64_t)row * a.nprobe + p;
    const int c = a.probe[pair], o = a.off[pair], s0 = a.start[c], size = a.start[c + 1] - s0;
    for (int base = 0; base < size; base += 64) {
      const int j = base + lane;
      const bool have = j < size;
      const float v = have ? d[o + j] : 0.f;
      const uint32_t g = have ? (uint32_t)a.list[s0 + j] : 0u;
      rt_offer(rt_key(v, g), have, mine, kth, lane, k);
    }
  }
  if (lane < RT_MAX_K) sl[wave][lane] = mine;
  __syncthreads();
  if (wave == 0) {
    for (int w = 1; w < 4; ++w)
      for (int j = 0; j < k; ++j) rt_insert(sl[w][j], mine, lane, k);
    if (lane < k) {
      idx[(int64_t)row * k + lane] = mine == RT_NOKEY ? -1 : (int32_t)(uint32_t)mine;
      dst[(int64_t)row * k + lane] = mine == RT_NOKEY ? 0.f : rt_key_dist(mine);
    }
  }
}
void launch_ivf_select(const IvfBlock& b, int k, int32_t* idx, float* dist, hipStream_t s) {
  hipLaunchKernelGGL(k_ivf_select, dim3((unsigned)b.rows), dim3(256), 0, s, b, k, idx, dist);
}

}  // namespace vv
