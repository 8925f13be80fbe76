// vv_ivf_plan.h -- the sizes of vv_ivf_search's device buffers (ivf.hip on ivf_coarse.hip): the candidate pitch, the rows of one query block, the pairs of a
// block and what their grouping needs, the capacity of the tile table, the grid of the grouped similarity, and the bytes of everything
// together.  The search allocates and launches by these numbers alone, so the block a call sizes and the limit it checks cannot disagree.
// A pure function of the shapes, of the index's list sizes (through ivf_pitch_items) and of the "ivf_block_rows" / "ivf_grid_wgs"
// options: no allocation, no device property.  No HIP header: a host compiler builds this alone (tools/ivf_plan_check.cc).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "vv_kmeans_plan.h"

namespace vv {

constexpr int IVF_MAX_PROBE = 64;         // nprobe at most, unless nprobe == num_clusters (k_ivf_probe keeps one selected cluster per lane)
constexpr int IVF_TILE = 128;             // rows and columns of one similarity tile (vv_internal.h: RT_BM, RT_BN)
constexpr int IVF_GRID_WGS = 512;         // workgroups of the grouped similarity's persistent grid: the plan's choice (a constant, not the device's CU count)
constexpr int IVF_GRID_MAX = 65535;       // ... and the most "ivf_grid_wgs" may ask for
constexpr int64_t IVF_BLOCK_ROWS_MAX = 65536;   // rows of one query block at most (block_rows * nprobe pairs stay far below 2^31)
constexpr int IVF_TIMED_BLOCKS = 64;      // blocks of a call whose legs get events of their own at most
constexpr size_t IVF_REC_BYTES = 16;      // the call's device record (vv_internal.h: IvfRec)
constexpr int IVF_BUFFERS = 20;           // buffers carved out of the one scratch allocation at most, each on IVF_ALIGN bytes
constexpr size_t IVF_ALIGN = 256;

// The sum of the nprobe largest list sizes: no query's candidate row is longer.  start: [C + 1], ascending.
inline int64_t ivf_pitch_items(const int32_t* start, int C, int nprobe) {
  std::vector<int32_t> size((size_t)C);
  for (int c = 0; c < C; ++c) size[c] = start[c + 1] - start[c];
  const int m = nprobe < C ? nprobe : C;
  std::partial_sort(size.begin(), size.begin() + m, size.end(), [](int32_t a, int32_t b) { return a > b; });
  int64_t s = 0;
  for (int p = 0; p < m; ++p) s += size[p];
  return s;
}

struct IvfPlan {
  int ok = 0;                             // 0: not even one query row fits the scratch limit
  int Dp = 0;
  int64_t pitch = 0;                      // floats between two candidate rows: pitch_items rounded up to 4, 4 at least
  int64_t block_rows = 0, blocks = 0;     // query rows of one block, blocks of the call
  int64_t pairs = 0;                      // (query, cluster) pairs of a full block: block_rows * nprobe
  int64_t pair_tiles = 0, max_chunks = 0; // what the counting sort of the pairs needs (k_km_hist's tiles, k_km_starts' chunk table)
  int64_t tile_cap = 0;                   // entries of the tile table
  int grid_wgs = 0;
  size_t total_bytes = 0;
};

// What ivf_plan and vv_pq_plan.h's pq_plan share, on either plan struct.  The head: the argument check, Dp and the pitch; 0: an argument is
// out of range, nothing is written.
template <class Plan>
inline int plan_head(Plan& p, int64_t n_ref, int dim, int C, int nprobe, int64_t n_q, int64_t pitch_items) {
  if (n_ref < 1 || dim < 1 || C < 1 || C > KM_MAX_CLUSTERS || n_q < 1 || pitch_items < 0 || pitch_items > n_ref) return 0;
  if (nprobe < 1 || nprobe > C || (nprobe > IVF_MAX_PROBE && nprobe != C)) return 0;
  p.Dp = (dim + RT_BK - 1) / RT_BK * RT_BK;
  p.pitch = (pitch_items + 3) / 4 * 4;
  if (p.pitch < 4) p.pitch = 4;
  return 1;
}
// ... and the row clamp: of the `fit` rows the scratch limit admits, the forced number if it is smaller, IVF_BLOCK_ROWS_MAX and n_q at most
template <class Plan>
inline void plan_rows(Plan& p, int64_t fit, int64_t forced_block_rows, int64_t n_q, int nprobe) {
  int64_t rows = fit;
  if (forced_block_rows > 0 && forced_block_rows < rows) rows = forced_block_rows;
  if (rows > IVF_BLOCK_ROWS_MAX) rows = IVF_BLOCK_ROWS_MAX;
  if (rows > n_q) rows = n_q;
  p.block_rows = rows; p.blocks = (n_q + rows - 1) / rows;
  p.pairs = rows * nprobe;
}

// Tiles of one block at most.  Cluster c with a_c >= 1 queries and b_c >= 1 items gives ceil(a_c / 128) ceil(b_c / 128) tiles, and
// ceil(x / 128) <= x / 128 + 1 - 1 / 128 < x / 128 + 1, so it gives fewer than a_c b_c / 16384 + a_c / 128 + b_c / 128 + 1.  Summed over the
// clusters that have both: sum a_c b_c = sum of the block's candidate counts m_i <= rows * pitch (no m_i exceeds the nprobe largest
// lists); sum a_c = pairs; sum b_c <= n_ref; and at most min(C, pairs) clusters have a query.  Each term rounded up on its own:
inline int64_t ivf_tile_cap(int64_t rows, int64_t pitch, int64_t pairs, int64_t n_ref, int C) {
  const int64_t t = IVF_TILE, tt = (int64_t)IVF_TILE * IVF_TILE;
  return (rows * pitch + tt - 1) / tt + (pairs + t - 1) / t + (n_ref + t - 1) / t + ((int64_t)C < pairs ? (int64_t)C : pairs);
}

// every byte a block of `rows` queries needs: per row the probe scores, the query's padded copy, the candidates, m and the k <= 32 results;
// per pair the probed cluster, its offset and its place in the grouping; the grouping's histogram, chunk table and per-cluster arrays
// (counts, start, chunk base); the tile table; the records and the buffers' alignment
inline size_t ivf_block_bytes(int64_t rows, int64_t pitch, int Dp, int C, int nprobe, int64_t n_ref) {
  const int64_t pairs = rows * nprobe, pair_tiles = (pairs + KM_TILE - 1) / KM_TILE;
  const int64_t max_chunks = pairs / KM_CHUNK + ((int64_t)C < pairs ? (int64_t)C : pairs);
  return (size_t)rows * ((size_t)C * 4 + (size_t)Dp * 4 + (size_t)pitch * 4 + 4 + (size_t)RT_MAX_K * 8) + (size_t)pairs * 12 +
         (size_t)pair_tiles * C * 4 + (size_t)max_chunks * 16 + ((size_t)3 * C + 2) * 4 +
         (size_t)ivf_tile_cap(rows, pitch, pairs, n_ref, C) * 16 + KM_REC_BYTES + IVF_REC_BYTES + 8 + IVF_BUFFERS * IVF_ALIGN;
}

// pitch_items: ivf_pitch_items of the index and this nprobe; forced_block_rows / forced_grid_wgs: the options (0: the plan's choice)
inline IvfPlan ivf_plan(int64_t n_ref, int dim, int C, int nprobe, int64_t n_q, int64_t pitch_items, int64_t forced_block_rows,
                        int64_t forced_grid_wgs) {
  IvfPlan p;
  if (!plan_head(p, n_ref, dim, C, nprobe, n_q, pitch_items)) return p;
  p.grid_wgs = forced_grid_wgs > 0 ? (int)(forced_grid_wgs < IVF_GRID_MAX ? forced_grid_wgs : IVF_GRID_MAX) : IVF_GRID_WGS;
  // an upper bound of ivf_block_bytes that is linear in the rows -- every ceiling above costs at most one more unit -- solved for them
  const size_t per_row = (size_t)C * 4 + (size_t)p.Dp * 4 + (size_t)p.pitch * 4 + 4 + (size_t)RT_MAX_K * 8 + (size_t)nprobe * 12 +
                         ((size_t)nprobe * C * 4 + KM_TILE - 1) / KM_TILE + ((size_t)nprobe * 16 + KM_CHUNK - 1) / KM_CHUNK +
                         ((size_t)p.pitch * 16 + (size_t)IVF_TILE * IVF_TILE - 1) / ((size_t)IVF_TILE * IVF_TILE) +
                         ((size_t)nprobe * 16 + IVF_TILE - 1) / IVF_TILE;
  const size_t fixed = (size_t)C * 4 + (size_t)C * 16 + ((size_t)3 * C + 2) * 4 + ((size_t)(n_ref + IVF_TILE - 1) / IVF_TILE + 2 + (size_t)C) * 16 +
                       KM_REC_BYTES + IVF_REC_BYTES + 8 + IVF_BUFFERS * IVF_ALIGN;
  if (fixed + per_row > GALLERY_SCRATCH_MAX) return p;
  plan_rows(p, (int64_t)((GALLERY_SCRATCH_MAX - fixed) / per_row), forced_block_rows, n_q, nprobe);
  const int64_t rows = p.block_rows;
  p.pair_tiles = (p.pairs + KM_TILE - 1) / KM_TILE;
  p.max_chunks = p.pairs / KM_CHUNK + ((int64_t)C < p.pairs ? (int64_t)C : p.pairs);
  p.tile_cap = ivf_tile_cap(rows, p.pitch, p.pairs, n_ref, C);
  p.total_bytes = ivf_block_bytes(rows, p.pitch, p.Dp, C, nprobe, n_ref);
  p.ok = 1;
  return p;
}

}  // namespace vv
