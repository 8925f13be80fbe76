// vv_kmeans_plan.h -- the sizes of vv_gallery_kmeans' device buffers (kmeans.hip): the rows of one score block, the tiles of the grouping,
// the slots of the objective, the chunks of the centroid sum, and the bytes of everything the call allocates.  kmeans.hip allocates and
// launches by these numbers alone, so the block a call sizes and the limit it checks cannot disagree.  A pure function of the shapes and
// of the "km_block_rows" option: no allocation, no device property.  No HIP header: a host compiler builds this alone
// (tools/kmeans_plan_check.cc).
#pragma once
#include <cstddef>
#include <cstdint>

#include "vv_gallery_plan.h"

namespace vv {

constexpr int KM_MAX_CLUSTERS = 4096;
constexpr int KM_CHUNK = 256;             // list entries of one partial sum (a serial fp32 chain): part of the call's arithmetic
constexpr int KM_SLOT_ROWS = 64;          // items of one k_km_assign workgroup = of one objective slot: part of the call's arithmetic
constexpr int KM_TILE = 1024;             // items of one grouping tile (one histogram row, one scatter workgroup)
constexpr int KM_SLICE = 512;             // columns of one k_km_partial workgroup
constexpr int KM_TIMED_BLOCKS = 1024;     // blocks of the timed iteration whose similarity / assign legs get events of their own at most
constexpr size_t KM_REC_BYTES = 40;       // one pass's record (vv_internal.h: KmRec)
constexpr size_t KM_SCORE_TARGET = (size_t)64 << 20;   // the score block the plan aims at: small enough that k_km_assign finds it in the cache

struct KmeansPlan {
  int ok = 0;                             // 0: not even a block of KM_SLOT_ROWS rows fits the scratch limit
  int Dp = 0;
  int64_t block_rows = 0, blocks = 0;     // rows of one score block (a multiple of KM_SLOT_ROWS), blocks of one pass
  int64_t tiles = 0, slots = 0;           // grouping tiles, objective slots
  int64_t max_chunks = 0;                 // chunks of one update at most: floor(n / KM_CHUNK) + min(C, n)
  int slices = 0;                         // column slices of the partial sums
  size_t score_bytes = 0, item_bytes = 0, partial_bytes = 0, total_bytes = 0;
};

// forced_block_rows: the "km_block_rows" option (0: the plan's choice); rounded up to a multiple of KM_SLOT_ROWS, cut to what fits
inline KmeansPlan kmeans_plan(int64_t n, int dim, int C, int64_t forced_block_rows) {
  KmeansPlan p;
  if (n < 1 || dim < 1 || C < 1 || C > KM_MAX_CLUSTERS) return p;
  p.Dp = (dim + RT_BK - 1) / RT_BK * RT_BK;
  p.tiles = (n + KM_TILE - 1) / KM_TILE;
  p.slots = (n + KM_SLOT_ROWS - 1) / KM_SLOT_ROWS;
  p.max_chunks = n / KM_CHUNK + ((int64_t)C < n ? (int64_t)C : n);
  p.slices = (p.Dp + KM_SLICE - 1) / KM_SLICE;
  // per item: assign, list; per tile: a histogram row; per slot: a double; per cluster: the centroid row, counts / nn / start /
  // chunk base / chunk count; per chunk: its table entry; 4096: the record's head and the allocations' alignment
  p.item_bytes = (size_t)n * 8 + (size_t)p.tiles * C * 4 + (size_t)p.slots * 8 + (size_t)C * p.Dp * 4 + (size_t)C * 24 +
                 (size_t)p.max_chunks * 16 + 4096;
  p.partial_bytes = (size_t)p.max_chunks * p.Dp * 4;
  const size_t fixed = p.item_bytes + p.partial_bytes, row = (size_t)C * 4;
  if (fixed + row * KM_SLOT_ROWS > GALLERY_SCRATCH_MAX) return p;
  const int64_t n_up = (n + KM_SLOT_ROWS - 1) / KM_SLOT_ROWS * KM_SLOT_ROWS;
  int64_t rows = forced_block_rows > 0 ? (forced_block_rows + KM_SLOT_ROWS - 1) / KM_SLOT_ROWS * KM_SLOT_ROWS
                                       : (int64_t)(KM_SCORE_TARGET / row) / KM_SLOT_ROWS * KM_SLOT_ROWS;
  if (rows < KM_SLOT_ROWS) rows = KM_SLOT_ROWS;
  if (rows > n_up) rows = n_up;
  const int64_t fit = (int64_t)((GALLERY_SCRATCH_MAX - fixed) / row) / KM_SLOT_ROWS * KM_SLOT_ROWS;
  if (rows > fit) rows = fit;
  if (rows > ((int64_t)1 << 24)) rows = (int64_t)1 << 24;      // (one similarity launch: its grid and its int row count)
  p.block_rows = rows; p.blocks = (n + rows - 1) / rows;
  p.score_bytes = (size_t)rows * row;
  p.total_bytes = fixed + p.score_bytes;
  p.ok = 1;
  return p;
}

// the traces' device record, iters + 1 entries: apart from the plan (it depends on iters, not on shapes), inside the same limit --
// vv_gallery_kmeans refuses a call whose plan and record together pass GALLERY_SCRATCH_MAX
inline size_t kmeans_record_bytes(int64_t iters) { return (size_t)(iters + 1) * KM_REC_BYTES; }

}  // namespace vv
