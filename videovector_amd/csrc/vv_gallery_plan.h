// vv_gallery_plan.h -- the sizes of the gallery path's scratch (retrieval.hip): a gallery's shape-dependent constants, the bytes of one
// scratch row, the rows of one query block.  gallery_init, gallery_ensure_scratch and every query call ask these functions, so the block
// a call sizes and the limit the allocation checks cannot disagree.  Pure functions of the values below: no allocation, no gallery
// pointer.  No HIP header: a host compiler builds this alone (tools/gallery_plan_check.cc).
#pragma once
#include <cstddef>
#include <cstdint>

namespace vv {

constexpr int RT_BK = 32;                 // K of the similarity tile; operand rows are padded to a multiple of RT_BK floats
constexpr int RT_CHUNK = 2048;            // positives of one query ranked per pass (their sorted keys: 16 KiB of LDS)
constexpr int RT_MAX_K = 32;
constexpr int RT_SEL_BINS = 4096;
constexpr int RT_SEL_LAST_BINS = 256;
constexpr size_t GALLERY_ACC_BYTES = 24;  // the per-query accumulator (vv_internal.h: RankAcc, ClassAcc -- they share the buffer)
constexpr size_t GALLERY_SCRATCH_MAX = (size_t)1 << 30;                         // every device buffer a query call needs, together
constexpr size_t GALLERY_DIST_MAX = GALLERY_SCRATCH_MAX - ((size_t)40 << 20);   // ... of which the distances
constexpr int GALLERY_QB_MAX = 512;                                             // rows of one query block at most
constexpr int GALLERY_SEG_MAX = 64;                                             // gallery segments (workgroups) per row at most

struct GalleryShape {
  int64_t pitch = 0;                     // floats between two rows of the distance scratch (n_ref rounded up to 64)
  int Dp = 0;
  int seg = 0, S = 0;                    // row kernels: items per workgroup (multiple of 1024), workgroups per row
  int qb_max = 0;                        // rows of a query block the scratch limit allows for this gallery; 0: not even one
};
inline GalleryShape gallery_shape(int64_t n_ref, int dim) {
  GalleryShape s;
  s.Dp = (dim + RT_BK - 1) / RT_BK * RT_BK; s.pitch = (n_ref + 63) / 64 * 64;
  int64_t seg = ((n_ref + GALLERY_SEG_MAX - 1) / GALLERY_SEG_MAX + 1023) / 1024 * 1024;
  if (seg < 16384) seg = 16384;
  s.seg = (int)seg; s.S = (int)((n_ref + seg - 1) / seg);
  const size_t fit = GALLERY_DIST_MAX / ((size_t)s.pitch * 4);
  s.qb_max = (int)(fit < (size_t)GALLERY_QB_MAX ? fit : (size_t)GALLERY_QB_MAX);
  return s;
}

// Bytes of one scratch row.  cls: the call is vv_gallery_class_stats, which needs skeys / cbins as well; sel: the selection form of
// vv_gallery_nearest*, which needs skeys (its candidate keys: counted once with both flags) and its own buffers
inline size_t gallery_row_bytes(const GalleryShape& s, bool cls, bool sel) {
  size_t b = (size_t)s.pitch * 4 + (size_t)s.Dp * 4 + (size_t)s.S * RT_MAX_K * 8 + (size_t)2 * RT_CHUNK * 4 +      // dist, qdev, part, bins
             (size_t)2 * RT_MAX_K * 4 + 3 * 4 + GALLERY_ACC_BYTES;                                              // out_idx / out_dist, pstart / pcount / qids, acc
  if (cls || sel) b += (size_t)RT_CHUNK * 8;                                                                    // skeys
  if (cls) b += (size_t)3 * RT_CHUNK * 4;                                                                       // cbins
  // the selection form: state, digit histogram, the segments' last-digit histograms, the lists
  if (sel) b += 4 * 4 + (size_t)RT_SEL_BINS * 4 + (size_t)s.S * RT_SEL_LAST_BINS * 4 + (size_t)2 * RT_CHUNK * 4;
  return b;
}
// Rows of one query block of a call with n_q queries: the gallery's own, fewer where the class / selection buffers would pass the
// scratch limit; 0: not even one row fits.  (Without a flag the second bound never binds: GALLERY_DIST_MAX leaves 40 MiB, and 512 rows
// of everything but the distances take under 33 -- tests/test_gallery_plan_host.py.)
inline int gallery_block_rows(const GalleryShape& s, int64_t n_q, bool cls, bool sel) {
  size_t rows = GALLERY_SCRATCH_MAX / gallery_row_bytes(s, cls, sel);
  if ((size_t)s.qb_max < rows) rows = (size_t)s.qb_max;
  return (int)((size_t)n_q < rows ? (size_t)n_q : rows);
}

}  // namespace vv
