// vv_pq_plan.h -- the limits of product quantisation (pq.hip: vv_pq_train, vv_pq_encode, vv_ivfpq_*) and the sizes of vv_ivfpq_search's
// device buffers: the floats of one query's look-up table, the bytes of one code row and the form k_pq_scan reads it in, the rows of one
// query block, and the bytes of everything together.  pq.hip checks, allocates and launches by these numbers alone.  A pure function of
// the shapes, of the index's list sizes (through vv_ivf_plan.h's ivf_pitch_items) and of the "ivf_block_rows" option: no allocation, no
// device property.  No HIP header: a host compiler builds this alone (tools/pq_plan_check.cc).
#pragma once
#include <cstddef>
#include <cstdint>

#include "vv_ivf_plan.h"

namespace vv {

constexpr int PQ_MAX_M = 64;              // sub-spaces at most
constexpr int PQ_MAX_KSUB = 256;          // codewords of one sub-space at most: a code is one byte
constexpr size_t PQ_LDS_BYTES = 65536;    // one query's whole table, M * ksub floats, at most: k_pq_scan holds it in LDS
constexpr int PQ_BUFFERS = 12;            // buffers carved out of the one scratch allocation at most, each on IVF_ALIGN bytes

// 0: the shape is legal; else which argument is not -- 1: M (outside 1 .. 64), 2: dim % M, 3: ksub (outside 2 .. 256), 4: M * ksub * 4
// passes the LDS limit
inline int pq_shape_error(int dim, int M, int ksub) {
  if (M < 1 || M > PQ_MAX_M) return 1;
  if (dim < 1 || dim % M != 0) return 2;
  if (ksub < 2 || ksub > PQ_MAX_KSUB) return 3;
  if ((size_t)M * ksub * 4 > PQ_LDS_BYTES) return 4;
  return 0;
}
// how k_pq_scan loads a code row -- 1: 16 bytes at a time (M % 16 == 0), 2: 4 bytes (M % 4 == 0), 3: bytes; and the bytes between two
// rows of the code slab: M itself in every form, since the slab's base is on 256 bytes and M a multiple of the load's size
inline int pq_scan_form(int M) { return M % 16 == 0 ? 1 : M % 4 == 0 ? 2 : 3; }
inline int pq_code_row_bytes(int M) { return M; }
// floats between two queries' tables in scratch: M * ksub rounded up to 4, so that every table starts on 16 bytes
inline int64_t pq_table_floats(int M, int ksub) { return ((int64_t)M * ksub + 3) / 4 * 4; }

struct PqPlan {
  int ok = 0;                             // 0: not even one query row fits the scratch limit (or an argument is out of range)
  int Dp = 0, dsub = 0, form = 0;
  int64_t table = 0;                      // pq_table_floats
  int64_t pitch = 0;                      // floats between two candidate rows: vv_ivf_plan.h's
  int64_t block_rows = 0, blocks = 0;
  int64_t pairs = 0;                      // block_rows * nprobe
  size_t total_bytes = 0;
};

// every byte a block of `rows` queries needs: per row the probe scores, the query's padded copy, its table, the candidates, m and the
// k <= 32 results; per pair the probed cluster and its offset; the clusters' pair counts, the call's record, the buffers' alignment
inline size_t pq_block_bytes(int64_t rows, int64_t pitch, int Dp, int C, int nprobe, int64_t table) {
  return (size_t)rows * ((size_t)C * 4 + (size_t)Dp * 4 + (size_t)table * 4 + (size_t)pitch * 4 + 4 + (size_t)RT_MAX_K * 8 + (size_t)nprobe * 8) +
         (size_t)C * 4 + IVF_REC_BYTES + PQ_BUFFERS * IVF_ALIGN;
}

// pitch_items: ivf_pitch_items of the index and this nprobe; forced_block_rows: the "ivf_block_rows" option (0: the plan's choice)
inline PqPlan pq_plan(int64_t n_ref, int dim, int C, int nprobe, int64_t n_q, int64_t pitch_items, int M, int ksub, int64_t forced_block_rows) {
  PqPlan p;
  if (pq_shape_error(dim, M, ksub) || !plan_head(p, n_ref, dim, C, nprobe, n_q, pitch_items)) return p;
  p.dsub = dim / M; p.form = pq_scan_form(M);
  p.table = pq_table_floats(M, ksub);
  const size_t fixed = pq_block_bytes(0, p.pitch, p.Dp, C, nprobe, p.table), per_row = pq_block_bytes(1, p.pitch, p.Dp, C, nprobe, p.table) - fixed;
  if (fixed + per_row > GALLERY_SCRATCH_MAX) return p;
  plan_rows(p, (int64_t)((GALLERY_SCRATCH_MAX - fixed) / per_row), forced_block_rows, n_q, nprobe);
  p.total_bytes = pq_block_bytes(p.block_rows, p.pitch, p.Dp, C, nprobe, p.table);
  p.ok = 1;
  return p;
}

}  // namespace vv
