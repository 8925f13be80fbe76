// vv_ivf_coarse.h -- what every inverted-file index keeps for its lists and what every search over them does, whatever an index stores
// beside the lists (ivf.hip: fp32 rows; pq.hip: codes and codebooks).  The functions are in ivf_coarse.hip; each takes the entry point's
// name as `who`, so a message begins with the caller's own function.  Internal.
#pragma once
#include <functional>

#include "vv_ctx.h"

namespace vv {

struct IvfCoarse {
  vv_ctx* ctx = nullptr;
  int64_t n_ref = 0;
  int dim = 0, Dp = 0, C = 0, metric = 0;
  float *cent = nullptr, *nn = nullptr;                        // [C][Dp], [C] (EUCLIDEAN)
  int32_t *start = nullptr, *list = nullptr;                   // [C + 1], [n_ref]: position -> item index
  std::vector<int32_t> h_start;                                // host copy of start: the plan's pitch comes from it
  int largest = 0, empty = 0;
  char* scratch = nullptr; size_t scratch_cap = 0;             // one allocation, grown on demand, carved up by every search
  int64_t last_blocks = 0, last_candidates = 0;
  double last_ms[5] = {0, 0, 0, 0, 0};                         // probe, the middle's two legs, select, the whole call
};

// vv_*_create.  The checks before anything is built, in their order: c, items and centroids, then every `more` pointer ({name, pointer}),
// not NULL; the gallery's context; C within 1 .. min(KM_MAX_CLUSTERS, n_ref); the metric.  -> *gr
int coarse_check(const char* who, vv_ctx* c, vv_gallery* items, const float* centroids,
                 std::initializer_list<std::pair<const char*, const void*>> more, int C, int metric, GalleryRows* gr);
// The assignment an index is built on, every entry within 0 .. C - 1: the caller's, or (assign NULL) into `own` what vv_gallery_kmeans with
// iters = 0 returns for these centroids and this metric.  -> *assign
int coarse_assign(const char* who, vv_ctx* c, vv_gallery* items, const GalleryRows& gr, const float* centroids, int C, int metric,
                  const int32_t** assign, std::vector<int32_t>* own);
// The lists, the centroids and nn_c on the device, the host's copy of start compared with the assignment's counts, largest / empty;
// synchronises.  ix holds c and the shape; on an error the caller releases.
int coarse_build(const char* who, IvfCoarse* ix, const float* centroids, const int32_t* assign);
void coarse_release(IvfCoarse* ix);                             // every device allocation above; not ix itself
// vv_*_destroy up to the release: VV_OK with ix NULL, else the index's context checked and its stream drained
int coarse_drain(const char* who, vv_ctx* c, const IvfCoarse* ix);
int coarse_lists(const char* who, vv_ctx* c, const IvfCoarse* ix, int32_t* start, int32_t* list);
// the names every index answers; false: not one of them
bool coarse_get(const IvfCoarse& ix, const std::string& name, double* value);

// What one kind of list supplies to a search.  Per block the shared part copies the queries in and probes, `block` queues the two legs
// in between, the shared part selects and copies the results back.
struct CoarsePlan { int ok; int64_t pitch, block_rows, blocks; size_t total_bytes; };    // of IvfPlan / PqPlan, what the loop reads
struct CoarseBlock {                                           // one block's buffers that the shared part carved, and its rows
  float* qdev; int32_t *probe, *off, *m; float* cand; int32_t* counts; IvfRec* rec; int rows;
};
struct CoarseMiddle {
  int buffers = 0;                                             // buffers of the scratch at most: the plan's IVF_BUFFERS / PQ_BUFFERS
  std::function<CoarsePlan(int64_t pitch_items)> plan;         // the call's plan (kept by the caller), after the argument checks
  std::function<void(const std::function<void*(size_t)>& take)> carve;   // its own buffers out of the scratch, before anything is queued
  std::function<int()> begin;                                  // (may be empty) queued once, behind the record's memset
  // its two legs, `mark` recorded between them, and the fields of blk that only it knows (the shared ones are set, the others zero)
  std::function<int(const CoarseBlock& b, const std::function<hipError_t()>& mark, IvfBlock* blk)> block;
};
// vv_*_search: the argument checks, the scratch, the events, the block loop, the call's one host wait, last_blocks / last_candidates /
// last_ms.  -> *rec: the call's device record
int coarse_search(const char* who, vv_ctx* c, IvfCoarse* ix, const float* q, int32_t n_q, int32_t nprobe, int32_t k, int32_t* idx,
                  float* dist, int32_t* n_candidates, const CoarseMiddle& mid, IvfRec* rec);

}  // namespace vv
