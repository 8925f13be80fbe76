// ivf_coarse.hip -- the coarse index and the search loop under every inverted-file index (vv_ivf_coarse.h; the entry points are ivf.hip's
// and pq.hip's).  The lists are built by the k-means grouping kernels as they stand, the probe's similarity is launch_sim_f32 as the gallery
// calls run it, probe and selection are kernels_ivf.hip's.  A search queues everything on the context's stream with no host wait between
// its blocks and synchronises once, at its end.  None of this reads or writes the training step's state.  HAS NO REFERENCE COUNTERPART.
#include <algorithm>

#include "vv_ivf_coarse.h"

namespace vv {

int coarse_check(const char* who, vv_ctx* c, vv_gallery* items, const float* centroids,
                 std::initializer_list<std::pair<const char*, const void*>> more, int C, int metric, GalleryRows* gr) {
  if (!c) return fail(VV_ERR_ARG, "%s: ctx is NULL", who);
  if (!items) return fail(VV_ERR_ARG, "%s: items is NULL", who);
  if (!centroids) return fail(VV_ERR_ARG, "%s: centroids is NULL", who);
  for (const auto& p : more)
    if (!p.second) return fail(VV_ERR_ARG, "%s: %s is NULL", who, p.first);
  *gr = gallery_rows(items);
  if (gr->ctx != c) return fail(VV_ERR_ARG, "%s: the items gallery belongs to another context", who);
  if (C < 1 || C > KM_MAX_CLUSTERS) return fail(VV_ERR_ARG, "%s: C = %d is outside 1 .. %d", who, C, KM_MAX_CLUSTERS);
  if (C > gr->n_ref) return fail(VV_ERR_ARG, "%s: C = %d exceeds the gallery's %lld items", who, C, (long long)gr->n_ref);
  if (metric != VV_KMEANS_EUCLIDEAN && metric != VV_KMEANS_SPHERICAL) return fail(VV_ERR_ARG, "%s: unknown metric %d", who, metric);
  return VV_OK;
}

int coarse_assign(const char* who, vv_ctx* c, vv_gallery* items, const GalleryRows& gr, const float* centroids, int C, int metric,
                  const int32_t** assign, std::vector<int32_t>* own) {
  const int64_t n = gr.n_ref;
  if (*assign) {
    for (int64_t i = 0; i < n; ++i)
      if ((*assign)[i] < 0 || (*assign)[i] >= C)
        return fail(VV_ERR_ARG, "%s: assign[%lld] = %d is outside 0 .. %d", who, (long long)i, (*assign)[i], C - 1);
    return VV_OK;
  }
  // what vv_gallery_kmeans with iters = 0 returns for these centroids and this metric: that call, not a restatement of it
  vv_kmeans_cfg cfg;
  vv_kmeans_cfg_default(&cfg);
  cfg.num_clusters = C; cfg.iters = 0; cfg.metric = metric;
  own->assign((size_t)n, 0);
  std::vector<float> cent_back((size_t)C * gr.dim);
  vv_kmeans_report rep;
  const int rc = vv_gallery_kmeans(c, items, &cfg, centroids, nullptr, cent_back.data(), own->data(), nullptr, nullptr, nullptr, &rep);
  if (rc) return rc;
  for (int64_t i = 0; i < n; ++i)
    if ((*own)[i] < 0 || (*own)[i] >= C) return fail(VV_ERR_STATE, "%s: the assignment pass left item %lld in cluster %d", who, (long long)i, (*own)[i]);
  *assign = own->data();
  return VV_OK;
}

int coarse_build(const char* who, IvfCoarse* ix, const float* centroids, const int32_t* assign) {
  const int64_t n = ix->n_ref;
  const int C = ix->C, Dp = ix->Dp, dim = ix->dim;
  hipStream_t s = ix->ctx->stream;
  const int64_t tiles = (n + KM_TILE - 1) / KM_TILE, max_chunks = n / KM_CHUNK + std::min<int64_t>(C, n);
  std::vector<int32_t> hcounts((size_t)C, 0);
  for (int64_t i = 0; i < n; ++i) ++hcounts[assign[i]];
  HIPCHK(hipMalloc((void**)&ix->cent, (size_t)C * Dp * 4)); HIPCHK(hipMalloc((void**)&ix->nn, (size_t)C * 4));
  HIPCHK(hipMalloc((void**)&ix->start, ((size_t)C + 1) * 4)); HIPCHK(hipMalloc((void**)&ix->list, (size_t)n * 4));
  DevTmp<int32_t> dassign, counts, hist, cbase, nchunks; DevTmp<int4> chunks; DevTmp<KmRec> rec;
  HIPCHK(dassign.alloc((size_t)n)); HIPCHK(counts.alloc((size_t)C)); HIPCHK(hist.alloc((size_t)tiles * C)); HIPCHK(cbase.alloc((size_t)C + 1));
  HIPCHK(nchunks.alloc(1)); HIPCHK(chunks.alloc((size_t)max_chunks)); HIPCHK(rec.alloc(1));
  HIPCHK(hipMemcpyAsync(dassign, assign, (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(counts, hcounts.data(), (size_t)C * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(rec, 0, sizeof(KmRec), s));
  // the lists: every cluster's items in ascending item index, the stable counting sort k-means runs
  launch_km_group(dassign, n, C, tiles, counts, hist, ix->start, cbase, chunks, max_chunks, nchunks, ix->list, rec, s);
  // the centroids, and under EUCLIDEAN nn_c as k-means forms it for centroids it is given
  if (Dp != dim) HIPCHK(hipMemsetAsync(ix->cent, 0, (size_t)C * Dp * 4, s));
  HIPCHK(hipMemcpy2DAsync(ix->cent, (size_t)Dp * 4, centroids, (size_t)dim * 4, (size_t)dim * 4, (size_t)C, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(ix->nn, 0, (size_t)C * 4, s));
  if (ix->metric == VV_KMEANS_EUCLIDEAN) launch_km_finish(nullptr, Dp, dim, nullptr, nullptr, 0, C, 1, 1, ix->cent, ix->nn, rec, s);
  HIPCHK(hipGetLastError());
  ix->h_start.assign((size_t)C + 1, 0);
  HIPCHK(hipMemcpyAsync(ix->h_start.data(), ix->start, ((size_t)C + 1) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int k = 0; k < C; ++k) {
    if (ix->h_start[k + 1] - ix->h_start[k] != hcounts[k]) return fail(VV_ERR_STATE, "%s: the device's list of cluster %d disagrees with the assignment", who, k);
    ix->largest = std::max(ix->largest, hcounts[k]); ix->empty += hcounts[k] == 0;
  }
  return VV_OK;
}

void coarse_release(IvfCoarse* ix) {
  dfree(ix->cent); dfree(ix->nn); dfree(ix->start); dfree(ix->list); dfree(ix->scratch);
}

int coarse_drain(const char* who, vv_ctx* c, const IvfCoarse* ix) {
  if (!c) return fail(VV_ERR_ARG, "%s: ctx is NULL", who);
  if (!ix) return VV_OK;
  if (ix->ctx != c) return fail(VV_ERR_ARG, "%s: the index belongs to another context", who);
  VV_ENTER(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  return VV_OK;
}

int coarse_lists(const char* who, vv_ctx* c, const IvfCoarse* ix, int32_t* start, int32_t* list) {
  if (!c || !ix || !start || !list) return fail(VV_ERR_ARG, "%s: NULL argument", who);
  if (ix->ctx != c) return fail(VV_ERR_ARG, "%s: the index belongs to another context", who);
  VV_ENTER(c);
  HIPCHK(hipMemcpyAsync(start, ix->start, ((size_t)ix->C + 1) * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(list, ix->list, (size_t)ix->n_ref * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return VV_OK;
}

bool coarse_get(const IvfCoarse& ix, const std::string& n, double* value) {
  if (n == "n_ref") *value = (double)ix.n_ref;
  else if (n == "dim") *value = ix.dim;
  else if (n == "num_clusters") *value = ix.C;
  else if (n == "metric") *value = ix.metric;
  else if (n == "largest_list") *value = ix.largest;
  else if (n == "empty_lists") *value = ix.empty;
  else if (n == "last_blocks") *value = (double)ix.last_blocks;
  else if (n == "last_candidates") *value = (double)ix.last_candidates;
  else if (n == "last_probe_ms") *value = ix.last_ms[0];
  else if (n == "last_select_ms") *value = ix.last_ms[3];
  else if (n == "last_device_ms") *value = ix.last_ms[4];
  else return false;
  return true;
}

int coarse_search(const char* who, vv_ctx* c, IvfCoarse* ix, const float* q, int32_t n_q, int32_t nprobe, int32_t k, int32_t* idx,
                  float* dist, int32_t* n_candidates, const CoarseMiddle& mid, IvfRec* hrec) {
  if (!c) return fail(VV_ERR_ARG, "%s: ctx is NULL", who);
  if (!ix) return fail(VV_ERR_ARG, "%s: index is NULL", who);
  if (!q) return fail(VV_ERR_ARG, "%s: q is NULL", who);
  if (!idx) return fail(VV_ERR_ARG, "%s: idx is NULL", who);
  if (!dist) return fail(VV_ERR_ARG, "%s: dist is NULL", who);
  if (ix->ctx != c) return fail(VV_ERR_ARG, "%s: the index belongs to another context", who);
  if (n_q < 1) return fail(VV_ERR_ARG, "%s: n_q = %d", who, n_q);
  const int C = ix->C, Dp = ix->Dp, dim = ix->dim;
  if (nprobe < 1 || nprobe > C || (nprobe > IVF_MAX_PROBE && nprobe != C))
    return fail(VV_ERR_ARG, "%s: nprobe = %d is neither in 1 .. %d nor the index's %d clusters", who, nprobe, std::min(C, IVF_MAX_PROBE), C);
  if (k < 1 || k > RT_MAX_K) return fail(VV_ERR_ARG, "%s: k = %d is outside 1 .. %d", who, k, RT_MAX_K);
  const CoarsePlan p = mid.plan(ivf_pitch_items(ix->h_start.data(), C, nprobe));
  if (!p.ok) return fail(VV_ERR_ARG, "%s: one query's %d probed lists of %lld items do not fit the scratch limit", who, nprobe, (long long)ix->n_ref);
  VV_ENTER(c);
  hipStream_t s = c->stream;
  if (p.total_bytes > ix->scratch_cap) {
    HIPCHK(hipStreamSynchronize(s));
    dfree(ix->scratch); ix->scratch = nullptr; ix->scratch_cap = 0;
    HIPCHK(hipMalloc((void**)&ix->scratch, p.total_bytes));
    ix->scratch_cap = p.total_bytes;
  }
  // the one allocation carved up: every buffer on IVF_ALIGN bytes (the plan counts mid.buffers of them)
  size_t used = 0; int taken = 0;
  const std::function<void*(size_t)> take = [&](size_t bytes) {
    char* at = ix->scratch + used; used += (bytes + IVF_ALIGN - 1) / IVF_ALIGN * IVF_ALIGN; ++taken; return (void*)at;
  };
  const size_t R = (size_t)p.block_rows, P = R * nprobe;
  float* score = (float*)take(R * C * 4);
  CoarseBlock bb;
  bb.qdev = (float*)take(R * Dp * 4); bb.cand = (float*)take(R * p.pitch * 4); bb.m = (int32_t*)take(R * 4);
  int32_t* oidx = (int32_t*)take(R * RT_MAX_K * 4); float* odist = (float*)take(R * RT_MAX_K * 4);
  bb.probe = (int32_t*)take(P * 4); bb.off = (int32_t*)take(P * 4); bb.counts = (int32_t*)take((size_t)C * 4);
  bb.rec = (IvfRec*)take(sizeof(IvfRec)); bb.rows = 0;
  mid.carve(take);
  if (used > ix->scratch_cap || taken > mid.buffers) return fail(VV_ERR_STATE, "%s: %zu bytes in %d buffers pass the plan's %zu", who, used, taken, p.total_bytes);

  // events at the boundaries of the first IVF_TIMED_BLOCKS blocks' four legs (a call of more blocks reports those scaled to all), and
  // around the whole call
  const int64_t tb = std::min<int64_t>(p.blocks, IVF_TIMED_BLOCKS);
  CallEvents ev;
  HIPCHK(ev.create((size_t)(5 * tb + 2)));
  const size_t e_begin = (size_t)(5 * tb), e_end = e_begin + 1;
  const int all = nprobe == C, euclid = ix->metric == VV_KMEANS_EUCLIDEAN;

  HIPCHK(hipEventRecord(ev.e[e_begin], s));
  HIPCHK(hipMemsetAsync(bb.rec, 0, sizeof(IvfRec), s));
  if (mid.begin) { const int rc = mid.begin(); if (rc) return rc; }
  if (Dp != dim) HIPCHK(hipMemsetAsync(bb.qdev, 0, R * Dp * 4, s));           // the K padding of the query rows stays zero over the blocks
  for (int64_t b = 0; b < p.blocks; ++b) {
    const int64_t q0 = b * p.block_rows;
    const int rows = bb.rows = (int)std::min<int64_t>(p.block_rows, n_q - q0);
    const bool timed = b < tb;
    hipEvent_t* e = timed ? &ev.e[(size_t)(5 * b)] : nullptr;
    if (timed) HIPCHK(hipEventRecord(e[0], s));
    // 1. probe, on full-dimension rows
    HIPCHK(hipMemcpy2DAsync(bb.qdev, (size_t)Dp * 4, q + (size_t)q0 * dim, (size_t)dim * 4, (size_t)dim * 4, (size_t)rows, hipMemcpyHostToDevice, s));
    launch_sim_f32(bb.qdev, ix->cent, score, rows, C, Dp, C, s);
    HIPCHK(hipMemsetAsync(bb.counts, 0, (size_t)C * 4, s));
    launch_ivf_probe(score, rows, C, nprobe, all, euclid, ix->nn, ix->start, bb.probe, bb.off, bb.m, bb.counts, bb.rec, s);
    if (timed) HIPCHK(hipEventRecord(e[1], s));
    // 2. and 3. the middle's legs, e[2] between them and e[3] behind; of the block k_ivf_select reads the candidates, the pairs and the lists
    IvfBlock blk = {};
    blk.Q = bb.qdev; blk.start = ix->start; blk.list = ix->list; blk.probe = bb.probe; blk.off = bb.off; blk.cand = bb.cand;
    blk.pitch = p.pitch; blk.rows = rows; blk.Dp = Dp; blk.C = C; blk.nprobe = nprobe;
    hipEvent_t e2 = timed ? e[2] : nullptr;
    const int rc = mid.block(bb, [e2, s]() { return e2 ? hipEventRecord(e2, s) : hipSuccess; }, &blk);
    if (rc) return rc;
    if (timed) HIPCHK(hipEventRecord(e[3], s));
    // 4. select
    launch_ivf_select(blk, k, oidx, odist, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(idx + (size_t)q0 * k, oidx, (size_t)rows * k * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(dist + (size_t)q0 * k, odist, (size_t)rows * k * 4, hipMemcpyDeviceToHost, s));
    if (n_candidates) HIPCHK(hipMemcpyAsync(n_candidates + q0, bb.m, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
    if (timed) HIPCHK(hipEventRecord(e[4], s));
  }
  HIPCHK(hipMemcpyAsync(hrec, bb.rec, sizeof(IvfRec), hipMemcpyDeviceToHost, s));
  HIPCHK(hipEventRecord(ev.e[e_end], s));
  HIPCHK(hipStreamSynchronize(s));                                       // the call's one wait

  double leg[4] = {0, 0, 0, 0};
  for (int64_t b = 0; b < tb; ++b)
    for (int l = 0; l < 4; ++l) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, ev.e[(size_t)(5 * b + l)], ev.e[(size_t)(5 * b + l + 1)]));
      leg[l] += ms;
    }
  float total = 0;
  HIPCHK(hipEventElapsedTime(&total, ev.e[e_begin], ev.e[e_end]));
  for (int l = 0; l < 4; ++l) ix->last_ms[l] = leg[l] * (double)p.blocks / (double)tb;
  ix->last_ms[4] = total;
  ix->last_blocks = p.blocks; ix->last_candidates = hrec->candidates;
  return VV_OK;
}

}  // namespace vv
