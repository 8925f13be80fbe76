// pq.hip -- entry points of product quantisation on a gallery and of the inverted-file index that keeps product-quantised codes in
// place of the items' rows (include/videovec.h: vv_pq_train, vv_pq_encode, vv_ivfpq_create, vv_ivfpq_destroy, vv_ivfpq_search,
// vv_ivfpq_get, vv_ivfpq_lists, vv_ivfpq_codes).  The kernels are in kernels_pq.hip; a codebook is trained and a code is assigned by
// k-means' own body on a column slice (kmeans.hip: vv_kmeans_rows), the lists are built by the k-means grouping kernels and the probe and
// the selection are the IVF search's (kernels_ivf.hip), all as they stand; the limits and the sizes of every search buffer are
// vv_pq_plan.h's.  A search queues everything on the context's stream with no host wait between its blocks and synchronises once, at
// its end; of the context it reads the ivf_block_rows option.  None of this reads or writes the training step's state.
// HAS NO REFERENCE COUNTERPART.
#include <algorithm>
#include <string>
#include <vector>

#include "vv_ctx.h"

using namespace vv;

struct vv_ivfpq {
  vv_ctx* ctx = nullptr;
  int64_t n_ref = 0;
  int dim = 0, Dp = 0, C = 0, metric = 0, M = 0, ksub = 0, dsub = 0, Mrow = 0;
  uint8_t* codes = nullptr;                                    // [n_ref][Mrow] list-position order
  float *cb = nullptr, *cent = nullptr, *nn = nullptr;         // [M][ksub][dsub], [C][Dp], [C] (EUCLIDEAN)
  int32_t *start = nullptr, *list = nullptr;                   // [C + 1], [n_ref]: position -> item index
  std::vector<int32_t> h_start;                                // host copy of start: the plan's pitch comes from it
  int largest = 0, empty = 0;
  size_t index_bytes = 0;                                      // every device byte above
  char* scratch = nullptr; size_t scratch_cap = 0;             // one allocation, grown on demand, carved up by every search
  int64_t last_blocks = 0, last_candidates = 0; int last_form = 0;
  double last_ms[5] = {0, 0, 0, 0, 0};                         // probe, table, scan, select, the whole call
};

namespace {
struct PqEvents {                                              // events that live for one call
  std::vector<hipEvent_t> e;
  ~PqEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
void pq_release(vv_ivfpq* ix) {
  dfree(ix->codes); dfree(ix->cb); dfree(ix->cent); dfree(ix->nn); dfree(ix->start); dfree(ix->list); dfree(ix->scratch);
  delete ix;
}
// the checks vv_pq_train, vv_pq_encode and vv_ivfpq_create share, on the host: the shape, and that one sub-space's k-means call fits
int pq_check(const char* who, const vv_ctx* c, const GalleryRows& gr, int M, int ksub, int iters) {
  switch (pq_shape_error(gr.dim, M, ksub)) {
    case 1: return fail(VV_ERR_ARG, "%s: M = %d is outside 1 .. %d", who, M, PQ_MAX_M);
    case 2: return fail(VV_ERR_ARG, "%s: M = %d does not divide the gallery's dim = %d", who, M, gr.dim);
    case 3: return fail(VV_ERR_ARG, "%s: ksub = %d is outside 2 .. %d", who, ksub, PQ_MAX_KSUB);
    case 4: return fail(VV_ERR_ARG, "%s: M * ksub * 4 = %d bytes of table pass the %zu of LDS (M = %d, ksub = %d)", who, M * ksub * 4, PQ_LDS_BYTES, M, ksub);
    default: break;
  }
  if (ksub > gr.n_ref) return fail(VV_ERR_ARG, "%s: ksub = %d exceeds the gallery's %lld items", who, ksub, (long long)gr.n_ref);
  if (iters < 0) return fail(VV_ERR_ARG, "%s: iters = %d is negative", who, iters);
  const int dsub = gr.dim / M;
  const KmeansPlan p = kmeans_plan(gr.n_ref, dsub, ksub, c->km_block_rows);
  if (!p.ok || p.total_bytes + kmeans_record_bytes(iters) + (size_t)gr.n_ref * p.Dp * 4 > GALLERY_SCRATCH_MAX)
    return fail(VV_ERR_ARG, "%s: a sub-space of %lld items x %d columns in ksub = %d clusters does not fit the scratch limit", who, (long long)gr.n_ref, dsub, ksub);
  return VV_OK;
}
// code[g][m] for every item and sub-space into dcodes (device [n_ref][M], item order): the column slice, vv_gallery_kmeans' body with
// iters = 0 on it, its assignment packed to bytes -- nothing of the assignment comes back to the host
int pq_encode_device(vv_ctx* c, const GalleryRows& gr, const float* codebooks, int M, int ksub, uint8_t* dcodes) {
  const int64_t n = gr.n_ref;
  const int dsub = gr.dim / M, Dps = (dsub + RT_BK - 1) / RT_BK * RT_BK;
  hipStream_t s = c->stream;
  DevTmp<float> slice; DevTmp<int32_t> dassign;
  HIPCHK(slice.alloc((size_t)n * Dps)); HIPCHK(dassign.alloc((size_t)n));
  std::vector<float> cent_back((size_t)ksub * dsub);
  vv_kmeans_cfg cfg;
  vv_kmeans_cfg_default(&cfg);
  cfg.num_clusters = ksub; cfg.iters = 0; cfg.metric = VV_KMEANS_EUCLIDEAN;
  for (int m = 0; m < M; ++m) {
    launch_pq_slice(gr.feat, n, gr.Dp, m * dsub, dsub, Dps, slice, s);
    HIPCHK(hipGetLastError());
    vv_kmeans_report rep;
    const GalleryRows sub = {slice, n, dsub, Dps, c};
    const int rc = vv_kmeans_rows(c, sub, &cfg, codebooks + (size_t)m * ksub * dsub, nullptr, cent_back.data(), nullptr, nullptr, nullptr, nullptr,
                                  &rep, dassign);
    if (rc) return rc;
    launch_pq_pack(dassign, n, m, M, ksub, dcodes, s);
    HIPCHK(hipGetLastError());
  }
  return VV_OK;
}
int pq_build(vv_ctx* c, vv_ivfpq* ix, const GalleryRows& gr, const float* centroids, const int32_t* assign, const float* codebooks) {
  const int64_t n = ix->n_ref;
  const int C = ix->C, Dp = ix->Dp, dim = ix->dim, M = ix->M;
  hipStream_t s = c->stream;
  const int64_t tiles = (n + KM_TILE - 1) / KM_TILE, max_chunks = n / KM_CHUNK + std::min<int64_t>(C, n);
  const size_t cb_floats = (size_t)M * ix->ksub * ix->dsub;
  std::vector<int32_t> hcounts((size_t)C, 0);
  for (int64_t i = 0; i < n; ++i) ++hcounts[assign[i]];
  HIPCHK(hipMalloc((void**)&ix->codes, (size_t)n * ix->Mrow)); HIPCHK(hipMalloc((void**)&ix->cb, cb_floats * 4));
  HIPCHK(hipMalloc((void**)&ix->cent, (size_t)C * Dp * 4)); HIPCHK(hipMalloc((void**)&ix->nn, (size_t)C * 4));
  HIPCHK(hipMalloc((void**)&ix->start, ((size_t)C + 1) * 4)); HIPCHK(hipMalloc((void**)&ix->list, (size_t)n * 4));
  ix->index_bytes = (size_t)n * ix->Mrow + cb_floats * 4 + (size_t)C * Dp * 4 + (size_t)C * 4 + ((size_t)C + 1) * 4 + (size_t)n * 4;
  DevTmp<int32_t> dassign, counts, hist, cbase, nchunks; DevTmp<int4> chunks; DevTmp<KmRec> rec; DevTmp<uint8_t> item_codes;
  HIPCHK(dassign.alloc((size_t)n)); HIPCHK(counts.alloc((size_t)C)); HIPCHK(hist.alloc((size_t)tiles * C)); HIPCHK(cbase.alloc((size_t)C + 1));
  HIPCHK(nchunks.alloc(1)); HIPCHK(chunks.alloc((size_t)max_chunks)); HIPCHK(rec.alloc(1)); HIPCHK(item_codes.alloc((size_t)n * M));
  HIPCHK(hipMemcpyAsync(dassign, assign, (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(counts, hcounts.data(), (size_t)C * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(rec, 0, sizeof(KmRec), s));
  // the lists, the centroids and nn_c: what vv_ivf_create builds, by the same launches
  launch_km_group(dassign, n, C, tiles, counts, hist, ix->start, cbase, chunks, max_chunks, nchunks, ix->list, rec, s);
  if (Dp != dim) HIPCHK(hipMemsetAsync(ix->cent, 0, (size_t)C * Dp * 4, s));
  HIPCHK(hipMemcpy2DAsync(ix->cent, (size_t)Dp * 4, centroids, (size_t)dim * 4, (size_t)dim * 4, (size_t)C, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(ix->nn, 0, (size_t)C * 4, s));
  if (ix->metric == VV_KMEANS_EUCLIDEAN) launch_km_finish(nullptr, Dp, dim, nullptr, nullptr, 0, C, 1, 1, ix->cent, ix->nn, rec, s);
  HIPCHK(hipMemcpyAsync(ix->cb, codebooks, cb_floats * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipGetLastError());
  // the codes in item order, then code row p = item list[p]'s
  const int rc = pq_encode_device(c, gr, codebooks, M, ix->ksub, item_codes);
  if (rc) return rc;
  launch_pq_permute(item_codes, ix->list, n, M, ix->Mrow, ix->codes, s);
  HIPCHK(hipGetLastError());
  ix->h_start.assign((size_t)C + 1, 0);
  HIPCHK(hipMemcpyAsync(ix->h_start.data(), ix->start, ((size_t)C + 1) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int k = 0; k < C; ++k) {
    if (ix->h_start[k + 1] - ix->h_start[k] != hcounts[k]) return fail(VV_ERR_STATE, "vv_ivfpq_create: the device's list of cluster %d disagrees with the assignment", k);
    ix->largest = std::max(ix->largest, hcounts[k]); ix->empty += hcounts[k] == 0;
  }
  return VV_OK;
}
}  // namespace

extern "C" {

int vv_pq_train(vv_ctx* c, vv_gallery* items, int32_t M, int32_t ksub, int32_t iters, uint64_t seed, float* codebooks_out, double* objective_out) {
  if (!c) return fail(VV_ERR_ARG, "vv_pq_train: ctx is NULL");
  if (!items) return fail(VV_ERR_ARG, "vv_pq_train: items is NULL");
  if (!codebooks_out) return fail(VV_ERR_ARG, "vv_pq_train: codebooks_out is NULL");
  const GalleryRows gr = gallery_rows(items);
  if (gr.ctx != c) return fail(VV_ERR_ARG, "vv_pq_train: the items gallery belongs to another context");
  int rc = pq_check("vv_pq_train", c, gr, M, ksub, iters);
  if (rc) return rc;
  VV_ENTER(c);
  const int64_t n = gr.n_ref;
  const int dsub = gr.dim / M, Dps = (dsub + RT_BK - 1) / RT_BK * RT_BK;
  DevTmp<float> slice;
  HIPCHK(slice.alloc((size_t)n * Dps));
  std::vector<int32_t> rows((size_t)ksub);
  vv_kmeans_cfg cfg;
  vv_kmeans_cfg_default(&cfg);
  cfg.num_clusters = ksub; cfg.iters = iters; cfg.metric = VV_KMEANS_EUCLIDEAN;
  for (int m = 0; m < M; ++m) {
    rc = vv_kmeans_init_rows(seed + (uint64_t)m, (int32_t)n, ksub, rows.data());
    if (rc) return rc;
    launch_pq_slice(gr.feat, n, gr.Dp, m * dsub, dsub, Dps, slice, c->stream);
    HIPCHK(hipGetLastError());
    vv_kmeans_report rep;
    const GalleryRows sub = {slice, n, dsub, Dps, c};
    rc = vv_kmeans_rows(c, sub, &cfg, nullptr, rows.data(), codebooks_out + (size_t)m * ksub * dsub, nullptr, nullptr, nullptr, nullptr, &rep, nullptr);
    if (rc) return rc;
    if (objective_out) objective_out[m] = rep.objective_last;
  }
  return VV_OK;
}

int vv_pq_encode(vv_ctx* c, vv_gallery* items, const float* codebooks, int32_t M, int32_t ksub, uint8_t* codes_out) {
  if (!c) return fail(VV_ERR_ARG, "vv_pq_encode: ctx is NULL");
  if (!items) return fail(VV_ERR_ARG, "vv_pq_encode: items is NULL");
  if (!codebooks) return fail(VV_ERR_ARG, "vv_pq_encode: codebooks is NULL");
  if (!codes_out) return fail(VV_ERR_ARG, "vv_pq_encode: codes_out is NULL");
  const GalleryRows gr = gallery_rows(items);
  if (gr.ctx != c) return fail(VV_ERR_ARG, "vv_pq_encode: the items gallery belongs to another context");
  int rc = pq_check("vv_pq_encode", c, gr, M, ksub, 0);
  if (rc) return rc;
  VV_ENTER(c);
  DevTmp<uint8_t> dcodes;
  HIPCHK(dcodes.alloc((size_t)gr.n_ref * M));
  rc = pq_encode_device(c, gr, codebooks, M, ksub, dcodes);
  if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
  HIPCHK(hipMemcpyAsync(codes_out, dcodes, (size_t)gr.n_ref * M, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return VV_OK;
}

int vv_ivfpq_create(vv_ctx* c, vv_gallery* items, const float* centroids, int32_t C, int32_t metric, const int32_t* assign,
                    const float* codebooks, int32_t M, int32_t ksub, vv_ivfpq** out) {
  if (!c) return fail(VV_ERR_ARG, "vv_ivfpq_create: ctx is NULL");
  if (!items) return fail(VV_ERR_ARG, "vv_ivfpq_create: items is NULL");
  if (!centroids) return fail(VV_ERR_ARG, "vv_ivfpq_create: centroids is NULL");
  if (!codebooks) return fail(VV_ERR_ARG, "vv_ivfpq_create: codebooks is NULL");
  if (!out) return fail(VV_ERR_ARG, "vv_ivfpq_create: out is NULL");
  const GalleryRows gr = gallery_rows(items);
  if (gr.ctx != c) return fail(VV_ERR_ARG, "vv_ivfpq_create: the items gallery belongs to another context");
  const int64_t n = gr.n_ref;
  if (C < 1 || C > KM_MAX_CLUSTERS) return fail(VV_ERR_ARG, "vv_ivfpq_create: C = %d is outside 1 .. %d", C, KM_MAX_CLUSTERS);
  if (C > n) return fail(VV_ERR_ARG, "vv_ivfpq_create: C = %d exceeds the gallery's %lld items", C, (long long)n);
  if (metric != VV_KMEANS_EUCLIDEAN && metric != VV_KMEANS_SPHERICAL) return fail(VV_ERR_ARG, "vv_ivfpq_create: unknown metric %d", metric);
  int rc = pq_check("vv_ivfpq_create", c, gr, M, ksub, 0);
  if (rc) return rc;
  if (assign)
    for (int64_t i = 0; i < n; ++i)
      if (assign[i] < 0 || assign[i] >= C)
        return fail(VV_ERR_ARG, "vv_ivfpq_create: assign[%lld] = %d is outside 0 .. %d", (long long)i, assign[i], C - 1);
  std::vector<int32_t> own;
  if (!assign) {
    // what vv_gallery_kmeans with iters = 0 returns for these centroids and this metric: that call, as vv_ivf_create makes it
    vv_kmeans_cfg cfg;
    vv_kmeans_cfg_default(&cfg);
    cfg.num_clusters = C; cfg.iters = 0; cfg.metric = metric;
    own.assign((size_t)n, 0);
    std::vector<float> cent_back((size_t)C * gr.dim);
    vv_kmeans_report rep;
    rc = vv_gallery_kmeans(c, items, &cfg, centroids, nullptr, cent_back.data(), own.data(), nullptr, nullptr, nullptr, &rep);
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i)
      if (own[i] < 0 || own[i] >= C) return fail(VV_ERR_STATE, "vv_ivfpq_create: the assignment pass left item %lld in cluster %d", (long long)i, own[i]);
    assign = own.data();
  }
  VV_ENTER(c);
  vv_ivfpq* ix = new vv_ivfpq;
  ix->ctx = c; ix->n_ref = n; ix->dim = gr.dim; ix->Dp = gr.Dp; ix->C = C; ix->metric = metric;
  ix->M = M; ix->ksub = ksub; ix->dsub = gr.dim / M; ix->Mrow = pq_code_row_bytes(M);
  rc = pq_build(c, ix, gr, centroids, assign, codebooks);
  if (rc) { (void)hipStreamSynchronize(c->stream); pq_release(ix); return rc; }
  *out = ix;
  return VV_OK;
}

int vv_ivfpq_destroy(vv_ctx* c, vv_ivfpq* ix) {
  if (!c) return fail(VV_ERR_ARG, "vv_ivfpq_destroy: ctx is NULL");
  if (!ix) return VV_OK;
  if (ix->ctx != c) return fail(VV_ERR_ARG, "vv_ivfpq_destroy: the index belongs to another context");
  VV_ENTER(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  pq_release(ix);
  return VV_OK;
}

int vv_ivfpq_get(const vv_ivfpq* ix, const char* name, double* value) {
  if (!ix || !name || !value) return fail(VV_ERR_ARG, "vv_ivfpq_get: NULL argument");
  const std::string n(name);
  if (n == "n_ref") *value = (double)ix->n_ref;
  else if (n == "dim") *value = ix->dim;
  else if (n == "num_clusters") *value = ix->C;
  else if (n == "metric") *value = ix->metric;
  else if (n == "M") *value = ix->M;
  else if (n == "ksub") *value = ix->ksub;
  else if (n == "index_bytes") *value = (double)ix->index_bytes;
  else if (n == "largest_list") *value = ix->largest;
  else if (n == "empty_lists") *value = ix->empty;
  else if (n == "last_blocks") *value = (double)ix->last_blocks;
  else if (n == "last_candidates") *value = (double)ix->last_candidates;
  else if (n == "last_scan_form") *value = ix->last_form;
  else if (n == "last_probe_ms") *value = ix->last_ms[0];
  else if (n == "last_lut_ms") *value = ix->last_ms[1];
  else if (n == "last_scan_ms") *value = ix->last_ms[2];
  else if (n == "last_select_ms") *value = ix->last_ms[3];
  else if (n == "last_device_ms") *value = ix->last_ms[4];
  else return fail(VV_ERR_ARG, "vv_ivfpq_get: unknown name '%s'", name);
  return VV_OK;
}

int vv_ivfpq_lists(vv_ctx* c, vv_ivfpq* ix, int32_t* start, int32_t* list) {
  if (!c || !ix || !start || !list) return fail(VV_ERR_ARG, "vv_ivfpq_lists: NULL argument");
  if (ix->ctx != c) return fail(VV_ERR_ARG, "vv_ivfpq_lists: the index belongs to another context");
  VV_ENTER(c);
  HIPCHK(hipMemcpyAsync(start, ix->start, ((size_t)ix->C + 1) * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(list, ix->list, (size_t)ix->n_ref * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return VV_OK;
}

int vv_ivfpq_codes(vv_ctx* c, vv_ivfpq* ix, uint8_t* codes) {
  if (!c || !ix || !codes) return fail(VV_ERR_ARG, "vv_ivfpq_codes: NULL argument");
  if (ix->ctx != c) return fail(VV_ERR_ARG, "vv_ivfpq_codes: the index belongs to another context");
  VV_ENTER(c);
  HIPCHK(hipMemcpy2DAsync(codes, (size_t)ix->M, ix->codes, (size_t)ix->Mrow, (size_t)ix->M, (size_t)ix->n_ref, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return VV_OK;
}

int vv_ivfpq_search(vv_ctx* c, vv_ivfpq* ix, const float* q, int32_t n_q, int32_t nprobe, int32_t k, int32_t* idx, float* dist,
                    int32_t* n_candidates) {
  if (!c) return fail(VV_ERR_ARG, "vv_ivfpq_search: ctx is NULL");
  if (!ix) return fail(VV_ERR_ARG, "vv_ivfpq_search: index is NULL");
  if (!q) return fail(VV_ERR_ARG, "vv_ivfpq_search: q is NULL");
  if (!idx) return fail(VV_ERR_ARG, "vv_ivfpq_search: idx is NULL");
  if (!dist) return fail(VV_ERR_ARG, "vv_ivfpq_search: dist is NULL");
  if (ix->ctx != c) return fail(VV_ERR_ARG, "vv_ivfpq_search: the index belongs to another context");
  if (n_q < 1) return fail(VV_ERR_ARG, "vv_ivfpq_search: n_q = %d", n_q);
  const int C = ix->C, Dp = ix->Dp, dim = ix->dim;
  if (nprobe < 1 || nprobe > C || (nprobe > IVF_MAX_PROBE && nprobe != C))
    return fail(VV_ERR_ARG, "vv_ivfpq_search: nprobe = %d is neither in 1 .. %d nor the index's %d clusters", nprobe, std::min(C, IVF_MAX_PROBE), C);
  if (k < 1 || k > RT_MAX_K) return fail(VV_ERR_ARG, "vv_ivfpq_search: k = %d is outside 1 .. %d", k, RT_MAX_K);
  const PqPlan p = pq_plan(ix->n_ref, dim, C, nprobe, n_q, ivf_pitch_items(ix->h_start.data(), C, nprobe), ix->M, ix->ksub, c->ivf_block_rows);
  if (!p.ok) return fail(VV_ERR_ARG, "vv_ivfpq_search: one query's %d probed lists of %lld items do not fit the scratch limit", nprobe, (long long)ix->n_ref);
  VV_ENTER(c);
  hipStream_t s = c->stream;
  if (p.total_bytes > ix->scratch_cap) {
    HIPCHK(hipStreamSynchronize(s));
    dfree(ix->scratch); ix->scratch = nullptr; ix->scratch_cap = 0;
    HIPCHK(hipMalloc((void**)&ix->scratch, p.total_bytes));
    ix->scratch_cap = p.total_bytes;
  }
  // the one allocation carved up: every buffer on IVF_ALIGN bytes (the plan counts PQ_BUFFERS of them)
  size_t used = 0; int taken = 0;
  auto take = [&](size_t bytes) { char* at = ix->scratch + used; used += (bytes + IVF_ALIGN - 1) / IVF_ALIGN * IVF_ALIGN; ++taken; return (void*)at; };
  const size_t R = (size_t)p.block_rows, P = (size_t)p.pairs;
  float* score = (float*)take(R * C * 4); float* qdev = (float*)take(R * Dp * 4); float* lut = (float*)take(R * p.table * 4);
  float* cand = (float*)take(R * p.pitch * 4); int32_t* m = (int32_t*)take(R * 4);
  int32_t* oidx = (int32_t*)take(R * RT_MAX_K * 4); float* odist = (float*)take(R * RT_MAX_K * 4);
  int32_t* probe = (int32_t*)take(P * 4); int32_t* off = (int32_t*)take(P * 4);
  int32_t* counts = (int32_t*)take((size_t)C * 4); IvfRec* rec = (IvfRec*)take(sizeof(IvfRec));
  if (used > ix->scratch_cap || taken > PQ_BUFFERS) return fail(VV_ERR_STATE, "vv_ivfpq_search: %zu bytes in %d buffers pass the plan's %zu", used, taken, p.total_bytes);

  const int64_t tb = std::min<int64_t>(p.blocks, IVF_TIMED_BLOCKS);
  PqEvents ev;
  ev.e.assign((size_t)(5 * tb + 2), nullptr);
  for (hipEvent_t& x : ev.e) HIPCHK(hipEventCreate(&x));
  const size_t e_begin = (size_t)(5 * tb), e_end = e_begin + 1;
  const int all = nprobe == C, euclid = ix->metric == VV_KMEANS_EUCLIDEAN;

  HIPCHK(hipEventRecord(ev.e[e_begin], s));
  HIPCHK(hipMemsetAsync(rec, 0, sizeof(IvfRec), s));
  if (Dp != dim) HIPCHK(hipMemsetAsync(qdev, 0, R * Dp * 4, s));      // the K padding of the query rows stays zero over the blocks
  for (int64_t b = 0; b < p.blocks; ++b) {
    const int64_t q0 = b * p.block_rows;
    const int rows = (int)std::min<int64_t>(p.block_rows, n_q - q0);
    const bool timed = b < tb;
    hipEvent_t* e = timed ? &ev.e[(size_t)(5 * b)] : nullptr;
    if (timed) HIPCHK(hipEventRecord(e[0], s));
    // 1. probe: vv_ivf_search's, on full-dimension rows
    HIPCHK(hipMemcpy2DAsync(qdev, (size_t)Dp * 4, q + (size_t)q0 * dim, (size_t)dim * 4, (size_t)dim * 4, (size_t)rows, hipMemcpyHostToDevice, s));
    launch_sim_f32(qdev, ix->cent, score, rows, C, Dp, C, s);
    HIPCHK(hipMemsetAsync(counts, 0, (size_t)C * 4, s));
    launch_ivf_probe(score, rows, C, nprobe, all, euclid, ix->nn, ix->start, probe, off, m, counts, rec, s);
    if (timed) HIPCHK(hipEventRecord(e[1], s));
    // 2. every query's table
    launch_pq_lut(qdev, rows, Dp, ix->cb, ix->M, ix->ksub, ix->dsub, lut, p.table, s);
    if (timed) HIPCHK(hipEventRecord(e[2], s));
    // 3. the scan of the probed lists' codes
    PqScan sc;
    sc.lut = lut; sc.table = p.table; sc.slab = ix->codes; sc.Mrow = ix->Mrow; sc.start = ix->start; sc.probe = probe; sc.off = off;
    sc.cand = cand; sc.pitch = p.pitch; sc.rows = rows; sc.nprobe = nprobe; sc.M = ix->M; sc.ksub = ix->ksub;
    launch_pq_scan(sc, p.form, s);
    if (timed) HIPCHK(hipEventRecord(e[3], s));
    // 4. select: of the block k_ivf_select reads the candidates, the pairs and the lists
    IvfBlock blk;
    blk.Q = qdev; blk.slab = nullptr; blk.start = ix->start; blk.list = ix->list; blk.probe = probe; blk.off = off; blk.qstart = nullptr;
    blk.qlist = nullptr; blk.tiles = nullptr; blk.ntiles = nullptr; blk.cand = cand; blk.pitch = p.pitch; blk.rows = rows; blk.Dp = Dp; blk.C = C;
    blk.nprobe = nprobe; blk.tile_cap = 0;
    launch_ivf_select(blk, k, oidx, odist, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(idx + (size_t)q0 * k, oidx, (size_t)rows * k * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(dist + (size_t)q0 * k, odist, (size_t)rows * k * 4, hipMemcpyDeviceToHost, s));
    if (n_candidates) HIPCHK(hipMemcpyAsync(n_candidates + q0, m, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
    if (timed) HIPCHK(hipEventRecord(e[4], s));
  }
  IvfRec hrec;
  HIPCHK(hipMemcpyAsync(&hrec, rec, sizeof(IvfRec), hipMemcpyDeviceToHost, s));
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
  ix->last_blocks = p.blocks; ix->last_candidates = hrec.candidates; ix->last_form = p.form;
  return VV_OK;
}

}  // extern "C"
