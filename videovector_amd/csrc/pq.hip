// pq.hip -- entry points of product quantisation on a gallery and of the inverted-file index that keeps product-quantised codes in
// place of the items' rows (include/videovec.h: vv_pq_train, vv_pq_encode, vv_ivfpq_create, vv_ivfpq_destroy, vv_ivfpq_search,
// vv_ivfpq_get, vv_ivfpq_lists, vv_ivfpq_codes).  The kernels are in kernels_pq.hip; a codebook is trained and a code is assigned by
// k-means' own body on a column slice (kmeans.hip: vv_kmeans_rows).  The lists, their checks and accessors and the search loop are the
// coarse index's (vv_ivf_coarse.h, ivf_coarse.hip); this file adds what this index stores beside the lists -- codes and codebooks -- and
// what a block of a search does between probe and select: every query's table, then the scan of the probed lists' codes.  The limits
// and the sizes of every search buffer are vv_pq_plan.h's; of the context a search reads the ivf_block_rows option.
// HAS NO REFERENCE COUNTERPART.
#include <algorithm>
#include <string>
#include <vector>

#include "vv_ivf_coarse.h"

using namespace vv;

struct vv_ivfpq : IvfCoarse {
  int M = 0, ksub = 0, dsub = 0, Mrow = 0;
  uint8_t* codes = nullptr;                                    // [n_ref][Mrow] list-position order
  float* cb = nullptr;                                         // [M][ksub][dsub]
  size_t index_bytes = 0;                                      // every device byte of the index but the scratch
  int last_form = 0;                                           // last_ms[1], [2]: table, scan
};

namespace {
void pq_release(vv_ivfpq* ix) {
  dfree(ix->codes); dfree(ix->cb); coarse_release(ix);
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
  int rc = coarse_build("vv_ivfpq_create", ix, centroids, assign);
  if (rc) return rc;
  const int64_t n = ix->n_ref;
  const int C = ix->C, M = ix->M;
  hipStream_t s = c->stream;
  const size_t cb_floats = (size_t)M * ix->ksub * ix->dsub;
  HIPCHK(hipMalloc((void**)&ix->codes, (size_t)n * ix->Mrow)); HIPCHK(hipMalloc((void**)&ix->cb, cb_floats * 4));
  ix->index_bytes = (size_t)n * ix->Mrow + cb_floats * 4 + (size_t)C * ix->Dp * 4 + (size_t)C * 4 + ((size_t)C + 1) * 4 + (size_t)n * 4;
  DevTmp<uint8_t> item_codes;
  HIPCHK(item_codes.alloc((size_t)n * M));
  HIPCHK(hipMemcpyAsync(ix->cb, codebooks, cb_floats * 4, hipMemcpyHostToDevice, s));
  // the codes in item order, then code row p = item list[p]'s
  rc = pq_encode_device(c, gr, codebooks, M, ix->ksub, item_codes);
  if (rc) return rc;
  launch_pq_permute(item_codes, ix->list, n, M, ix->Mrow, ix->codes, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
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
  GalleryRows gr;
  int rc = coarse_check("vv_ivfpq_create", c, items, centroids, {{"codebooks", codebooks}, {"out", out}}, C, metric, &gr);
  if (rc) return rc;
  rc = pq_check("vv_ivfpq_create", c, gr, M, ksub, 0);
  if (rc) return rc;
  std::vector<int32_t> own;
  rc = coarse_assign("vv_ivfpq_create", c, items, gr, centroids, C, metric, &assign, &own);
  if (rc) return rc;
  VV_ENTER(c);
  vv_ivfpq* ix = new vv_ivfpq;
  ix->ctx = c; ix->n_ref = gr.n_ref; ix->dim = gr.dim; ix->Dp = gr.Dp; ix->C = C; ix->metric = metric;
  ix->M = M; ix->ksub = ksub; ix->dsub = gr.dim / M; ix->Mrow = pq_code_row_bytes(M);
  rc = pq_build(c, ix, gr, centroids, assign, codebooks);
  if (rc) { (void)hipStreamSynchronize(c->stream); pq_release(ix); return rc; }
  *out = ix;
  return VV_OK;
}

int vv_ivfpq_destroy(vv_ctx* c, vv_ivfpq* ix) {
  const int rc = coarse_drain("vv_ivfpq_destroy", c, ix);
  if (!rc && ix) pq_release(ix);
  return rc;
}

int vv_ivfpq_get(const vv_ivfpq* ix, const char* name, double* value) {
  if (!ix || !name || !value) return fail(VV_ERR_ARG, "vv_ivfpq_get: NULL argument");
  const std::string n(name);
  if (coarse_get(*ix, n, value)) return VV_OK;
  if (n == "M") *value = ix->M;
  else if (n == "ksub") *value = ix->ksub;
  else if (n == "index_bytes") *value = (double)ix->index_bytes;
  else if (n == "last_scan_form") *value = ix->last_form;
  else if (n == "last_lut_ms") *value = ix->last_ms[1];
  else if (n == "last_scan_ms") *value = ix->last_ms[2];
  else return fail(VV_ERR_ARG, "vv_ivfpq_get: unknown name '%s'", name);
  return VV_OK;
}

int vv_ivfpq_lists(vv_ctx* c, vv_ivfpq* ix, int32_t* start, int32_t* list) { return coarse_lists("vv_ivfpq_lists", c, ix, start, list); }

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
  PqPlan p;
  float* lut = nullptr;
  CoarseMiddle mid;
  mid.buffers = PQ_BUFFERS;
  mid.plan = [&](int64_t pitch_items) {
    p = pq_plan(ix->n_ref, ix->dim, ix->C, nprobe, n_q, pitch_items, ix->M, ix->ksub, c->ivf_block_rows);
    return CoarsePlan{p.ok, p.pitch, p.block_rows, p.blocks, p.total_bytes};
  };
  mid.carve = [&](const std::function<void*(size_t)>& take) { lut = (float*)take((size_t)p.block_rows * p.table * 4); };
  mid.block = [&](const CoarseBlock& b, const std::function<hipError_t()>& mark, IvfBlock*) -> int {
    // every query's table
    launch_pq_lut(b.qdev, b.rows, ix->Dp, ix->cb, ix->M, ix->ksub, ix->dsub, lut, p.table, c->stream);
    HIPCHK(mark());
    // the scan of the probed lists' codes
    PqScan sc;
    sc.lut = lut; sc.table = p.table; sc.slab = ix->codes; sc.Mrow = ix->Mrow; sc.start = ix->start; sc.probe = b.probe; sc.off = b.off;
    sc.cand = b.cand; sc.pitch = p.pitch; sc.rows = b.rows; sc.nprobe = nprobe; sc.M = ix->M; sc.ksub = ix->ksub;
    launch_pq_scan(sc, p.form, c->stream);
    return VV_OK;
  };
  IvfRec rec;
  const int rc = coarse_search("vv_ivfpq_search", c, ix, q, n_q, nprobe, k, idx, dist, n_candidates, mid, &rec);
  if (rc) return rc;
  ix->last_form = p.form;
  return VV_OK;
}

}  // extern "C"
