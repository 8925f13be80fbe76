// retrieval.hip -- entry points of the retrieval statistics (include/videovec.h: vv_retrieval_stats, vv_gallery_*).  The kernels are
// in kernels_retrieval.hip, the sizes of the gallery's scratch in vv_gallery_plan.h.  Everything is queued on the context's stream;
// of the context these calls read the nearest_select_min_k option, and vv_gallery_from_table the embedding helpers of api.hip.  None
// of this reads or writes the training step's state.
#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "vv_ctx.h"

using namespace vv;

extern "C" {

int vv_retrieval_stats(vv_ctx* c, const float* feat, int32_t n, int32_t dim, const int32_t* video_ids,
                       const int32_t* map_ids, const int32_t* map_cls, int32_t n_map,
                       int exclude_same, float* mean_ap, float* hit1, float* hit5) {
  if (!c || !feat || !video_ids || n < 2 || dim < 1 || (n_map > 0 && (!map_ids || !map_cls)))
    return fail(VV_ERR_ARG, "vv_retrieval_stats: bad argument");
  if (n_map < 1) return fail(VV_ERR_ARG, "need atleast one entry in id-to-class map!");   // retrieval_stats_layer.cpp:49
  VV_ENTER(c);
  DevTmp<float> dx, dd;
  HIPCHK(dx.alloc((size_t)n * dim)); HIPCHK(dd.alloc((size_t)n * n));
  HIPCHK(hipMemcpyAsync(dx, feat, (size_t)n * dim * 4, hipMemcpyHostToDevice, c->stream));
  launch_gram(dx, n, dim, -2.0f, dd, c->stream);                                           // :208-209
  std::vector<float> dist((size_t)n * n);
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(dist.data(), dd, dist.size() * 4, hipMemcpyDeviceToHost));
  std::unordered_map<int, int> cls;
  for (int i = 0; i < n_map; ++i) cls[map_ids[i]] = map_cls[i];
  auto cls_of = [&](int id) { auto it = cls.find(id); return it == cls.end() ? 0 : it->second; };
  std::vector<int> order(n);
  double s_ap = 0, s_1 = 0, s_5 = 0, npos = 0;
  for (int i = 0; i < n; ++i) {
    float* row = dist.data() + (size_t)i * n;
    row[i] = -1e15f;                                                                       // :228-229
    for (int j = 0; j < n; ++j) order[j] = j;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return row[a] < row[b] || (row[a] == row[b] && a < b); });
    const int label = cls_of(video_ids[i]);
    if (label < 0) continue;                                                               // :246-248
    double ap = 0, a1 = 0, a5 = 0, val = 0, ret = 0;                                       // :104-141
    for (int kk = 1; kk < n; ++kk) {
      const int j = order[kk];
      if (video_ids[j] != video_ids[i] || !exclude_same) {
        val += 1;
        if (cls_of(video_ids[j]) == label) { if (val <= 1) a1 += 1; if (val <= 5) a5 += 1; ret += 1; ap += ret / val; }
      }
    }
    if (ret > 0) ap /= ret;
    s_ap += ap; s_1 += a1; s_5 += a5 / 5; npos += 1;
  }
  if (npos == 0) return fail(VV_ERR_ARG, "vv_retrieval_stats: no sample with a non-negative class");
  if (mean_ap) *mean_ap = (float)(s_ap / npos);
  if (hit1) *hit1 = (float)(s_1 / npos);
  if (hit5) *hit5 = (float)(s_5 / npos);
  return VV_OK;
}

// ------------------------------------------------------------------------------- gallery ------
// RetrievalRankStatsFixedRefLayer (retrieval_rank_stats_fixed_ref_layer.cpp): queries ranked against a fixed reference set.
// The similarity, the selection and the counting run in kernels_retrieval.hip, one query block at a time through a scratch
// buffer that never exceeds GALLERY_SCRATCH_MAX (vv_gallery_plan.h); the host only walks per-query scalars.
struct vv_gallery : GalleryShape {       // pitch, Dp, seg, S, qb_max: gallery_shape(n_ref, dim)
  vv_ctx* ctx = nullptr;
  int64_t n_ref = 0;
  int dim = 0;
  float* feat = nullptr;                 // [n_ref][Dp], columns dim .. Dp-1 zero
  int32_t* ref_ids = nullptr;            // [n_ref] or NULL (a gallery for top-k only)
  int32_t* pos_idx = nullptr;            // gallery indices grouped by id (ascending id, ascending index inside one id)
  std::vector<int32_t> uid, ustart;      // host: the distinct ids, ascending, and where each one's group starts in pos_idx
  std::vector<int32_t> h_ids;            // host: ref_ids
  // class-level statistics: the lists of the id -> class map last given, kept until another map arrives
  std::vector<int32_t> cs_map_ids, cs_map_cls;     // that map
  std::vector<int32_t> h_cls, cvals, cstart;       // class of every item; the distinct classes, ascending; their groups in cpos
  int32_t *cls = nullptr, *cpos = nullptr;         // device: class of every item; item indices grouped by class (ascending index inside)
  // scratch, grown on demand up to qb_max rows and kept between calls
  int qb_cap = 0;
  float *dist = nullptr, *qdev = nullptr, *out_dist = nullptr;
  uint64_t* part = nullptr; uint32_t* bins = nullptr; int32_t* out_idx = nullptr;
  int32_t *pstart = nullptr, *pcount = nullptr, *qids = nullptr; RankAcc* acc = nullptr;
  uint64_t* skeys = nullptr; uint32_t* cbins = nullptr;      // class-level statistics only: allocated by its first call
  // the selection form of vv_gallery_nearest* only (it shares skeys: its candidate keys): allocated by its first call
  uint32_t *sel_st = nullptr, *sel_hist = nullptr, *sel_segh = nullptr; int32_t* nn_idx = nullptr; float* nn_dist = nullptr;
  size_t scratch_bytes = 0;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // call begin / end, similarity begin / end, vote begin / end (of the block in flight)
  double last_sim_ms = 0, last_device_ms = 0, last_knn_vote_ms = 0; int last_passes = 0;
  int last_nearest_form = 0;             // vv_gallery_nearest*: 1 streaming, 2 selection; 0 before the first call
};

extern "C++" vv::GalleryRows vv::gallery_rows(const vv_gallery* g) { return {g->feat, g->n_ref, g->dim, g->Dp, g->ctx}; }      // (linear.hip)

static void gallery_free_scratch(vv_gallery* g) {
  dfree(g->dist); dfree(g->qdev); dfree(g->out_dist); dfree(g->part); dfree(g->bins); dfree(g->out_idx);
  dfree(g->pstart); dfree(g->pcount); dfree(g->qids); dfree(g->acc); dfree(g->skeys); dfree(g->cbins);
  g->dist = g->qdev = g->out_dist = nullptr; g->part = nullptr; g->bins = nullptr; g->out_idx = nullptr;
  g->pstart = g->pcount = g->qids = nullptr; g->acc = nullptr; g->skeys = nullptr; g->cbins = nullptr;
  dfree(g->sel_st); dfree(g->sel_hist); dfree(g->sel_segh); dfree(g->nn_idx); dfree(g->nn_dist);
  g->sel_st = g->sel_hist = g->sel_segh = nullptr; g->nn_idx = nullptr; g->nn_dist = nullptr;
  g->qb_cap = 0; g->scratch_bytes = 0;
}

// cls: the call is vv_gallery_class_stats, which needs skeys / cbins as well; sel: the selection form of vv_gallery_nearest*,
// which needs skeys and its own buffers
static int gallery_ensure_scratch(vv_gallery* g, int rows, bool cls, bool sel) {
  if (rows <= g->qb_cap && (!cls || g->cbins) && (!sel || g->sel_st)) return VV_OK;
  gallery_free_scratch(g);
  const size_t r = (size_t)rows;
  const size_t b_dist = r * g->pitch * 4, b_q = r * g->Dp * 4, b_part = r * g->S * RT_MAX_K * sizeof(uint64_t), b_bins = r * 2 * RT_CHUNK * 4,
               b_out = r * RT_MAX_K * 4, b_row = r * 4, b_acc = r * sizeof(RankAcc);
  const size_t total = r * gallery_row_bytes(*g, cls, sel);
  if (total > GALLERY_SCRATCH_MAX) return fail(VV_ERR_STATE, "gallery scratch of %zu bytes exceeds the limit", total);
  if (cls || sel) HIPCHK(hipMalloc((void**)&g->skeys, r * RT_CHUNK * 8));
  if (cls) HIPCHK(hipMalloc((void**)&g->cbins, r * 3 * RT_CHUNK * 4));
  if (sel) {
    HIPCHK(hipMalloc((void**)&g->sel_st, r * 4 * 4)); HIPCHK(hipMalloc((void**)&g->sel_hist, r * RT_SEL_BINS * 4));
    HIPCHK(hipMalloc((void**)&g->sel_segh, r * g->S * RT_SEL_LAST_BINS * 4));
    HIPCHK(hipMalloc((void**)&g->nn_idx, r * RT_CHUNK * 4)); HIPCHK(hipMalloc((void**)&g->nn_dist, r * RT_CHUNK * 4));
  }
  HIPCHK(hipMalloc((void**)&g->dist, b_dist)); HIPCHK(hipMalloc((void**)&g->qdev, b_q));
  HIPCHK(hipMalloc((void**)&g->part, b_part)); HIPCHK(hipMalloc((void**)&g->bins, b_bins));
  HIPCHK(hipMalloc((void**)&g->out_idx, b_out)); HIPCHK(hipMalloc((void**)&g->out_dist, b_out));
  HIPCHK(hipMalloc((void**)&g->pstart, b_row)); HIPCHK(hipMalloc((void**)&g->pcount, b_row)); HIPCHK(hipMalloc((void**)&g->qids, b_row));
  HIPCHK(hipMalloc((void**)&g->acc, b_acc));
  HIPCHK(hipMemset(g->qdev, 0, b_q));                       // the K padding of the query rows stays zero from here on
  g->qb_cap = rows; g->scratch_bytes = total;
  return VV_OK;
}

// shape-dependent constants, the feature buffer and the id -> gallery-index lists; g->feat is filled by the caller
static int gallery_init(vv_ctx* c, vv_gallery* g, int64_t n_ref, int32_t dim, const int32_t* ref_ids) {
  g->ctx = c; g->n_ref = n_ref; g->dim = dim;
  static_cast<GalleryShape&>(*g) = gallery_shape(n_ref, dim);
  if (g->qb_max < 1) return fail(VV_ERR_ARG, "vv_gallery: %lld reference items do not fit one query row into the scratch limit", (long long)n_ref);
  HIPCHK(hipMalloc((void**)&g->feat, (size_t)n_ref * g->Dp * 4));
  if (g->Dp != dim) HIPCHK(hipMemsetAsync(g->feat, 0, (size_t)n_ref * g->Dp * 4, c->stream));
  for (int i = 0; i < 6; ++i) HIPCHK(hipEventCreate(&g->ev[i]));
  if (!ref_ids) return VV_OK;
  // the id -> index lists, once (the reference re-reads every reference id for every query: ComputeApStats :73-75)
  std::vector<int32_t> order((size_t)n_ref);
  for (int64_t i = 0; i < n_ref; ++i) order[i] = (int32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return ref_ids[a] < ref_ids[b]; });
  for (int64_t i = 0; i < n_ref; ++i)
    if (i == 0 || ref_ids[order[i]] != ref_ids[order[i - 1]]) { g->uid.push_back(ref_ids[order[i]]); g->ustart.push_back((int32_t)i); }
  g->ustart.push_back((int32_t)n_ref);
  g->h_ids.assign(ref_ids, ref_ids + n_ref);
  HIPCHK(hipMalloc((void**)&g->ref_ids, (size_t)n_ref * 4)); HIPCHK(hipMalloc((void**)&g->pos_idx, (size_t)n_ref * 4));
  HIPCHK(hipMemcpy(g->ref_ids, ref_ids, (size_t)n_ref * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g->pos_idx, order.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice));
  return VV_OK;
}

static void gallery_release(vv_gallery* g) {
  gallery_free_scratch(g);
  dfree(g->feat); dfree(g->ref_ids); dfree(g->pos_idx); dfree(g->cls); dfree(g->cpos);
  for (int i = 0; i < 6; ++i) if (g->ev[i]) (void)hipEventDestroy(g->ev[i]);
  delete g;
}

int vv_gallery_create(vv_ctx* c, const float* feat, int64_t n_ref, int32_t dim, const int32_t* ref_ids, vv_gallery** out) {
  if (!c || !feat || !out) return fail(VV_ERR_ARG, "vv_gallery_create: NULL argument");
  if (n_ref < 1 || n_ref > (1ll << 30) || dim < 1 || dim > 8192)
    return fail(VV_ERR_ARG, "vv_gallery_create: %lld reference items of dimension %d", (long long)n_ref, dim);
  VV_ENTER(c);
  vv_gallery* g = new vv_gallery;
  int rc = gallery_init(c, g, n_ref, dim, ref_ids);
  if (!rc) {
    const hipError_t e = hipMemcpy2DAsync(g->feat, (size_t)g->Dp * 4, feat, (size_t)dim * 4, (size_t)dim * 4, (size_t)n_ref,
                                          hipMemcpyHostToDevice, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || e2 != hipSuccess) rc = fail(VV_ERR_HIP, "vv_gallery_create: upload failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
  }
  if (rc) { gallery_release(g); return rc; }
  *out = g;
  return VV_OK;
}

int vv_gallery_from_table(vv_ctx* c, const int32_t* rows, int64_t n, int32_t k, const float* coeff, int relu, int l2norm,
                          const int32_t* ref_ids, vv_gallery** out) {
  if (!c || !rows || !out || n <= 0 || k <= 0) return fail(VV_ERR_ARG, "vv_gallery_from_table: bad argument");
  if (!c->table || !c->W) return fail(VV_ERR_STATE, "vv_gallery_from_table: table and parameters must be set first");
  if (n > (1ll << 24)) return fail(VV_ERR_ARG, "vv_gallery_from_table: n too large");
  { const int rcg = vv_upd_pending_guard(c, "vv_gallery_from_table"); if (rcg) return rcg; }
  VV_ENTER(c);
  { const int rcj = vv_comm_join(c); if (rcj) return rcj; }
  DevTmp<float> emb;                                                          // [n][D]; copied into the padded rows below
  HIPCHK(emb.alloc((size_t)n * c->D));
  int rc = (k == 1 && !coeff) ? vv_embed_rows_device(c, "vv_gallery_from_table", rows, n, relu, l2norm, emb)
                              : vv_embed_mean_device(c, "vv_gallery_from_table", rows, n, k, coeff, relu, l2norm, emb);
  if (rc) return rc;
  vv_gallery* g = new vv_gallery;
  rc = gallery_init(c, g, n, c->D, ref_ids);
  if (!rc) {
    const hipError_t e = hipMemcpy2DAsync(g->feat, (size_t)g->Dp * 4, emb, (size_t)c->D * 4, (size_t)c->D * 4, (size_t)n,
                                          hipMemcpyDeviceToDevice, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || e2 != hipSuccess) rc = fail(VV_ERR_HIP, "vv_gallery_from_table: copy failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
  }
  if (rc) { gallery_release(g); return rc; }
  *out = g;
  return VV_OK;
}

int vv_gallery_destroy(vv_ctx* c, vv_gallery* g) {
  if (!c) return fail(VV_ERR_ARG, "vv_gallery_destroy: ctx is NULL");
  if (!g) return VV_OK;
  if (g->ctx != c) return fail(VV_ERR_ARG, "vv_gallery_destroy: the gallery belongs to another context");
  VV_ENTER(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  gallery_release(g);
  return VV_OK;
}

int vv_gallery_get(const vv_gallery* g, const char* name, double* value) {
  if (!g || !name || !value) return fail(VV_ERR_ARG, "vv_gallery_get: NULL argument");
  const std::string n(name);
  if (n == "n_ref") *value = (double)g->n_ref;
  else if (n == "n_ids") *value = (double)g->uid.size();
  else if (n == "row_floats") *value = g->Dp;
  else if (n == "feat_device") *value = (double)(uintptr_t)g->feat;      // (a device address: below 2^48, exact in a double)
  else if (n == "dim") *value = g->dim;
  else if (n == "scratch_bytes") *value = (double)g->scratch_bytes;
  else if (n == "scratch_limit_bytes") *value = (double)GALLERY_SCRATCH_MAX;
  else if (n == "query_block") *value = g->qb_max;
  else if (n == "positive_chunk") *value = RT_CHUNK;
  else if (n == "last_passes") *value = g->last_passes;
  else if (n == "last_nearest_form") *value = g->last_nearest_form;
  else if (n == "last_sim_ms") *value = g->last_sim_ms;
  else if (n == "last_device_ms") *value = g->last_device_ms;
  else if (n == "last_knn_vote_ms") *value = g->last_knn_vote_ms;
  else return fail(VV_ERR_ARG, "vv_gallery_get: unknown name '%s'", name);
  return VV_OK;
}

// One query block: rows [q0, q0 + rows) of the host queries to the device, their distances to every reference item into the scratch.
// q == NULL: the query rows are the gallery's own device rows from q0, nothing is uploaded.
static int gallery_block_sim(vv_ctx* c, vv_gallery* g, const float* q, int q0, int rows) {
  const float* qrows = q ? g->qdev : g->feat + (size_t)q0 * g->Dp;
  if (q) HIPCHK(hipMemcpy2DAsync(g->qdev, (size_t)g->Dp * 4, q + (size_t)q0 * g->dim, (size_t)g->dim * 4, (size_t)g->dim * 4, (size_t)rows,
                                 hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipEventRecord(g->ev[2], c->stream));
  launch_sim_f32(qrows, g->feat, g->dist, rows, (int)g->n_ref, g->Dp, g->pitch, c->stream);
  HIPCHK(hipEventRecord(g->ev[3], c->stream));
  return VV_OK;
}
static int gallery_block_done(vv_ctx* c, vv_gallery* g) {     // after the block's results are on the host (the stream is idle)
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, g->ev[2], g->ev[3]));
  g->last_sim_ms += ms;
  return VV_OK;
}
// Every query call starts here: the rows of its blocks (vv_gallery_plan.h), the scratch for them, the call's timers.  cls / sel: as
// gallery_ensure_scratch
static int gallery_call_begin(vv_ctx* c, vv_gallery* g, const char* who, int n_q, bool cls = false, bool sel = false) {
  const int block = gallery_block_rows(*g, n_q, cls, sel);
  if (block < 1) return fail(VV_ERR_ARG, "%s: %lld items do not fit one query row into the scratch limit", who, (long long)g->n_ref);
  const int rc = gallery_ensure_scratch(g, block, cls, sel);
  if (rc) return rc;
  g->last_sim_ms = 0; g->last_device_ms = 0; g->last_passes = 0;
  HIPCHK(hipEventRecord(g->ev[0], c->stream));
  return VV_OK;
}
static int gallery_call_end(vv_ctx* c, vv_gallery* g) {
  HIPCHK(hipEventRecord(g->ev[1], c->stream));
  HIPCHK(hipEventSynchronize(g->ev[1]));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, g->ev[0], g->ev[1]));
  g->last_device_ms = ms;
  return VV_OK;
}

int vv_gallery_topk(vv_ctx* c, vv_gallery* g, const float* q, int32_t n_q, int32_t k, int32_t* idx, float* dist) {
  if (!c || !g || !q || !idx || !dist) return fail(VV_ERR_ARG, "vv_gallery_topk: NULL argument");
  if (g->ctx != c) return fail(VV_ERR_ARG, "vv_gallery_topk: the gallery belongs to another context");
  if (n_q < 1) return fail(VV_ERR_ARG, "vv_gallery_topk: n_q = %d", n_q);
  if (k < 1 || k > RT_MAX_K) return fail(VV_ERR_ARG, "vv_gallery_topk: k = %d is outside 1 .. %d", k, RT_MAX_K);
  if (k > g->n_ref) return fail(VV_ERR_ARG, "vv_gallery_topk: k = %d exceeds the gallery's %lld items", k, (long long)g->n_ref);
  VV_ENTER(c);
  int rc = gallery_call_begin(c, g, "vv_gallery_topk", n_q);
  if (rc) return rc;
  for (int q0 = 0; q0 < n_q; q0 += g->qb_cap) {
    const int rows = std::min(g->qb_cap, n_q - q0);
    if ((rc = gallery_block_sim(c, g, q, q0, rows))) return rc;
    launch_topk(g->dist, g->pitch, rows, (int)g->n_ref, k, g->seg, g->S, g->part, g->out_idx, g->out_dist, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(idx + (size_t)q0 * k, g->out_idx, (size_t)rows * k * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(dist + (size_t)q0 * k, g->out_dist, (size_t)rows * k * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if ((rc = gallery_block_done(c, g))) return rc;
  }
  return gallery_call_end(c, g);
}

// vv_gallery_nearest / vv_gallery_nearest_self.  q == NULL: the self form -- the rows of a block are the gallery's own device rows
// and no item is eligible for itself; q_ids (host queries) / exclude (self form): only items of another id are eligible.
// k below the context's "nearest_select_min_k": the streaming top-k with that predicate; otherwise the selection form.  Either
// way the lists are read off the floats k_sim_f32 stored in the block's scratch rows.
// The block's lists go to one of two sinks: the host arrays idx / dist (vote == NULL), or k_knn_vote, which reads them where they are
// and writes the block's rows of vote->out_dev (vv_gallery_knn_scores*: the lists are not downloaded).
struct KnnVote {
  const int32_t* labels_dev;             // [n_ref], every entry in [0, C)
  int C, exp_weights; float T;
  float* out_dev;                        // [n_q][C]
  int32_t* n_used;                       // host [n_q] or NULL
};
static int gallery_nearest_run(vv_ctx* c, vv_gallery* g, const float* q, int n_q, const int32_t* q_ids, bool exclude, int k,
                               int32_t* idx, float* dist, const KnnVote* vote = nullptr) {
  const bool self = q == nullptr, select = k >= c->nearest_select_min_k;
  int rc = gallery_call_begin(c, g, vote ? "vv_gallery_knn_scores" : "vv_gallery_nearest", n_q, false, select);
  if (rc) return rc;
  g->last_nearest_form = select ? 2 : 1;
  if (vote) g->last_knn_vote_ms = 0;
  const int ng = (int)g->n_ref;
  for (int q0 = 0; q0 < n_q; q0 += g->qb_cap) {
    const int rows = std::min(g->qb_cap, n_q - q0);
    const int32_t* own = nullptr;                                       // device: the id whose items row r may not list
    if (self) {
      if (exclude) own = g->ref_ids + q0;
    } else if (q_ids) {
      HIPCHK(hipMemcpyAsync(g->qids, q_ids + q0, (size_t)rows * 4, hipMemcpyHostToDevice, c->stream));
      own = g->qids;
    }
    if ((rc = gallery_block_sim(c, g, q, q0, rows))) return rc;
    const int32_t* d_idx = g->out_idx; const float* d_dist = g->out_dist;
    if (select) {
      HIPCHK(hipMemsetAsync(g->sel_st, 0, (size_t)rows * 4 * 4, c->stream));
      HIPCHK(hipMemsetAsync(g->sel_hist, 0, (size_t)rows * RT_SEL_BINS * 4, c->stream));
      launch_select(g->dist, g->pitch, rows, ng, k, g->seg, g->S, g->ref_ids, own, self ? q0 : -1, g->sel_st, g->sel_hist,
                    g->sel_segh, g->skeys, g->nn_idx, g->nn_dist, c->stream);
      d_idx = g->nn_idx; d_dist = g->nn_dist;
    } else {
      launch_topk_eligible(g->dist, g->pitch, rows, ng, k, g->seg, g->S, g->ref_ids, own, self ? q0 : -1, g->part, g->out_idx,
                           g->out_dist, c->stream);
    }
    HIPCHK(hipGetLastError());
    if (vote) {                                                         // both forms leave rows of k entries; pcount: the rows' m
      HIPCHK(hipEventRecord(g->ev[4], c->stream));
      c->last_knn_form = launch_knn_vote(d_idx, d_dist, k, rows, k, vote->exp_weights, vote->T, vote->labels_dev, vote->C,
                                         vote->out_dev + (size_t)q0 * vote->C, g->pcount, c->stream);
      HIPCHK(hipEventRecord(g->ev[5], c->stream));
      HIPCHK(hipGetLastError());
      if (vote->n_used) HIPCHK(hipMemcpyAsync(vote->n_used + q0, g->pcount, (size_t)rows * 4, hipMemcpyDeviceToHost, c->stream));
    } else {
      HIPCHK(hipMemcpyAsync(idx + (size_t)q0 * k, d_idx, (size_t)rows * k * 4, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(dist + (size_t)q0 * k, d_dist, (size_t)rows * k * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));                            // (the next block's upload reuses qdev)
    if ((rc = gallery_block_done(c, g))) return rc;
    if (vote) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, g->ev[4], g->ev[5]));
      g->last_knn_vote_ms += ms;
    }
  }
  return gallery_call_end(c, g);
}

int vv_gallery_nearest(vv_ctx* c, vv_gallery* g, const float* q, int32_t n_q, const int32_t* q_ids, int32_t k, int32_t* idx,
                       float* dist) {
  if (!c || !g || !q || !idx || !dist) return fail(VV_ERR_ARG, "vv_gallery_nearest: NULL argument");
  if (g->ctx != c) return fail(VV_ERR_ARG, "vv_gallery_nearest: the gallery belongs to another context");
  if (n_q < 1) return fail(VV_ERR_ARG, "vv_gallery_nearest: n_q = %d", n_q);
  if (k < 1 || k > RT_CHUNK) return fail(VV_ERR_ARG, "vv_gallery_nearest: k = %d is outside 1 .. %d", k, RT_CHUNK);
  if (q_ids && !g->ref_ids) return fail(VV_ERR_ARG, "vv_gallery_nearest: q_ids given, but the gallery was created without ids");
  VV_ENTER(c);
  return gallery_nearest_run(c, g, q, n_q, q_ids, false, k, idx, dist);
}

int vv_gallery_nearest_self(vv_ctx* c, vv_gallery* g, int32_t k, int exclude_same_id, int32_t* idx, float* dist) {
  if (!c || !g || !idx || !dist) return fail(VV_ERR_ARG, "vv_gallery_nearest_self: NULL argument");
  if (g->ctx != c) return fail(VV_ERR_ARG, "vv_gallery_nearest_self: the gallery belongs to another context");
  if (k < 1 || k > RT_CHUNK) return fail(VV_ERR_ARG, "vv_gallery_nearest_self: k = %d is outside 1 .. %d", k, RT_CHUNK);
  if (exclude_same_id && !g->ref_ids) return fail(VV_ERR_ARG, "vv_gallery_nearest_self: exclude_same_id, but the gallery was created without ids");
  VV_ENTER(c);
  return gallery_nearest_run(c, g, nullptr, (int)g->n_ref, nullptr, exclude_same_id != 0, k, idx, dist);
}

// What the two k-NN calls share: every refusal (nothing is launched or written before the last of them has passed), the labels'
// upload -- one [n_ref] device array per call -- and the run.  q == NULL: the self form.
static int gallery_knn_run(vv_ctx* c, vv_gallery* g, const char* who, const int32_t* labels, int num_classes, const float* q, int n_q,
                           const int32_t* q_ids, bool exclude, int k, int weighting, float temperature, float* out_dev, int32_t* n_used) {
  if (g->ctx != c) return fail(VV_ERR_ARG, "%s: the gallery belongs to another context", who);
  if (n_q < 1) return fail(VV_ERR_ARG, "%s: n_q = %d", who, n_q);
  if (k < 1 || k > RT_CHUNK) return fail(VV_ERR_ARG, "%s: k = %d is outside 1 .. %d", who, k, RT_CHUNK);
  if (num_classes < 1 || num_classes > 4096) return fail(VV_ERR_ARG, "%s: num_classes = %d is outside 1 .. 4096", who, num_classes);
  if (weighting != VV_KNN_UNIFORM && weighting != VV_KNN_EXP) return fail(VV_ERR_ARG, "%s: unknown weighting %d", who, weighting);
  if (weighting == VV_KNN_EXP && !(std::isfinite(temperature) && temperature > 0.f))
    return fail(VV_ERR_ARG, "%s: temperature = %g is not a finite positive number", who, (double)temperature);
  if ((q_ids || exclude) && !g->ref_ids) return fail(VV_ERR_ARG, "%s: q_ids / exclude_same_id, but the gallery was created without ids", who);
  for (int64_t i = 0; i < g->n_ref; ++i)
    if (labels[i] < 0 || labels[i] >= num_classes)
      return fail(VV_ERR_ARG, "%s: labels[%lld] = %d is outside 0 .. %d", who, (long long)i, labels[i], num_classes - 1);
  VV_ENTER(c);
  DevTmp<int32_t> dl;
  HIPCHK(dl.alloc((size_t)g->n_ref));
  HIPCHK(hipMemcpyAsync(dl, labels, (size_t)g->n_ref * 4, hipMemcpyHostToDevice, c->stream));
  const KnnVote vote{dl, num_classes, weighting == VV_KNN_EXP, temperature, out_dev, n_used};
  const int rc = gallery_nearest_run(c, g, q, n_q, q_ids, exclude, k, nullptr, nullptr, &vote);
  if (rc) (void)hipStreamSynchronize(c->stream);                        // (dl is released on return)
  return rc;
}

int vv_gallery_knn_scores(vv_ctx* c, vv_gallery* g, const int32_t* labels, int32_t num_classes, const float* q, int32_t n_q,
                          const int32_t* q_ids, int32_t k, int32_t weighting, float temperature, float* out_dev, int32_t* n_used) {
  if (!c || !g || !labels || !q || !out_dev) return fail(VV_ERR_ARG, "vv_gallery_knn_scores: NULL argument");
  return gallery_knn_run(c, g, "vv_gallery_knn_scores", labels, num_classes, q, n_q, q_ids, false, k, weighting, temperature, out_dev, n_used);
}

int vv_gallery_knn_scores_self(vv_ctx* c, vv_gallery* g, const int32_t* labels, int32_t num_classes, int32_t k, int exclude_same_id,
                               int32_t weighting, float temperature, float* out_dev, int32_t* n_used) {
  if (!c || !g || !labels || !out_dev) return fail(VV_ERR_ARG, "vv_gallery_knn_scores_self: NULL argument");
  return gallery_knn_run(c, g, "vv_gallery_knn_scores_self", labels, num_classes, nullptr, (int)g->n_ref, nullptr, exclude_same_id != 0, k,
                         weighting, temperature, out_dev, n_used);
}

int vv_gallery_rank_stats(vv_ctx* c, vv_gallery* g, const float* q, int32_t n_q, const int32_t* q_ids, vv_rank_stats* out,
                          int32_t* best_rank, float* ap, int32_t* top5_idx, float* top5_dist) {
  if (!c || !g || !q || !q_ids || !out) return fail(VV_ERR_ARG, "vv_gallery_rank_stats: NULL argument");
  if (g->ctx != c) return fail(VV_ERR_ARG, "vv_gallery_rank_stats: the gallery belongs to another context");
  if (!g->ref_ids) return fail(VV_ERR_ARG, "vv_gallery_rank_stats: the gallery was created without reference ids");
  if (n_q < 1) return fail(VV_ERR_ARG, "vv_gallery_rank_stats: n_q = %d", n_q);
  if ((top5_idx != nullptr) != (top5_dist != nullptr)) return fail(VV_ERR_ARG, "vv_gallery_rank_stats: top5_idx and top5_dist go together");
  VV_ENTER(c);
  int rc = gallery_call_begin(c, g, "vv_gallery_rank_stats", n_q);
  if (rc) return rc;
  const int k5 = (int)std::min<int64_t>(5, g->n_ref);
  std::vector<int32_t> hstart, hcount, ranks((size_t)n_q), t5i; std::vector<float> t5d;
  std::vector<RankAcc> hacc;
  double s1 = 0, s5 = 0, s10 = 0, sap = 0;                                                     // :150
  for (int q0 = 0; q0 < n_q; q0 += g->qb_cap) {
    const int rows = std::min(g->qb_cap, n_q - q0);
    hstart.assign(rows, 0); hcount.assign(rows, 0); hacc.assign(rows, RankAcc{0.0, 10000, 0, 0, 0});   // :68-70
    int max_p = 0;
    for (int i = 0; i < rows; ++i) {
      const auto it = std::lower_bound(g->uid.begin(), g->uid.end(), q_ids[q0 + i]);
      if (it == g->uid.end() || *it != q_ids[q0 + i]) continue;                                // an id the gallery does not hold
      const size_t u = it - g->uid.begin();
      hstart[i] = g->ustart[u]; hcount[i] = g->ustart[u + 1] - g->ustart[u];
      max_p = std::max(max_p, hcount[i]);
    }
    HIPCHK(hipMemcpyAsync(g->pstart, hstart.data(), (size_t)rows * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g->pcount, hcount.data(), (size_t)rows * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g->qids, q_ids + q0, (size_t)rows * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g->acc, hacc.data(), (size_t)rows * sizeof(RankAcc), hipMemcpyHostToDevice, c->stream));
    if ((rc = gallery_block_sim(c, g, q, q0, rows))) return rc;
    const int passes = (max_p + RT_CHUNK - 1) / RT_CHUNK;
    g->last_passes = std::max(g->last_passes, passes);
    for (int pass = 0; pass < passes; ++pass) {
      HIPCHK(hipMemsetAsync(g->bins, 0, (size_t)rows * 2 * RT_CHUNK * 4, c->stream));
      launch_rank_pass(g->dist, g->pitch, rows, (int)g->n_ref, g->seg, g->S, g->pos_idx, g->pstart, g->pcount, g->qids, g->ref_ids,
                       pass, g->bins, g->acc, c->stream);
    }
    if (top5_idx) {
      launch_topk(g->dist, g->pitch, rows, (int)g->n_ref, k5, g->seg, g->S, g->part, g->out_idx, g->out_dist, c->stream);
      t5i.resize((size_t)rows * k5); t5d.resize((size_t)rows * k5);
      HIPCHK(hipMemcpyAsync(t5i.data(), g->out_idx, t5i.size() * 4, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(t5d.data(), g->out_dist, t5d.size() * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hacc.data(), g->acc, (size_t)rows * sizeof(RankAcc), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if ((rc = gallery_block_done(c, g))) return rc;
    for (int i = 0; i < rows; ++i) {
      const RankAcc& a = hacc[i];
      const double ret = hcount[i];
      double qap = 0, r5 = a.acc5, r10 = a.acc10;
      if (ret > 0) { qap = a.ap_sum / ret; r5 /= ret < 5 ? ret : 5; r10 /= ret < 10 ? ret : 10; }   // :95-108
      sap += qap; s1 += a.acc1; s5 += r5; s10 += r10;                                               // :172-176
      ranks[q0 + i] = a.best;
      if (best_rank) best_rank[q0 + i] = a.best;
      if (ap) ap[q0 + i] = (float)qap;
      if (top5_idx)
        for (int j = 0; j < 5; ++j) {                          // fewer than five reference items: index -1, distance 0
          top5_idx[(size_t)(q0 + i) * 5 + j] = j < k5 ? t5i[(size_t)i * k5 + j] : -1;
          top5_dist[(size_t)(q0 + i) * 5 + j] = j < k5 ? t5d[(size_t)i * k5 + j] : 0.f;
        }
    }
  }
  std::sort(ranks.begin(), ranks.end());                                                            // :218-224
  out->median_rank = (float)(n_q % 2 == 0 ? (ranks[n_q / 2 - 1] + ranks[n_q / 2]) / 2.0 : (double)ranks[n_q / 2]);
  out->recall_1 = (float)(s1 / n_q); out->recall_5 = (float)(s5 / n_q); out->recall_10 = (float)(s10 / n_q);   // :226-230
  out->mean_ap = (float)(sap / n_q);
  return gallery_call_end(c, g);
}

// One item per distinct id, ids ascending: the video-level features of RetrievalStatsLayer (retrieval_stats_layer.cpp:165-198;
// the reference enumerates the videos in boost::unordered_map order, which is unspecified).
int vv_gallery_pool_by_id(vv_ctx* c, vv_gallery* g, vv_gallery** out) {
  if (!c || !g || !out) return fail(VV_ERR_ARG, "vv_gallery_pool_by_id: NULL argument");
  if (g->ctx != c) return fail(VV_ERR_ARG, "vv_gallery_pool_by_id: the gallery belongs to another context");
  if (!g->ref_ids) return fail(VV_ERR_ARG, "vv_gallery_pool_by_id: the gallery was created without ids");
  VV_ENTER(c);
  const int n_ids = (int)g->uid.size();
  DevTmp<int32_t> dstart;
  HIPCHK(dstart.alloc((size_t)n_ids + 1));
  HIPCHK(hipMemcpyAsync(dstart, g->ustart.data(), ((size_t)n_ids + 1) * 4, hipMemcpyHostToDevice, c->stream));
  vv_gallery* p = new vv_gallery;
  int rc = gallery_init(c, p, n_ids, g->dim, g->uid.data());
  if (!rc) {
    launch_pool_by_id(g->feat, g->Dp, g->pos_idx, dstart, n_ids, p->feat, c->stream);
    const hipError_t e = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || e2 != hipSuccess) rc = fail(VV_ERR_HIP, "vv_gallery_pool_by_id: %s", hipGetErrorString(e != hipSuccess ? e : e2));
  }
  if (rc) { gallery_release(p); return rc; }
  *out = p;
  return VV_OK;
}

// The class of every item and the per-class item lists for one id -> class map (an id absent from it: class 0, :110, :117; an id
// listed twice: the later entry, as vv_retrieval_stats reads the same arrays).  Kept until a different map arrives.
static int gallery_class_lists(vv_gallery* g, const int32_t* map_ids, const int32_t* map_cls, int32_t n_map) {
  if (g->cls && (int32_t)g->cs_map_ids.size() == n_map && std::equal(map_ids, map_ids + n_map, g->cs_map_ids.begin()) &&
      std::equal(map_cls, map_cls + n_map, g->cs_map_cls.begin()))
    return VV_OK;
  const int64_t n = g->n_ref;
  std::unordered_map<int, int> m;
  for (int i = 0; i < n_map; ++i) m[map_ids[i]] = map_cls[i];
  std::vector<int32_t> ucls(g->uid.size());
  for (size_t u = 0; u < g->uid.size(); ++u) { const auto it = m.find(g->uid[u]); ucls[u] = it == m.end() ? 0 : it->second; }
  g->h_cls.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i)
    g->h_cls[i] = ucls[std::lower_bound(g->uid.begin(), g->uid.end(), g->h_ids[i]) - g->uid.begin()];
  std::vector<int32_t> order((size_t)n);
  for (int64_t i = 0; i < n; ++i) order[i] = (int32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return g->h_cls[a] < g->h_cls[b]; });
  g->cvals.clear(); g->cstart.clear();
  for (int64_t i = 0; i < n; ++i)
    if (i == 0 || g->h_cls[order[i]] != g->h_cls[order[i - 1]]) { g->cvals.push_back(g->h_cls[order[i]]); g->cstart.push_back((int32_t)i); }
  g->cstart.push_back((int32_t)n);
  g->cs_map_ids.clear();                                                   // (nothing valid until both uploads are queued)
  if (!g->cls) { HIPCHK(hipMalloc((void**)&g->cls, (size_t)n * 4)); HIPCHK(hipMalloc((void**)&g->cpos, (size_t)n * 4)); }
  HIPCHK(hipMemcpy(g->cls, g->h_cls.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g->cpos, order.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  g->cs_map_ids.assign(map_ids, map_ids + n_map); g->cs_map_cls.assign(map_cls, map_cls + n_map);
  return VV_OK;
}

// RetrievalStatsLayer::Forward_cpu (:213-304, :351-353) with ComputeStats (:104-141) over the gallery's own items: every item is a
// query against all the others.  The counts come from kernels_retrieval.hip; the host divides and averages.
int vv_gallery_class_stats(vv_ctx* c, vv_gallery* g, const int32_t* map_ids, const int32_t* map_cls, int32_t n_map,
                           int exclude_same_id, vv_class_stats* out, float* ap, float* acc1, float* acc5, int32_t* top5_idx) {
  if (!c || !g || !out || (n_map > 0 && (!map_ids || !map_cls))) return fail(VV_ERR_ARG, "vv_gallery_class_stats: NULL argument");
  if (g->ctx != c) return fail(VV_ERR_ARG, "vv_gallery_class_stats: the gallery belongs to another context");
  if (!g->ref_ids) return fail(VV_ERR_ARG, "vv_gallery_class_stats: the gallery was created without ids");
  if (n_map < 1) return fail(VV_ERR_ARG, "need atleast one entry in id-to-class map!");              // :48
  VV_ENTER(c);
  int rc = gallery_class_lists(g, map_ids, map_cls, n_map);
  if (rc) return rc;
  const int n = (int)g->n_ref;
  int n_scored = 0;
  for (int i = 0; i < n; ++i) n_scored += g->h_cls[i] >= 0;
  if (n_scored == 0) return fail(VV_ERR_ARG, "vv_gallery_class_stats: no item with a non-negative class");
  if ((rc = gallery_call_begin(c, g, "vv_gallery_class_stats", n, true))) return rc;
  // counting segments: long ones, a workgroup's bins are flushed once per segment
  const int cseg = std::max(g->seg, 65536), cS = (n + cseg - 1) / cseg;
  ClassAcc* dacc = reinterpret_cast<ClassAcc*>(g->acc);
  std::vector<int32_t> hstart, hcount, t5; std::vector<ClassAcc> hacc;
  double s_ap = 0, s_1 = 0, s_5 = 0;                                                                   // :213
  const float nanv = std::numeric_limits<float>::quiet_NaN();
  for (int q0 = 0; q0 < n; q0 += g->qb_cap) {
    const int rows = std::min(g->qb_cap, n - q0);
    hstart.assign(rows, 0); hcount.assign(rows, 0); hacc.resize(rows);
    int max_p = 0;
    for (int i = 0; i < rows; ++i) {
      const int32_t cl = g->h_cls[q0 + i];
      if (cl < 0) continue;                                                                            // :250-252
      const size_t u = std::lower_bound(g->cvals.begin(), g->cvals.end(), cl) - g->cvals.begin();
      hstart[i] = g->cstart[u]; hcount[i] = g->cstart[u + 1] - g->cstart[u];
      max_p = std::max(max_p, hcount[i]);
    }
    HIPCHK(hipMemcpyAsync(g->pstart, hstart.data(), (size_t)rows * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g->pcount, hcount.data(), (size_t)rows * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(dacc, 0, (size_t)rows * sizeof(ClassAcc), c->stream));
    if ((rc = gallery_block_sim(c, g, nullptr, q0, rows))) return rc;  // the query rows are the gallery's own device rows (:208-209)
    const int passes = (max_p + RT_CHUNK - 1) / RT_CHUNK;
    g->last_passes = std::max(g->last_passes, passes);
    for (int pass = 0; pass < passes; ++pass) {
      HIPCHK(hipMemsetAsync(g->cbins, 0, (size_t)rows * 3 * RT_CHUNK * 4, c->stream));
      launch_class_pass(g->dist, g->pitch, rows, n, cseg, cS, g->cpos, g->pstart, g->pcount, g->ref_ids, g->cls, q0,
                        exclude_same_id ? 1 : 0, pass, g->skeys, g->cbins, dacc, c->stream);
    }
    if (top5_idx) {                                                                                    // :310-316
      launch_topk_other_id(g->dist, g->pitch, rows, n, 5, g->seg, g->S, g->ref_ids, q0, g->part, g->out_idx, g->out_dist, c->stream);
      t5.resize((size_t)rows * 5);
      HIPCHK(hipMemcpyAsync(t5.data(), g->out_idx, t5.size() * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hacc.data(), dacc, (size_t)rows * sizeof(ClassAcc), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if ((rc = gallery_block_done(c, g))) return rc;
    for (int i = 0; i < rows; ++i) {
      const bool scored = g->h_cls[q0 + i] >= 0;
      const ClassAcc& a = hacc[i];
      const double qap = a.npos > 0 ? a.ap_sum / a.npos : 0.0, q1 = a.acc1, q5 = a.n5 / 5.0;          // :131-135
      if (scored) { s_ap += qap; s_1 += q1; s_5 += q5; }                                               // :297-301
      if (ap) ap[q0 + i] = scored ? (float)qap : nanv;
      if (acc1) acc1[q0 + i] = scored ? (float)q1 : nanv;
      if (acc5) acc5[q0 + i] = scored ? (float)q5 : nanv;
      if (top5_idx)
        for (int j = 0; j < 5; ++j) top5_idx[(size_t)(q0 + i) * 5 + j] = scored ? t5[(size_t)i * 5 + j] : -1;
    }
  }
  out->mean_ap = (float)(s_ap / n_scored); out->hit_at_1 = (float)(s_1 / n_scored); out->hit_at_5 = (float)(s_5 / n_scored);   // :351-353
  out->n_scored = n_scored;
  return gallery_call_end(c, g);
}

// The fp32 dot products of a query block, as the other gallery calls see them: the float k_sim_f32 stored, times -0.5f.
int vv_gallery_scores(vv_ctx* c, vv_gallery* g, const float* q, int32_t n_q, float* out_dev) {
  if (!c || !g || !q || !out_dev) return fail(VV_ERR_ARG, "vv_gallery_scores: NULL argument");
  if (g->ctx != c) return fail(VV_ERR_ARG, "vv_gallery_scores: the gallery belongs to another context");
  if (n_q < 1) return fail(VV_ERR_ARG, "vv_gallery_scores: n_q = %d", n_q);
  VV_ENTER(c);
  int rc = gallery_call_begin(c, g, "vv_gallery_scores", n_q);
  if (rc) return rc;
  for (int q0 = 0; q0 < n_q; q0 += g->qb_cap) {
    const int rows = std::min(g->qb_cap, n_q - q0);
    if ((rc = gallery_block_sim(c, g, q, q0, rows))) return rc;
    launch_scores_out(g->dist, g->pitch, rows, (int)g->n_ref, out_dev + (size_t)q0 * g->n_ref, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));                   // (the next block's upload reuses qdev)
    if ((rc = gallery_block_done(c, g))) return rc;
  }
  return gallery_call_end(c, g);
}

}  // extern "C"
