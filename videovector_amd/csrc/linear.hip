// linear.hip -- entry points of the linear classifier on gallery embeddings, under the softmax loss or the one-vs-rest hinge loss
// (include/videovec.h: vv_linear_*, vv_op_softmax_loss, vv_op_hinge_loss, vv_op_gemm_tn).  The kernels are in kernels_linear.hip; the logits' product is launch_sim_f32
// (kernels_retrieval.hip) on W kept as [Cp][Dp] rows, zero-padded the way a gallery is.  Everything is queued on the context's
// stream; a fit synchronises once, at its end.  None of this reads or writes the training step's state.
// vv_linear_fit_rows / _grad_rows / _scores_rows run the same steps on a LIST of gallery rows (shuffled epochs, folds; the lists are
// vv_rows.h's): the reference's counterpart is only its data order, the database cursor of data_layer.cpp:53, 180-198; the lists are
// this project's own.  check_rows is the host check that keeps a bad index from every kernel.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "vv_ctx.h"
#include "vv_rows.h"

using namespace vv;

#define NEED(c) do { if (!(c)) return vv_fail(VV_ERR_ARG, "%s: ctx is NULL", __func__); HIPCHK(hipSetDevice((c)->device)); vv::g_ko = &(c)->ko; } while (0)

static constexpr int LIN_MAX_CLASSES = 4096;

struct vv_linear {
  vv_ctx* ctx = nullptr;
  int dim = 0, Dp = 0, C = 0, Cp = 0, bias = 0;
  int64_t cursor = 0, steps = 0;
  int loss = VV_LIN_LOSS_SOFTMAX, norm = VV_NORM_L2;        // vv_linear_loss_set; norm is read under VV_LIN_LOSS_HINGE only
  float* P = nullptr;                       // ONE allocation: W [Cp][Dp] | hW [Cp][Dp] | b [Cp] | hb [Cp], pads zero
  float *W = nullptr, *hW = nullptr, *b = nullptr, *hb = nullptr;
  // scratch, grown on demand and kept between calls
  float *z = nullptr, *dz = nullptr; int64_t z_rows = 0;          // [rows][Cp] each
  float *slabs = nullptr, *dbs = nullptr; int slab_S = 0;        // [S][Cp][Dp], [S][Cp]
  double* part_loss = nullptr;                                   // k_softmax_xent's partials, then its arrival counter (sm_parts)
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

namespace {

inline bool aligned16(const void* p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

// the softmax kernel's partial buffers: [LIN_SM_BLOCKS] doubles, [LIN_SM_BLOCKS][2] counts, the arrival counter
constexpr size_t kSmPartBytes = (size_t)LIN_SM_BLOCKS * 8 + (size_t)LIN_SM_BLOCKS * 2 * 4 + 16;

template <class Args> void sm_parts(void* base, Args& a) {
  a.part_loss = (double*)base;
  a.part_cnt = (uint32_t*)((char*)base + (size_t)LIN_SM_BLOCKS * 8);
  a.arrived = a.part_cnt + (size_t)LIN_SM_BLOCKS * 2;
}

int ensure_rows(vv_ctx* c, vv_linear* l, int64_t rows) {
  if (rows <= l->z_rows) return VV_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  dfree(l->z); dfree(l->dz); l->z = l->dz = nullptr; l->z_rows = 0;
  HIPCHK(hipMalloc((void**)&l->z, (size_t)rows * l->Cp * 4));
  HIPCHK(hipMalloc((void**)&l->dz, (size_t)rows * l->Cp * 4));
  l->z_rows = rows;
  return VV_OK;
}
int ensure_slabs(vv_ctx* c, vv_linear* l, int S) {
  if (S <= l->slab_S) return VV_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  dfree(l->slabs); dfree(l->dbs); l->slabs = l->dbs = nullptr; l->slab_S = 0;
  HIPCHK(hipMalloc((void**)&l->slabs, (size_t)S * l->Cp * l->Dp * 4));
  HIPCHK(hipMalloc((void**)&l->dbs, (size_t)S * l->Cp * 4));
  l->slab_S = S;
  return VV_OK;
}

// rows of one row block of a batch of `count` rows: the split plan's, and logits + dz within the gallery path's scratch limit
struct BatchPlan { LinPlan p; int64_t block_rows; int blocks; };
BatchPlan batch_plan(const vv_ctx* c, const vv_linear* l, int64_t count) {
  BatchPlan bp;
  bp.p = lin_plan(count, l->Cp, l->Dp, c->lin_split_rows);
  const int64_t fit = std::max<int64_t>(1, (int64_t)(GALLERY_SCRATCH_MAX / ((size_t)2 * l->Cp * 4)));
  bp.block_rows = std::min(bp.p.block_rows, fit / bp.p.split_rows * bp.p.split_rows);      // (whole splits)
  if (bp.block_rows < 1) bp.block_rows = std::min(bp.p.block_rows, fit);
  bp.block_rows = std::min(bp.block_rows, count);
  bp.blocks = (int)((count + bp.block_rows - 1) / bp.block_rows);
  bp.p.S = (int)((bp.block_rows + bp.p.split_rows - 1) / bp.p.split_rows);
  return bp;
}

int check_pair(const char* who, vv_ctx* c, vv_linear* l, vv_gallery* g, GalleryRows* gr) {
  if (!l) return vv_fail(VV_ERR_ARG, "%s: the classifier is NULL", who);
  if (l->ctx != c) return vv_fail(VV_ERR_ARG, "%s: the classifier belongs to another context", who);
  if (g) {
    *gr = gallery_rows(g);
    if (gr->ctx != c) return vv_fail(VV_ERR_ARG, "%s: the gallery belongs to another context", who);
    if (gr->dim != l->dim) return vv_fail(VV_ERR_ARG, "%s: the gallery's dimension %d differs from the classifier's %d", who, gr->dim, l->dim);
  }
  return VV_OK;
}
// hinge_loss_layer.cpp:68 and :71, each evaluated left to right in fp32
float hinge_scale(int norm, float loss_weight, int64_t count) {
  if (norm == VV_NORM_L1) return loss_weight / (float)count;
  const float twice = loss_weight * 2.0f;
  return twice / (float)count;
}
int check_labels(const char* who, const int32_t* labels, int64_t n, int C) {
  for (int64_t i = 0; i < n; ++i)
    if (labels[i] < 0 || labels[i] >= C) return vv_fail(VV_ERR_ARG, "%s: label %d of item %lld is outside 0 .. %d", who, labels[i], (long long)i, C - 1);
  return VV_OK;
}

// One batch: logits, the selected loss (softmax / cross-entropy, or the hinge loss) and the weight-gradient product of rows [first, first + count), row block by row
// block in order; the slabs then hold the batch's gradient in bp.p.S splits.  ev: NULL, or four events recorded around the legs of
// the batch (the last row block's).  rows_dev NULL: the rows are gallery items first .. first + count - 1 and labels_dev is by item.
// Else `first` and `count` are positions in the list rows_dev (device; every entry checked on the host to lie in [0, n_ref)), labels_dev
// is by position, and both products run their gathered forms; the loss kernels and everything behind them see no difference.
int queue_batch(vv_ctx* c, vv_linear* l, const GalleryRows& gr, const int32_t* rows_dev, const int32_t* labels_dev, int64_t first, int64_t count,
                float loss_weight, const BatchPlan& bp, LinRec* rec, hipEvent_t* ev) {
  const float scale = loss_weight / (float)count;
  for (int blk = 0; blk < bp.blocks; ++blk) {
    const int64_t r0 = first + (int64_t)blk * bp.block_rows, rows = std::min(bp.block_rows, first + count - r0);
    const float* X = rows_dev ? gr.feat : gr.feat + r0 * gr.Dp;
    const bool timed = ev && blk == bp.blocks - 1;
    if (timed) HIPCHK(hipEventRecord(ev[0], c->stream));
    if (rows_dev) launch_sim_f32_rows(X, rows_dev + r0, l->W, l->z, (int)rows, l->C, l->Dp, l->Cp, c->stream);
    else launch_sim_f32(X, l->W, l->z, (int)rows, l->C, l->Dp, l->Cp, c->stream);
    if (timed) HIPCHK(hipEventRecord(ev[1], c->stream));
    if (l->loss == VV_LIN_LOSS_HINGE) {
      LinHingeArgs ha;
      ha.sim = l->z; ha.pitch = l->Cp; ha.rows = rows; ha.cols = l->C; ha.mul = -0.5f; ha.bias = l->bias ? l->b : nullptr;
      ha.labels = labels_dev + r0; ha.norm = l->norm; ha.scale = hinge_scale(l->norm, loss_weight, count); ha.dz = l->dz;
      ha.wd = lin_hinge_lanes(l->C); ha.vec = 1; ha.rec = rec; ha.first_block = blk == 0;      // (hipMalloc'd, Cp % 32 == 0)
      sm_parts(l->part_loss, ha);
      launch_hinge(ha, c->stream);
      c->last_hinge_form = 1;
    } else {
      LinSoftmaxArgs sa;
      sa.sim = l->z; sa.pitch = l->Cp; sa.rows = rows; sa.cols = l->C; sa.mul = -0.5f; sa.bias = l->bias ? l->b : nullptr;
      sa.labels = labels_dev + r0; sa.scale = scale; sa.dz = l->dz; sa.prob = nullptr; sa.row_loss = nullptr; sa.row_flags = nullptr;
      sa.wd = l->C <= 32 ? 32 : 64; sa.rec = rec; sa.first_block = blk == 0;
      sm_parts(l->part_loss, sa);
      launch_softmax_xent(sa, c->stream);
    }
    if (timed) HIPCHK(hipEventRecord(ev[2], c->stream));
    LinWgradArgs wa;
    wa.A = l->dz; wa.lda = l->Cp; wa.B = X; wa.ldb = gr.Dp; wa.k = rows; wa.m = l->Cp; wa.n = l->Dp;
    wa.split_rows = bp.p.split_rows; wa.S = (int)((rows + bp.p.split_rows - 1) / bp.p.split_rows);
    wa.slabs = l->slabs; wa.slab_stride = (int64_t)l->Cp * l->Dp; wa.dbs = l->bias ? l->dbs : nullptr;
    wa.accumulate = blk > 0; wa.vec_a = 1; wa.vec_b = 1; wa.rowidx = rows_dev ? rows_dev + r0 : nullptr;
    launch_lin_wgrad(wa, c->stream);
    if (timed) HIPCHK(hipEventRecord(ev[3], c->stream));
  }
  HIPCHK(hipGetLastError());
  c->last_lin_splits = bp.p.S; c->last_lin_blocks = bp.blocks; c->last_lin_gather = rows_dev ? 2 : 1;
  return VV_OK;
}

// A row list of the caller against the gallery and the labels: every entry in [0, n_ref) and the label of every LISTED item in
// [0, C).  Nothing has been launched or changed when this refuses; it is the only thing between a bad index and a kernel.
// lab_out: labels[rows[i]], the list the loss kernels read by position (NULL: no labels wanted).
int check_rows(const char* who, const int32_t* rows, int64_t n_rows, int64_t n_ref, const int32_t* labels, int C, std::vector<int32_t>* lab_out) {
  if (n_rows < 1 || n_rows > (1ll << 30)) return vv_fail(VV_ERR_ARG, "%s: n_rows = %lld is outside 1 .. 2^30", who, (long long)n_rows);
  if (!rows) return vv_fail(VV_ERR_ARG, "%s: rows is NULL", who);
  for (int64_t i = 0; i < n_rows; ++i)
    if (rows[i] < 0 || rows[i] >= n_ref)
      return vv_fail(VV_ERR_ARG, "%s: rows[%lld] = %d is outside the gallery's items 0 .. %lld", who, (long long)i, rows[i], (long long)n_ref - 1);
  if (!labels) return VV_OK;
  lab_out->resize((size_t)n_rows);
  for (int64_t i = 0; i < n_rows; ++i) {
    const int32_t y = labels[rows[i]];
    if (y < 0 || y >= C) return vv_fail(VV_ERR_ARG, "%s: label %d of item %d (rows[%lld]) is outside 0 .. %d", who, y, rows[i], (long long)i, C - 1);
    (*lab_out)[(size_t)i] = y;
  }
  return VV_OK;
}

LinUpdArgs upd_args(const vv_linear* l, int S) {
  LinUpdArgs u;
  u.slabs = l->slabs; u.slab_stride = (int64_t)l->Cp * l->Dp; u.S = S; u.nW = (int64_t)l->Cp * l->Dp;
  u.dbs = l->dbs; u.db_stride = l->Cp; u.nb = l->bias ? l->Cp : 0;
  u.W = l->W; u.hW = l->hW; u.b = l->b; u.hb = l->hb;
  u.lr = 0.f; u.momentum = 0.f; u.wd = 0.f; u.rule = 1; u.vec = 1;
  return u;
}

}  // namespace

extern "C" {

void vv_linear_cfg_default(vv_linear_cfg* cfg) {
  if (!cfg) return;
  cfg->iters = 100; cfg->batch = 0; cfg->lr = 0.1f; cfg->momentum = 0.9f; cfg->weight_decay = 0.f; cfg->loss_weight = 1.f;
}

int vv_linear_create(vv_ctx* c, int32_t dim, int32_t num_classes, int bias, vv_linear** out) {
  NEED(c);
  if (!out) return vv_fail(VV_ERR_ARG, "vv_linear_create: out is NULL");
  if (num_classes < 1 || num_classes > LIN_MAX_CLASSES) return vv_fail(VV_ERR_ARG, "vv_linear_create: num_classes = %d is outside 1 .. %d", num_classes, LIN_MAX_CLASSES);
  if (dim < 1 || dim > 8192) return vv_fail(VV_ERR_ARG, "vv_linear_create: dim = %d is outside 1 .. 8192", dim);
  vv_linear* l = new vv_linear;
  l->ctx = c; l->dim = dim; l->Dp = (int)round_up(dim, RT_BK); l->C = num_classes; l->Cp = (int)round_up(num_classes, 32); l->bias = bias != 0;
  const size_t nW = (size_t)l->Cp * l->Dp, total = 2 * nW + 2 * (size_t)l->Cp;
  hipError_t e = hipMalloc((void**)&l->P, total * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&l->part_loss, kSmPartBytes);
  if (e == hipSuccess) e = hipMemsetAsync(l->P, 0, total * 4, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(l->part_loss, 0, kSmPartBytes, c->stream);
  for (int i = 0; i < 5 && e == hipSuccess; ++i) e = hipEventCreate(&l->ev[i]);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { vv_linear_destroy(c, l); return vv_fail(VV_ERR_HIP, "vv_linear_create: %s", hipGetErrorString(e)); }
  l->W = l->P; l->hW = l->P + nW; l->b = l->P + 2 * nW; l->hb = l->b + l->Cp;
  *out = l;
  return VV_OK;
}

int vv_linear_destroy(vv_ctx* c, vv_linear* l) {
  NEED(c);
  if (!l) return VV_OK;
  if (l->ctx != c) return vv_fail(VV_ERR_ARG, "vv_linear_destroy: the classifier belongs to another context");
  (void)hipStreamSynchronize(c->stream);
  dfree(l->P); dfree(l->z); dfree(l->dz); dfree(l->slabs); dfree(l->dbs); dfree(l->part_loss);
  for (hipEvent_t e : l->ev) if (e) (void)hipEventDestroy(e);
  delete l;
  return VV_OK;
}

int vv_linear_get(vv_ctx* c, vv_linear* l, float* W, float* b, float* hW, float* hb, int64_t* steps) {
  NEED(c);
  { const int rc = check_pair("vv_linear_get", c, l, nullptr, nullptr); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(c->stream));
  const size_t rowb = (size_t)l->dim * 4;
  if (W) HIPCHK(hipMemcpy2D(W, rowb, l->W, (size_t)l->Dp * 4, rowb, (size_t)l->C, hipMemcpyDeviceToHost));
  if (hW) HIPCHK(hipMemcpy2D(hW, rowb, l->hW, (size_t)l->Dp * 4, rowb, (size_t)l->C, hipMemcpyDeviceToHost));
  if (b) HIPCHK(hipMemcpy(b, l->b, (size_t)l->C * 4, hipMemcpyDeviceToHost));          // (bias == 0: zeros, as created)
  if (hb) HIPCHK(hipMemcpy(hb, l->hb, (size_t)l->C * 4, hipMemcpyDeviceToHost));
  if (steps) *steps = l->steps;
  return VV_OK;
}

int vv_linear_put(vv_ctx* c, vv_linear* l, const float* W, const float* b, const float* hW, const float* hb, int64_t steps) {
  NEED(c);
  { const int rc = check_pair("vv_linear_put", c, l, nullptr, nullptr); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(c->stream));
  const size_t rowb = (size_t)l->dim * 4;
  if (W) HIPCHK(hipMemcpy2D(l->W, (size_t)l->Dp * 4, W, rowb, rowb, (size_t)l->C, hipMemcpyHostToDevice));
  if (hW) HIPCHK(hipMemcpy2D(l->hW, (size_t)l->Dp * 4, hW, rowb, rowb, (size_t)l->C, hipMemcpyHostToDevice));
  if (b && l->bias) HIPCHK(hipMemcpy(l->b, b, (size_t)l->C * 4, hipMemcpyHostToDevice));
  if (hb && l->bias) HIPCHK(hipMemcpy(l->hb, hb, (size_t)l->C * 4, hipMemcpyHostToDevice));
  l->steps = steps; l->cursor = 0;
  return VV_OK;
}

// vv_linear_fit (rows NULL: the gallery's items from the object's cursor) and vv_linear_fit_rows (the list from position 0, the cursor
// neither read nor moved): one body, so the two differ in where a batch's rows come from and in nothing else.
static int fit_common(const char* who, vv_ctx* c, vv_linear* l, vv_gallery* train, const int32_t* labels, const int32_t* rows, int64_t n_rows,
                      bool by_rows, const vv_linear_cfg* cfg, const float* lr_schedule, float* loss_trace, vv_linear_report* out) {
  if (!train || !labels || !cfg || !out) return vv_fail(VV_ERR_ARG, "%s: NULL argument", who);
  GalleryRows gr;
  { const int rc = check_pair(who, c, l, train, &gr); if (rc) return rc; }
  if (cfg->iters < 1) return vv_fail(VV_ERR_ARG, "%s: iters = %d", who, cfg->iters);
  if (cfg->batch < 0) return vv_fail(VV_ERR_ARG, "%s: batch = %d", who, cfg->batch);
  std::vector<int32_t> listed;                                             // by_rows: labels[rows[i]]
  { const int rc = by_rows ? check_rows(who, rows, n_rows, gr.n_ref, labels, l->C, &listed) : check_labels(who, labels, gr.n_ref, l->C); if (rc) return rc; }
  const int64_t n = by_rows ? n_rows : gr.n_ref, batch = cfg->batch == 0 ? n : std::min<int64_t>(cfg->batch, n);
  if (!by_rows && l->cursor >= n) l->cursor = 0;                           // (a smaller gallery than the last call's)
  int64_t pos = by_rows ? 0 : l->cursor;
  // the steps' batches, by the cursor; the scratch is sized for the largest plan among them before anything is queued
  std::vector<int64_t> counts((size_t)cfg->iters);
  std::vector<BatchPlan> plans((size_t)cfg->iters);
  {
    int64_t cur = pos, rows_max = 0;
    int S_max = 0;
    for (int t = 0; t < cfg->iters; ++t) {
      counts[t] = std::min(batch, n - cur);
      plans[t] = t > 0 && counts[t] == counts[t - 1] ? plans[t - 1] : batch_plan(c, l, counts[t]);
      rows_max = std::max(rows_max, plans[t].block_rows); S_max = std::max(S_max, plans[t].p.S);
      cur += counts[t];
      if (cur >= n) cur = 0;
    }
    int rc = ensure_rows(c, l, rows_max);
    if (!rc) rc = ensure_slabs(c, l, S_max);
    if (rc) return rc;
  }
  DevTmp<int32_t> lab, idx;
  DevTmp<LinRec> recs;
  HIPCHK(lab.alloc((size_t)n));
  if (by_rows) HIPCHK(idx.alloc((size_t)n));
  HIPCHK(recs.alloc((size_t)cfg->iters));
  HIPCHK(hipMemcpyAsync(lab, by_rows ? listed.data() : labels, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  if (by_rows) HIPCHK(hipMemcpyAsync(idx, rows, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  for (int t = 0; t < cfg->iters; ++t) {
    const int64_t count = counts[t];
    const BatchPlan& bp = plans[t];
    const bool timed = t == cfg->iters - 1;
    const int rc = queue_batch(c, l, gr, by_rows ? idx.p : nullptr, lab, pos, count, cfg->loss_weight, bp, recs + t, timed ? l->ev : nullptr);
    if (rc) return rc;
    LinUpdArgs u = upd_args(l, bp.p.S);
    u.lr = lr_schedule ? lr_schedule[t] : cfg->lr; u.momentum = cfg->momentum; u.wd = cfg->weight_decay;
    launch_lin_update(u, c->stream);
    if (timed) HIPCHK(hipEventRecord(l->ev[4], c->stream));
    pos += count;
    if (pos >= n) pos = 0;
    if (!by_rows) l->cursor = pos;
    l->steps += 1;
  }
  HIPCHK(hipGetLastError());
  std::vector<LinRec> h((size_t)cfg->iters);
  HIPCHK(hipMemcpyAsync(h.data(), recs, h.size() * sizeof(LinRec), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int i = 0; i < 4; ++i) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, l->ev[i], l->ev[i + 1])); c->last_lin_ms[i] = ms; }
  // loss_t = loss_weight (1 / count_t) sum_t, formed in double and rounded once
  int64_t nonfinite = 0;
  float first_loss = 0.f, last_loss = 0.f;
  for (int t = 0; t < cfg->iters; ++t) {
    const float loss = (float)((double)cfg->loss_weight * h[t].loss_sum / (double)counts[t]);
    if (loss_trace) loss_trace[t] = loss;
    if (t == 0) first_loss = loss;
    last_loss = loss;
    nonfinite += h[t].nonfinite;
  }
  out->loss_first = first_loss; out->loss_last = last_loss;
  out->accuracy_last = (float)h.back().correct / (float)counts.back();
  out->reserved_ = 0; out->steps = l->steps; out->nonfinite_rows = nonfinite;
  return VV_OK;
}

int vv_linear_fit(vv_ctx* c, vv_linear* l, vv_gallery* train, const int32_t* labels, const vv_linear_cfg* cfg, const float* lr_schedule,
                  float* loss_trace, vv_linear_report* out) {
  NEED(c);
  return fit_common("vv_linear_fit", c, l, train, labels, nullptr, 0, false, cfg, lr_schedule, loss_trace, out);
}

int vv_linear_fit_rows(vv_ctx* c, vv_linear* l, vv_gallery* train, const int32_t* labels, const int32_t* rows, int64_t n_rows,
                       const vv_linear_cfg* cfg, const float* lr_schedule, float* loss_trace, vv_linear_report* out) {
  NEED(c);
  return fit_common("vv_linear_fit_rows", c, l, train, labels, rows, n_rows, true, cfg, lr_schedule, loss_trace, out);
}

// vv_linear_grad (rows NULL: items first .. first + count - 1) and vv_linear_grad_rows (the whole list: first 0, count n_rows)
static int grad_common(const char* who, vv_ctx* c, vv_linear* l, vv_gallery* train, const int32_t* labels, const int32_t* rows, bool by_rows,
                       int64_t first, int64_t count, float loss_weight, float* dW, float* db, float* loss) {
  if (!train || !labels) return vv_fail(VV_ERR_ARG, "%s: NULL argument", who);
  GalleryRows gr;
  { const int rc = check_pair(who, c, l, train, &gr); if (rc) return rc; }
  std::vector<int32_t> listed;
  if (by_rows) { const int rc = check_rows(who, rows, count, gr.n_ref, labels, l->C, &listed); if (rc) return rc; }
  else {
    if (first < 0 || count < 1 || first > gr.n_ref - count)
      return vv_fail(VV_ERR_ARG, "%s: rows %lld .. +%lld are outside the gallery's %lld items", who, (long long)first, (long long)count, (long long)gr.n_ref);
    const int rc = check_labels(who, labels, gr.n_ref, l->C); if (rc) return rc;
  }
  const int64_t n_lab = by_rows ? count : gr.n_ref;
  const BatchPlan bp = batch_plan(c, l, count);
  { int rc = ensure_rows(c, l, bp.block_rows); if (!rc) rc = ensure_slabs(c, l, bp.p.S); if (rc) return rc; }
  DevTmp<int32_t> lab, idx;
  DevTmp<LinRec> rec;
  DevTmp<float> g;                                                         // [Cp][Dp] | [Cp]
  const size_t nW = (size_t)l->Cp * l->Dp;
  HIPCHK(lab.alloc((size_t)n_lab)); HIPCHK(rec.alloc(1)); HIPCHK(g.alloc(nW + l->Cp));
  if (by_rows) HIPCHK(idx.alloc((size_t)count));
  HIPCHK(hipMemcpyAsync(lab, by_rows ? listed.data() : labels, (size_t)n_lab * 4, hipMemcpyHostToDevice, c->stream));
  if (by_rows) HIPCHK(hipMemcpyAsync(idx, rows, (size_t)count * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(g, 0, (nW + l->Cp) * 4, c->stream));
  { const int rc = queue_batch(c, l, gr, by_rows ? idx.p : nullptr, lab, first, count, loss_weight, bp, rec, nullptr); if (rc) return rc; }
  LinUpdArgs u = upd_args(l, bp.p.S);                                      // the same reduction, without the rule
  u.rule = 0; u.W = g; u.b = g + nW; u.hW = u.hb = nullptr;
  launch_lin_update(u, c->stream);
  HIPCHK(hipGetLastError());
  LinRec h;
  HIPCHK(hipMemcpyAsync(&h, rec, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (dW) HIPCHK(hipMemcpy2D(dW, (size_t)l->dim * 4, g, (size_t)l->Dp * 4, (size_t)l->dim * 4, (size_t)l->C, hipMemcpyDeviceToHost));
  if (db) HIPCHK(hipMemcpy(db, g + nW, (size_t)l->C * 4, hipMemcpyDeviceToHost));       // (bias == 0: zeros)
  if (loss) *loss = (float)((double)loss_weight * h.loss_sum / (double)count);
  return VV_OK;
}

int vv_linear_grad(vv_ctx* c, vv_linear* l, vv_gallery* train, const int32_t* labels, int64_t first, int64_t count, float loss_weight,
                   float* dW, float* db, float* loss) {
  NEED(c);
  return grad_common("vv_linear_grad", c, l, train, labels, nullptr, false, first, count, loss_weight, dW, db, loss);
}

int vv_linear_grad_rows(vv_ctx* c, vv_linear* l, vv_gallery* train, const int32_t* labels, const int32_t* rows, int64_t n_rows,
                        float loss_weight, float* dW, float* db, float* loss) {
  NEED(c);
  return grad_common("vv_linear_grad_rows", c, l, train, labels, rows, true, 0, n_rows, loss_weight, dW, db, loss);
}

int vv_linear_scores_rows(vv_ctx* c, vv_linear* l, vv_gallery* src, const int32_t* rows, int64_t n_rows, float* out_dev) {
  NEED(c);
  if (!src || !out_dev) return vv_fail(VV_ERR_ARG, "vv_linear_scores_rows: NULL argument");
  GalleryRows gr = {};
  { const int rc = check_pair("vv_linear_scores_rows", c, l, src, &gr); if (rc) return rc; }
  { const int rc = check_rows("vv_linear_scores_rows", rows, n_rows, gr.n_ref, nullptr, l->C, nullptr); if (rc) return rc; }
  const int64_t blk = std::min<int64_t>(n_rows, std::max<int64_t>(1, std::min<int64_t>(65536, (int64_t)(GALLERY_SCRATCH_MAX / ((size_t)2 * l->Cp * 4)))));
  { const int rc = ensure_rows(c, l, blk); if (rc) return rc; }
  DevTmp<int32_t> idx;
  HIPCHK(idx.alloc((size_t)n_rows));
  HIPCHK(hipMemcpyAsync(idx, rows, (size_t)n_rows * 4, hipMemcpyHostToDevice, c->stream));
  for (int64_t q0 = 0; q0 < n_rows; q0 += blk) {                           // (queued in order on one stream: a block's z is read before the next writes it)
    const int64_t cnt = std::min(blk, n_rows - q0);
    launch_sim_f32_rows(gr.feat, idx.p + q0, l->W, l->z, (int)cnt, l->C, l->Dp, l->Cp, c->stream);
    launch_lin_scores_out(l->z, l->Cp, cnt, l->C, l->bias ? l->b : nullptr, out_dev + (size_t)q0 * l->C, c->stream);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));                                 // (the list's device copy lives for this call)
  return VV_OK;
}

int vv_linear_scores(vv_ctx* c, vv_linear* l, vv_gallery* src, const float* q, int64_t n_q, float* out_dev) {
  NEED(c);
  if (!out_dev || (src != nullptr) == (q != nullptr)) return vv_fail(VV_ERR_ARG, "vv_linear_scores: exactly one of the gallery and the host rows must be given, and out_dev");
  GalleryRows gr = {};
  { const int rc = check_pair("vv_linear_scores", c, l, src, &gr); if (rc) return rc; }
  if (n_q < 1 || n_q > (1ll << 30) || (src && n_q != gr.n_ref)) return vv_fail(VV_ERR_ARG, "vv_linear_scores: n_q = %lld", (long long)n_q);
  const int64_t blk = std::min<int64_t>(n_q, std::max<int64_t>(1, std::min<int64_t>(65536, (int64_t)(GALLERY_SCRATCH_MAX / ((size_t)2 * l->Cp * 4)))));
  { const int rc = ensure_rows(c, l, blk); if (rc) return rc; }
  DevTmp<float> qd;
  if (q) { HIPCHK(qd.alloc((size_t)blk * l->Dp)); HIPCHK(hipMemsetAsync(qd, 0, (size_t)blk * l->Dp * 4, c->stream)); }
  for (int64_t q0 = 0; q0 < n_q; q0 += blk) {
    const int64_t rows = std::min(blk, n_q - q0);
    const float* X = src ? gr.feat + q0 * gr.Dp : qd.p;
    if (q) HIPCHK(hipMemcpy2DAsync(qd, (size_t)l->Dp * 4, q + (size_t)q0 * l->dim, (size_t)l->dim * 4, (size_t)l->dim * 4, (size_t)rows, hipMemcpyHostToDevice, c->stream));
    launch_sim_f32(X, l->W, l->z, (int)rows, l->C, l->Dp, l->Cp, c->stream);
    launch_lin_scores_out(l->z, l->Cp, rows, l->C, l->bias ? l->b : nullptr, out_dev + (size_t)q0 * l->C, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));                               // (the next block's upload reuses qd)
  }
  return VV_OK;
}

int vv_op_softmax_loss(vv_ctx* c, const float* z_dev, int64_t rows, int32_t cols, int64_t pitch, const int32_t* labels, float loss_weight,
                       float* prob_dev, float* dz_dev, float* loss, int64_t* correct) {
  NEED(c);
  if (!z_dev || !labels) return vv_fail(VV_ERR_ARG, "vv_op_softmax_loss: NULL argument");
  if (rows < 1 || rows > (1ll << 30) || cols < 1 || cols > LIN_MAX_CLASSES || pitch < cols)
    return vv_fail(VV_ERR_ARG, "vv_op_softmax_loss: %lld rows of %d columns, pitch %lld", (long long)rows, cols, (long long)pitch);
  { const int rc = check_labels("vv_op_softmax_loss", labels, rows, cols); if (rc) return rc; }
  DevTmp<int32_t> lab;
  DevTmp<char> parts;                                                      // the record, then the partials
  HIPCHK(lab.alloc((size_t)rows)); HIPCHK(parts.alloc(64 + kSmPartBytes));
  HIPCHK(hipMemcpyAsync(lab, labels, (size_t)rows * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(parts, 0, 64 + kSmPartBytes, c->stream));
  LinSoftmaxArgs sa;
  sa.sim = z_dev; sa.pitch = pitch; sa.rows = rows; sa.cols = cols; sa.mul = 1.f; sa.bias = nullptr; sa.labels = lab;
  sa.scale = loss_weight / (float)rows; sa.dz = dz_dev; sa.prob = prob_dev; sa.row_loss = nullptr; sa.row_flags = nullptr;
  sa.wd = cols <= 32 ? 32 : 64; sa.rec = (LinRec*)parts.p; sa.first_block = 1;
  sm_parts(parts.p + 64, sa);
  launch_softmax_xent(sa, c->stream);
  HIPCHK(hipGetLastError());
  LinRec h;
  HIPCHK(hipMemcpyAsync(&h, parts, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (loss) *loss = (float)((double)loss_weight * h.loss_sum / (double)rows);
  if (correct) *correct = h.correct;
  return VV_OK;
}

int vv_linear_loss_set(vv_ctx* c, vv_linear* l, int32_t loss, int32_t norm) {
  NEED(c);
  { const int rc = check_pair("vv_linear_loss_set", c, l, nullptr, nullptr); if (rc) return rc; }
  if (loss != VV_LIN_LOSS_SOFTMAX && loss != VV_LIN_LOSS_HINGE) return vv_fail(VV_ERR_ARG, "vv_linear_loss_set: loss = %d is neither VV_LIN_LOSS_SOFTMAX nor VV_LIN_LOSS_HINGE", loss);
  if (loss == VV_LIN_LOSS_HINGE) {
    if (norm != VV_NORM_L1 && norm != VV_NORM_L2) return vv_fail(VV_ERR_ARG, "vv_linear_loss_set: norm = %d is neither VV_NORM_L1 nor VV_NORM_L2", norm);
    l->norm = norm;
  }
  l->loss = loss;
  return VV_OK;
}

int vv_linear_loss_get(vv_ctx* c, vv_linear* l, int32_t* loss, int32_t* norm) {
  NEED(c);
  { const int rc = check_pair("vv_linear_loss_get", c, l, nullptr, nullptr); if (rc) return rc; }
  if (loss) *loss = l->loss;
  if (norm) *norm = l->norm;
  return VV_OK;
}

int vv_op_hinge_loss(vv_ctx* c, const float* z_dev, int64_t rows, int32_t cols, int64_t pitch, const int32_t* labels, int32_t norm,
                     float loss_weight, float* dz_dev, float* loss, int64_t* correct) {
  NEED(c);
  if (!z_dev || !labels) return vv_fail(VV_ERR_ARG, "vv_op_hinge_loss: NULL argument");
  if (rows < 1 || rows > (1ll << 30) || cols < 1 || cols > LIN_MAX_CLASSES || pitch < cols)
    return vv_fail(VV_ERR_ARG, "vv_op_hinge_loss: %lld rows of %d columns, pitch %lld", (long long)rows, cols, (long long)pitch);
  if (norm != VV_NORM_L1 && norm != VV_NORM_L2) return vv_fail(VV_ERR_ARG, "vv_op_hinge_loss: norm = %d is neither VV_NORM_L1 nor VV_NORM_L2", norm);
  { const int rc = check_labels("vv_op_hinge_loss", labels, rows, cols); if (rc) return rc; }
  DevTmp<int32_t> lab;
  DevTmp<char> parts;                                                      // the record, then the partials
  HIPCHK(lab.alloc((size_t)rows)); HIPCHK(parts.alloc(64 + kSmPartBytes));
  HIPCHK(hipMemcpyAsync(lab, labels, (size_t)rows * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(parts, 0, 64 + kSmPartBytes, c->stream));
  LinHingeArgs ha;
  ha.sim = z_dev; ha.pitch = pitch; ha.rows = rows; ha.cols = cols; ha.mul = 1.f; ha.bias = nullptr; ha.labels = lab;
  ha.norm = norm; ha.scale = hinge_scale(norm, loss_weight, rows); ha.dz = dz_dev;
  ha.wd = lin_hinge_lanes(cols); ha.vec = aligned16(z_dev, pitch) && (!dz_dev || aligned16(dz_dev, pitch));
  ha.rec = (LinRec*)parts.p; ha.first_block = 1;
  sm_parts(parts.p + 64, ha);
  launch_hinge(ha, c->stream);
  HIPCHK(hipGetLastError());
  c->last_hinge_form = ha.vec ? 1 : 2;
  LinRec h;
  HIPCHK(hipMemcpyAsync(&h, parts, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->last_hinge_nonfinite = h.nonfinite;
  if (loss) *loss = (float)((double)loss_weight * h.loss_sum / (double)rows);
  if (correct) *correct = h.correct;
  return VV_OK;
}

int vv_op_gemm_tn(vv_ctx* c, const float* A, int64_t lda, const float* B, int64_t ldb, int64_t k, int32_t m, int32_t n, float* out_dev) {
  NEED(c);
  if (!A || !B || !out_dev) return vv_fail(VV_ERR_ARG, "vv_op_gemm_tn: NULL argument");
  if (k < 1 || m < 1 || n < 1 || lda < m || ldb < n || k > (1ll << 40) || (int64_t)m * n > (1ll << 30))
    return vv_fail(VV_ERR_ARG, "vv_op_gemm_tn: k = %lld, m = %d, n = %d, lda = %lld, ldb = %lld", (long long)k, m, n, (long long)lda, (long long)ldb);
  const LinPlan p = lin_plan(k, m, n, c->lin_split_rows);
  const int64_t stride = round_up((int64_t)m * n, 4);
  DevTmp<float> slabs;
  HIPCHK(slabs.alloc((size_t)p.S * stride));
  for (int blk = 0; blk < p.blocks; ++blk) {
    const int64_t r0 = (int64_t)blk * p.block_rows, rows = std::min(p.block_rows, k - r0);
    LinWgradArgs wa;
    wa.A = A + r0 * lda; wa.lda = lda; wa.B = B + r0 * ldb; wa.ldb = ldb; wa.k = rows; wa.m = m; wa.n = n;
    wa.split_rows = p.split_rows; wa.S = (int)((rows + p.split_rows - 1) / p.split_rows);
    wa.slabs = slabs; wa.slab_stride = stride; wa.dbs = nullptr; wa.accumulate = blk > 0;
    wa.vec_a = aligned16(wa.A, lda); wa.vec_b = aligned16(wa.B, ldb);
    launch_lin_wgrad(wa, c->stream);
  }
  LinUpdArgs u;
  u.slabs = slabs; u.slab_stride = stride; u.S = p.S; u.nW = (int64_t)m * n; u.dbs = nullptr; u.db_stride = 0; u.nb = 0;
  u.W = out_dev; u.hW = u.b = u.hb = nullptr; u.lr = u.momentum = u.wd = 0.f; u.rule = 0; u.vec = ((uintptr_t)out_dev & 15) == 0;
  launch_lin_update(u, c->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));                                 // (the slabs live for this call)
  c->last_lin_splits = p.S; c->last_lin_blocks = p.blocks;
  return VV_OK;
}

int vv_rows_shuffled(uint64_t seed, int32_t n, int32_t epochs, int32_t* out) {
  switch (vv::rows_shuffled(seed, n, epochs, out)) {
    case ROWS_OK: return VV_OK;
    case ROWS_BAD_N: return vv_fail(VV_ERR_ARG, "vv_rows_shuffled: n = %d", n);
    case ROWS_BAD_EPOCHS: return vv_fail(VV_ERR_ARG, "vv_rows_shuffled: epochs = %d", epochs);
    default: return vv_fail(VV_ERR_ARG, "vv_rows_shuffled: out is NULL");
  }
}

int vv_rows_fold(uint64_t seed, int32_t n, int32_t folds, int32_t fold, int32_t* train, int64_t* n_train, int32_t* held, int64_t* n_held) {
  std::vector<int32_t> perm((size_t)std::max(n, 1));
  switch (vv::rows_fold(seed, n, folds, fold, perm.data(), train, n_train, held, n_held)) {
    case ROWS_OK: return VV_OK;
    case ROWS_BAD_N: return vv_fail(VV_ERR_ARG, "vv_rows_fold: n = %d", n);
    case ROWS_BAD_FOLDS: return vv_fail(VV_ERR_ARG, "vv_rows_fold: folds = %d is outside 2 .. n = %d", folds, n);
    case ROWS_BAD_FOLD: return vv_fail(VV_ERR_ARG, "vv_rows_fold: fold = %d is outside 0 .. %d", fold, folds - 1);
    default: return vv_fail(VV_ERR_ARG, "vv_rows_fold: NULL argument");
  }
}

}  // extern "C"
