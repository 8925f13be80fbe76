// classify.hip -- entry point of the classification statistics (include/videovec.h: vv_classification_stats).  The kernels are in
// kernels_classify.hip.  Everything is queued on the context's stream; of the context the call reads and writes the cls_* / last_cls_*
// options.  None of this reads or writes the training step's state.
#include <algorithm>
#include <vector>

#include "vv_ctx.h"

using namespace vv;

extern "C" {

// ------------------------------------------------------------------------------- classification statistics ------
// ClassificationStatsLayer::Forward_cpu (classification_stats_layer.cpp:36-95).  The host validates the labels and builds the
// per-class lists of positives in ascending item index (as gallery_init builds its id lists); everything that touches a score
// runs in kernels_classify.hip, one column block at a time; the host divides the integer counts (:71, :93).
namespace {
struct EvTmp {                                            // events that live for one API call
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  ~EvTmp() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
}  // namespace

int vv_classification_stats(vv_ctx* c, const float* scores, int64_t n, int32_t num_classes, const int32_t* labels,
                            int scores_on_device, float* accuracy, float* ap, int32_t* count, vv_classification_report* out) {
  if (!c || !scores || !labels || !out) return fail(VV_ERR_ARG, "vv_classification_stats: NULL argument");
  if (n < 1 || n > (1ll << 24) || num_classes < 1)
    return fail(VV_ERR_ARG, "vv_classification_stats: %lld rows of %d classes (1 <= n <= 2^24, num_classes >= 1)", (long long)n, num_classes);
  const int C = num_classes, N = (int)n;
  std::vector<int32_t> hcount((size_t)C, 0), hstart((size_t)C + 1, 0);
  for (int i = 0; i < N; ++i) {
    if (labels[i] < 0 || labels[i] >= C)
      return fail(VV_ERR_ARG, "vv_classification_stats: label %d of row %d is outside 0 .. %d", labels[i], i, C - 1);
    ++hcount[labels[i]];                                                                   // :53
  }
  VV_ENTER(c);
  c->last_cls_passes = c->last_cls_segments = c->last_cls_blocks = 0; c->last_cls_row_ms = c->last_cls_count_ms = 0;
  const int64_t np = round_up(n, 64);
  for (int k = 0; k < C; ++k) hstart[k + 1] = hstart[k] + hcount[k];
  std::vector<int32_t> hpos((size_t)N), fill(hstart.begin(), hstart.end() - 1), hlab((size_t)np, -1);
  for (int i = 0; i < N; ++i) { hpos[fill[labels[i]]++] = i; hlab[i] = labels[i]; }
  // the counting pass's tiles, class by class: {first position in hpos, positives, class, 0}; tbegin[k]: the first tile of class k
  std::vector<int4> htiles; std::vector<int32_t> tbegin((size_t)C + 1, 0);
  for (int k = 0; k < C; ++k) {
    tbegin[k] = (int32_t)htiles.size();
    for (int o = 0; o < hcount[k]; o += CLS_TILE) htiles.push_back(make_int4(hstart[k] + o, std::min(CLS_TILE, hcount[k] - o), k, 0));
  }
  tbegin[C] = (int32_t)htiles.size();
  // device buffers of the call, all of them within the gallery path's scratch limit
  const bool host = !scores_on_device;
  const size_t fixed = (size_t)np * 4 + (size_t)N * (4 + 12 + 4 + 4) + ((size_t)C + 1) * 4 + (size_t)C * (4 + 8 + 4) + 8 + htiles.size() * 16 + 4096;
  const size_t per_col = (size_t)np * 4 + (host ? (size_t)N * 4 : 0);
  if (fixed + per_col > GALLERY_SCRATCH_MAX)
    return fail(VV_ERR_ARG, "vv_classification_stats: %lld rows of %d classes do not fit one column into the scratch limit", (long long)n, C);
  int cb_max = (int)std::min<size_t>((size_t)C, (GALLERY_SCRATCH_MAX - fixed) / per_col);
  if (c->cls_block_cols > 0) cb_max = std::min(cb_max, c->cls_block_cols);
  DevTmp<int32_t> dlab, dpos, dstart, rarg; DevTmp<uint32_t> cnt, correct; DevTmp<float> rmax, col, upl, dap; DevTmp<double> dapd;
  DevTmp<unsigned long long> dnan; DevTmp<int4> dtiles;
  HIPCHK(dlab.alloc((size_t)np)); HIPCHK(dpos.alloc((size_t)N)); HIPCHK(dstart.alloc((size_t)C + 1)); HIPCHK(rarg.alloc((size_t)N));
  HIPCHK(cnt.alloc((size_t)N * 3)); HIPCHK(correct.alloc((size_t)C)); HIPCHK(rmax.alloc((size_t)N));
  HIPCHK(col.alloc((size_t)cb_max * np)); HIPCHK(dap.alloc((size_t)C)); HIPCHK(dapd.alloc((size_t)C)); HIPCHK(dnan.alloc(1));
  HIPCHK(dtiles.alloc(htiles.size() + 1));
  if (host) HIPCHK(upl.alloc((size_t)cb_max * N));
  EvTmp ev;
  for (int i = 0; i < 3; ++i) HIPCHK(hipEventCreate(&ev.e[i]));
  hipStream_t s = c->stream;
  HIPCHK(hipMemcpyAsync(dlab, hlab.data(), (size_t)np * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dpos, hpos.data(), (size_t)N * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dstart, hstart.data(), ((size_t)C + 1) * 4, hipMemcpyHostToDevice, s));
  if (!htiles.empty()) HIPCHK(hipMemcpyAsync(dtiles, htiles.data(), htiles.size() * 16, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(cnt, 0, (size_t)N * 12, s));
  HIPCHK(hipMemsetAsync(correct, 0, (size_t)C * 4, s));
  HIPCHK(hipMemsetAsync(dnan, 0, 8, s));
  // counting segments: as the gallery's row kernels, at most GALLERY_SEG_MAX per column
  const int seg = std::max(4 * CLS_STAGE, (int)round_up((n + GALLERY_SEG_MAX - 1) / GALLERY_SEG_MAX, CLS_STAGE));
  const int S = (int)((n + seg - 1) / seg);
  c->last_cls_segments = S;
  for (int c0 = 0; c0 < C; c0 += cb_max) {
    const int cb = std::min(cb_max, C - c0);
    const float* src = scores + c0; int64_t pitch = C;
    if (host) {                                                  // the block's columns, uploaded as a [n][cb] matrix
      if (cb == C) HIPCHK(hipMemcpyAsync(upl, scores, (size_t)N * C * 4, hipMemcpyHostToDevice, s));
      else HIPCHK(hipMemcpy2DAsync(upl, (size_t)cb * 4, scores + c0, (size_t)C * 4, (size_t)cb * 4, (size_t)N, hipMemcpyHostToDevice, s));
      src = upl; pitch = cb;
    }
    HIPCHK(hipEventRecord(ev.e[0], s));
    launch_cls_rows(src, pitch, N, c0, cb, c0 + cb == C ? 1 : 0, dlab, rmax, rarg, correct, dnan, s);       // :49-67
    launch_cls_pack(src, pitch, N, cb, col, np, s);
    HIPCHK(hipEventRecord(ev.e[1], s));
    int passes = 0;
    for (int t0 = tbegin[c0]; t0 < tbegin[c0 + cb]; t0 += c->cls_pass_tiles, ++passes)
      launch_cls_count(col, np, N, seg, S, c0, dlab, dpos, dtiles, t0, std::min(c->cls_pass_tiles, tbegin[c0 + cb] - t0), cnt, s);
    launch_cls_final(col, np, c0, cb, dpos, dstart, cnt, dapd, dap, s);                                     // :76-85
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[2], s));
    HIPCHK(hipEventSynchronize(ev.e[2]));                        // (the next block's upload reuses upl)
    float ms_rows = 0, ms_count = 0;
    HIPCHK(hipEventElapsedTime(&ms_rows, ev.e[0], ev.e[1])); HIPCHK(hipEventElapsedTime(&ms_count, ev.e[1], ev.e[2]));
    c->last_cls_row_ms += ms_rows; c->last_cls_count_ms += ms_count;
    c->last_cls_passes = std::max(c->last_cls_passes, passes); c->last_cls_blocks += 1;
  }
  std::vector<uint32_t> hcorrect((size_t)C); std::vector<float> hap((size_t)C); std::vector<double> hapd((size_t)C);
  unsigned long long nans = 0;
  HIPCHK(hipMemcpyAsync(hcorrect.data(), correct, (size_t)C * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(hap.data(), dap, (size_t)C * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(hapd.data(), dapd, (size_t)C * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&nans, dnan, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (nans) return fail(VV_ERR_ARG, "vv_classification_stats: %llu NaN scores (the reference's sort is undefined on them)", nans);
  int64_t total = 0; int present = 0; double sum_ap = 0;
  for (int k = 0; k < C; ++k) {
    total += hcorrect[k];
    if (hcount[k] > 0) { present += 1; sum_ap += hapd[k]; }
    if (accuracy) accuracy[k] = hcount[k] > 0 ? (float)hcorrect[k] / (float)hcount[k] : 0.f;              // :71, :88
    if (ap) ap[k] = hap[k];                                                                              // :85, :89
    if (count) count[k] = hcount[k];
  }
  out->total_accuracy = (float)total / (float)n;                                                        // :93
  out->mean_ap = (float)(sum_ap / present);
  out->classes_present = present; out->reserved_ = 0; out->n = n;
  return VV_OK;
}

}  // extern "C"
