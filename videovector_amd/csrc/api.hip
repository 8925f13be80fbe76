// api.hip -- implementation of the C ABI in include/videovec.h (gfx950 / HIP only; there is no CPU fallback: every entry point fails with
// VV_ERR_NOGPU / VV_ERR_HIP when no device is usable): the context's life cycle, the options, the table, the parameters, the read-back
// accessors, the embeddings, the vv_comm_* wrappers and profiling.  The pass over a batch is pass.hip, the solver's half solver.hip.
#include "../../include/videovec.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <algorithm>
#include <limits>
#include <map>
#include <unordered_map>
#include <string>
#include <thread>
#include <vector>

#include "vv_ctx.h"

namespace vv { bool ablate_on(); thread_local const KernelOpts* g_ko = nullptr; }
using namespace vv;

thread_local char vv_g_err[512] = "";
int vv_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(vv_g_err, sizeof(vv_g_err), fmt, ap);
  va_end(ap);
  return code;
}

namespace vv { thread_local ProfPair g_prof; }

// Arms a pair of events for the launcher called next: its (first / last) kernel is dispatched with
// hipExtLaunchKernelGGL, which stamps them from the dispatch packet itself (vv_internal.h: VV_LAUNCH).
void vv_prof_begin(vv_ctx* c, const char* name, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (!c->prof || (c->prof_calls % (uint64_t)c->prof_every) != (uint64_t)c->prof_every - 1) return;   // the N-th, 2N-th, ... step
  if (!c->prof_only.empty() && c->prof_only.find(std::string(",") + name + ",") == std::string::npos) return;
  auto& pe = c->prof_map[name];
  if (pe.ev.size() >= 8192) return;
  while (c->ev_pool.size() < c->ev_used + 2) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    c->ev_pool.push_back(e);
  }
  *e0 = c->ev_pool[c->ev_used++]; *e1 = c->ev_pool[c->ev_used++];
  vv::g_prof.start = *e0; vv::g_prof.stop = *e1;
}
void vv_prof_end(vv_ctx* c, const char* name, hipEvent_t e0, hipEvent_t e1) {
  if (!e0) return;
  // a launcher that did not take the events (a kernel variant launched the plain way): fall back to stream records
  if (vv::g_prof.start) { (void)hipEventRecord(e0, c->stream); vv::g_prof.start = nullptr; }
  if (vv::g_prof.stop) { (void)hipEventRecord(e1, c->stream); vv::g_prof.stop = nullptr; }
  c->prof_map[name].ev.emplace_back(e0, e1);
}

extern "C" {

const char* vv_last_error(void) { return vv_g_err; }
const char* vv_version(void) { return "videovec-mi355x 0.1 (gfx950)"; }

void vv_step_cfg_default(vv_step_cfg* cfg) {
  memset(cfg, 0, sizeof(*cfg));
  cfg->margin = 2.0f; cfg->norm = VV_NORM_L2; cfg->loss_weight = 1.0f;
  cfg->momentum = 0.9f; cfg->weight_decay = 5e-4f; cfg->lr = 1e-3f;
  cfg->lr_mult[0] = 1.f; cfg->lr_mult[1] = 2.f;
  cfg->decay_mult[0] = 1.f; cfg->decay_mult[1] = 0.f;
  cfg->reg = VV_REG_L2;
  cfg->solver_type = VV_SOLVER_SGD; cfg->delta = 1e-8f; cfg->ip_regularization = 0.f;
}

static int create_init(vv_ctx* c);

int vv_create(int device, int prec, vv_ctx** out) {
  if (!out) return fail(VV_ERR_ARG, "vv_create: out is NULL");
  if (prec != VV_PREC_F16 && prec != VV_PREC_BF16) return fail(VV_ERR_ARG, "vv_create: bad prec %d", prec);
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(VV_ERR_NOGPU, "vv_create: no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= n) return fail(VV_ERR_ARG, "vv_create: device %d out of range (%d)", device, n);
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(VV_ERR_NOGPU, "vv_create: device %d is %s; this build targets gfx950 only", device,
                prop.gcnArchName);
  vv_ctx* c = new vv_ctx();
  c->device = device; c->prec = prec;
  const int rc = create_init(c);
  if (rc != VV_OK) { vv_destroy(c); return rc; }        // the message of the failing call stays in vv_last_error()
  *out = c;
  return VV_OK;
}

// everything vv_create allocates; a failure half way leaves a context vv_destroy can release
static int create_init(vv_ctx* c) {
  HIPCHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  c->stream = c->own_stream;

  HIPCHK(hipMalloc(&c->scales, sizeof(Scales)));
  Scales h = {1.f, 1.f, 1.f, 0u};
  HIPCHK(hipMemcpy(c->scales, &h, sizeof(h), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&c->wmax_blocks, 2 * WMAX_SLOTS * sizeof(float)));
  HIPCHK(hipMemset(c->wmax_blocks, 0, 2 * WMAX_SLOTS * sizeof(float)));
  HIPCHK(hipMalloc(&c->loss2, 2 * sizeof(float)));
  HIPCHK(hipMemset(c->loss2, 0, 2 * sizeof(float)));
  // product options: initial values from the environment, per context (vv_set_option changes them afterwards)
  if (const char* v = opt_env("VV_WGRAD_TR")) c->ko.wgrad_tr = atoi(v) != 0;
  if (const char* v = opt_env("VV_FWD_LEAD")) c->ko.fwd_lead = atoi(v);
  if (const char* v = opt_env("VV_SCORE_PF")) c->ko.score_pf = atoi(v);
  if (const char* v = opt_env("VV_WGRAD_LEAN")) c->ko.wgrad_lean = atoi(v);
  if (const char* v = opt_env("VV_SEG_BWD")) c->seg_bwd = atoi(v) != 0;
  if (const char* v = opt_env("VV_H16")) c->h16 = atoi(v) != 0;
  if (const char* v = opt_env("VV_SLAB16")) c->slab16 = atoi(v) != 0;
  if (const char* v = opt_env("VV_V16")) c->v16 = atoi(v) != 0;
  if (const char* v = opt_env("VV_DEDUP")) c->dedup = atoi(v) != 0;
  if (const char* v = opt_env("VV_FUSE_UPDATE")) c->fuse_update = atoi(v) != 0;
  if (const char* v = opt_env("VV_DROP_DEDUP")) {                 // 0, 1 or 2; anything else leaves the default
    char* end = nullptr;
    const double dv = strtod(v, &end);
    if (end != v && *end == 0 && (dv == 0.0 || dv == 1.0 || dv == 2.0)) c->drop_dedup = (int)dv;
  }
  if (const char* v = opt_env("VV_H16_GUARD")) {
    char* end = nullptr;
    const double dv = strtod(v, &end);
    if (end != v && *end == 0 && (dv == 0.0 || dv == 1.0 || dv == 2.0)) c->h16_guard = (int)dv;
  }
  if (const char* v = opt_env("VV_COMM_GATE")) c->comm_gate = atoi(v) != 0;
  if (const char* v = opt_env("VV_COMM_INLINE")) c->comm_inline = atoi(v) != 0;
  if (const char* v = opt_env("VV_COMM_TEST_DELAY_US")) c->comm_test_delay_us = atoi(v);
  if (const char* v = opt_env("VV_NEAREST_SELECT_MIN_K")) c->nearest_select_min_k = std::max(1, std::min(RT_MAX_K + 1, atoi(v)));
  // lab switches (-DVV_LAB builds only; several of them produce WRONG results by design)
  if (const char* v = lab_env("VV_ABLATE")) c->ko.ablate = atoi(v);
  if (const char* v = lab_env("VV_LAB_FWD_ABL")) c->ko.lab_fwd_abl = atoi(v);
  if (const char* v = lab_env("VV_LAB_WG_ABL")) c->ko.lab_wg_abl = atoi(v);
  if (const char* v = lab_env("VV_PH_MQ")) c->ko.ph_mq = atoi(v);
  if (const char* v = lab_env("VV_SCORE_REG")) c->ko.score_reg = atoi(v);
  if (const char* v = lab_env("VV_SCORE_RR")) c->ko.score_rr = atoi(v);
  if (const char* v = lab_env("VV_GUARD_PROACTIVE")) c->guard_proactive = atoi(v) != 0;
  if (const char* v = lab_env("VV_FUSE_KEEP_GRADS")) c->fuse_keep_grads = atoi(v) != 0;
  if (const char* v = lab_env("VV_COMM_SKIP_AR1")) c->comm_skip_ar1 = atoi(v) != 0;
  if (const char* v = lab_env("VV_DEDUP_GATE")) c->dd_gate_word = atoi(v) != 0;
  if (const char* v = lab_env("VV_DEDUP_LDS_KB")) c->dd_lds_kb = atoi(v);
  if (const char* v = lab_env("VV_TRACE_HOST")) c->trace_host_ms = atof(v);
  c->trace_waits = lab_env("VV_TRACE_WAITS") != nullptr;
  vv::g_ko = &c->ko;
  HIPCHK(hipMalloc(&c->dd_info_all, vv_ctx::kDdAll * 4 * sizeof(int32_t)));
  HIPCHK(hipMemset(c->dd_info_all, 0, vv_ctx::kDdAll * 4 * sizeof(int32_t)));
  HIPCHK(hipStreamCreateWithFlags(&c->dd_stream, hipStreamNonBlocking));
  { int ncu = 0; if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && ncu > 0) c->n_cu = ncu; }
  for (int i = 0; i < vv_ctx::kDdAll; ++i) {
    c->dd_set[i].info = c->dd_info_all + 4 * i;
    HIPCHK(hipEventCreateWithFlags(&c->dd_set[i].done, hipEventDisableTiming));
  }
  c->dd_info = c->dd_set[0].info;
  if (const char* v = lab_env("VV_DEDUP_ASYNC")) c->dd_async = atoi(v) != 0;
  if (const char* v = lab_env("VV_DEDUP_SPIN_US")) c->dd_spin_us = atof(v);
  HIPCHK(hipHostMalloc((void**)&c->U_host, 3 * sizeof(int32_t), hipHostMallocMapped));   // {U, saturated f16 gradient sums, U of the last forward-only pass}
  c->U_host[0] = c->U_host[1] = c->U_host[2] = 0;
  HIPCHK(hipHostGetDevicePointer((void**)&c->U_host_dev, c->U_host, 0));
  // the forward-only pass (vv_forward): its record and the event that marks the end of the pass that last read its grouping set
  HIPCHK(hipMalloc((void**)&c->eval_rec, sizeof(EvalRec)));
  HIPCHK(hipMemset(c->eval_rec, 0, sizeof(EvalRec)));
  HIPCHK(hipEventCreateWithFlags(&c->ev_eval, hipEventDisableTiming));
  HIPCHK(hipMalloc(&c->w_gate, (W_CHUNKS_MAX + 1) * W_GATE_STRIDE * sizeof(int32_t)));
  HIPCHK(hipMemset(c->w_gate, 0, (W_CHUNKS_MAX + 1) * W_GATE_STRIDE * sizeof(int32_t)));
  c->pub_count = c->w_gate + W_CHUNKS_MAX * W_GATE_STRIDE;      // the arrival counter of the publishing kernels: a line of its own
  if (const char* v = opt_env("VV_WGRAD_UPDATE")) c->wgrad_update = atoi(v) != 0;
  { const char* nc = opt_env("VV_COMM_CHUNKS"); if (nc) c->n_chunks = std::max(1, std::min(W_CHUNKS_MAX, atoi(nc))); }
  HIPCHK(hipEventCreateWithFlags(&c->ev_chunk0, hipEventDisableTiming));
  HIPCHK(hipHostMalloc((void**)&c->gate_err, sizeof(int32_t), hipHostMallocMapped));
  *c->gate_err = 0;
  HIPCHK(hipHostGetDevicePointer((void**)&c->gate_err_dev, c->gate_err, 0));
  HIPCHK(hipMalloc(&c->gg_bound, GG_BOUND_SLOTS * GG_BOUND_STRIDE * sizeof(unsigned long long)));
  HIPCHK(hipMemset(c->gg_bound, 0, GG_BOUND_SLOTS * GG_BOUND_STRIDE * sizeof(unsigned long long)));
  HIPCHK(hipMalloc(&c->gg, sizeof(GradGuard)));
  { GradGuard g0; memset(&g0, 0, sizeof(g0)); g0.mul = 1.f; HIPCHK(hipMemcpy(c->gg, &g0, sizeof(g0), hipMemcpyHostToDevice)); }
  HIPCHK(hipHostMalloc((void**)&c->gmax_host, GMAX_ENTRIES * GMAX_ENTRY_WORDS * sizeof(unsigned long long), hipHostMallocMapped));
  memset(c->gmax_host, 0, GMAX_ENTRIES * GMAX_ENTRY_WORDS * sizeof(unsigned long long));
  for (int i = 0; i < GMAX_ENTRIES; ++i) c->h16_counted[i] = INT32_MIN;
  HIPCHK(hipHostGetDevicePointer((void**)&c->gmax_host_dev, c->gmax_host, 0));
  HIPCHK(hipHostMalloc((void**)&c->seq_host, 2 * sizeof(int32_t), hipHostMallocMapped));
  c->seq_host[0] = c->seq_host[1] = 0;
  HIPCHK(hipHostGetDevicePointer((void**)&c->seq_host_dev, c->seq_host, 0));
  return VV_OK;
}

int vv_device_query(int device, char* buf, size_t n) {
  if (!buf || n == 0) return fail(VV_ERR_ARG, "vv_device_query: no buffer");
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return fail(VV_ERR_NOGPU, "vv_device_query: no HIP device visible");
  if (device < 0 || device >= cnt) return fail(VV_ERR_ARG, "vv_device_query: device %d out of range (%d)", device, cnt);
  hipDeviceProp_t p;
  HIPCHK(hipGetDeviceProperties(&p, device));
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipSetDevice(device));
  (void)hipMemGetInfo(&free_b, &total_b);
  snprintf(buf, n,
           "Device id:                     %d\nName:                          %s\nArchitecture:                  %s\n"
           "Compute units:                 %d\nClock rate:                    %d kHz\nMemory clock rate:             %d kHz\n"
           "Total global memory:           %zu\nFree global memory:            %zu\nShared memory (LDS) per block: %zu\n"
           "Registers per block:           %d\nWavefront size:                %d\nMax threads per block:         %d\n"
           "L2 cache size:                 %d\nConcurrent kernels:            %s\n",
           device, p.name, p.gcnArchName, p.multiProcessorCount, p.clockRate, p.memoryClockRate, (size_t)p.totalGlobalMem, free_b,
           (size_t)p.sharedMemPerBlock, p.regsPerBlock, p.warpSize, p.maxThreadsPerBlock, p.l2CacheSize, p.concurrentKernels ? "Yes" : "No");
  return VV_OK;
}

int vv_destroy(vv_ctx* c) {
  if (!c) return VV_OK;
  (void)hipSetDevice(c->device);
  if (vv::g_ko == &c->ko) vv::g_ko = nullptr;        // (this thread's launcher options pointed into the context)
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm) { vv::comm_destroy(c->comm); c->comm = nullptr; }    // drains the communication stream: before any buffer it uses goes
  vv_ops_release(c);
  vv_free_batch(c);
  dfree(c->table); dfree(c->patch_desc); dfree(c->W); dfree(c->b); dfree(c->hW); dfree(c->hb); dfree(c->hW2); dfree(c->hb2); dfree(c->Wh);
  dfree(c->clip_rec); dfree(c->bank_rec); dfree(c->stat_rec); dfree(c->upd_shadow); dfree(c->eW);
  dfree(c->scales); dfree(c->wmax_blocks); dfree(c->grads_own); dfree(c->mask); dfree(c->loss2);
  dfree(c->dd_key); dfree(c->dd_info_all); dfree(c->gg); dfree(c->gg_bound); dfree(c->w_gate);
  if (c->gate_err) (void)hipHostFree(c->gate_err);
  if (c->gmax_host) (void)hipHostFree(c->gmax_host);
  for (int i = 0; i < vv_ctx::kDdAll; ++i) {
    if (c->dd_set[i].done) (void)hipEventDestroy(c->dd_set[i].done);
  }
  dfree(c->eval_rec);
  if (c->ev_eval) (void)hipEventDestroy(c->ev_eval);
  for (int i = 0; i < vv_ctx::kEvalStage; ++i) {
    if (c->eval_stage_host[i]) (void)hipHostFree(c->eval_stage_host[i]);
    if (c->eval_stage_done[i]) (void)hipEventDestroy(c->eval_stage_done[i]);
  }
  if (c->dd_stream) (void)hipStreamDestroy(c->dd_stream);
  if (c->ev_chunk) (void)hipEventDestroy(c->ev_chunk);
  if (c->ev_idx) (void)hipEventDestroy(c->ev_idx);
  if (c->ev_chunk0) (void)hipEventDestroy(c->ev_chunk0);
  if (c->U_host) (void)hipHostFree(c->U_host);
  for (int i = 0; i < vv_ctx::kStage; ++i)
    if (c->stage_host[i]) (void)hipHostFree(c->stage_host[i]);
  if (c->seq_host) (void)hipHostFree(c->seq_host);
  for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);

  delete c;
  return VV_OK;
}

// ---- the per-context switches by name (include/videovec.h: vv_set_option / vv_get_option).  ONE row per name: its kind, how it is read,
// and for a settable one how a value is checked and written (value: as given; iv: (int)value).
// ReadOnly: what the launchers last chose, what the guards found.  Retired: the alternatives were retired -- reads as the value the library
// always runs with, 0, and accepts only it.  Lab: settable in a library built with -DVV_LAB, otherwise an unknown name; never read.
enum class OptKind { Settable, ReadOnly, Retired, Lab };
struct Option {
  const char* name; OptKind kind;
  int (*get)(vv_ctx* c, double* v);
  int (*set)(vv_ctx* c, double value, int iv);
};
// the guard's state as the last vv_forward_backward's kernels left it (GradGuard: on the device); bf16 / no step yet: 0
static int last_grad(vv_ctx* c, int which, double* v) {
  *v = 0;
  if (!c->gg_last_seq || !c->gg) return VV_OK;
  VV_ENTER(c);
  { const int rcj = vv_comm_join(c); if (rcj) return rcj; }
  HIPCHK(hipStreamSynchronize(c->stream));
  GradGuard gh;
  HIPCHK(hipMemcpy(&gh, c->gg, sizeof(gh), hipMemcpyDeviceToHost));
  if (which == 0) *v = gh.shift[3];
  else if (which == 1) *v = c->gg_last_rounds > 0 ? gh.shift[1] : 0;      // (the proactive form has no round 1)
  else *v = gh.repeat_seq == c->gg_last_seq ? 1 : 0;
  return VV_OK;
}
#define RD(expr) [](vv_ctx* c, double* v) -> int { *v = (double)(expr); return VV_OK; }
#define WR(stmt) [](vv_ctx* c, double value, int iv) -> int { stmt; return VV_OK; }
#define FLAG(name, member) {name, OptKind::Settable, RD(c->member), WR(c->member = iv != 0)}
#define INT(name, member) {name, OptKind::Settable, RD(c->member), WR(c->member = iv)}
#define LAST(name, expr) {name, OptKind::ReadOnly, RD(expr), nullptr}
static const Option kOptions[] = {
  {"fwd_merge", OptKind::Retired, RD(0), nullptr}, {"score_stream", OptKind::Retired, RD(0), nullptr}, {"comm_first_inline", OptKind::Retired, RD(0), nullptr},
  {"dedup", OptKind::Settable, RD(c->dedup), [](vv_ctx* c, double, int iv) -> int { return vv_set_dedup(c, iv); }},
  FLAG("seg_bwd", seg_bwd),
  {"drop_dedup", OptKind::Settable, RD(c->drop_dedup), [](vv_ctx* c, double value, int iv) -> int {
     if (!(value == 0.0 || value == 1.0 || value == 2.0)) return fail(VV_ERR_ARG, "vv_set_option: drop_dedup = %g is none of 0 (dense), 1 (the register-resident shapes), 2 (every segment-path shape)", value);
     c->drop_dedup = iv; return VV_OK; }},
  // setting it on re-arms the guard: a fallback (h16_guard 2) ends, and no report of a step issued before this call starts another
  {"h16", OptKind::Settable, RD(c->h16), WR(c->h16 = iv != 0; if (c->h16) { c->h16_fallback = false; c->h16_arm_seq = c->step_seq; })},
  {"h16_guard", OptKind::Settable, RD(c->h16_guard), [](vv_ctx* c, double value, int iv) -> int {
     if (!(value == 0.0 || value == 1.0 || value == 2.0)) return fail(VV_ERR_ARG, "vv_set_option: h16_guard = %g is none of 0 (off), 1 (count and report), 2 (count, report and fall back to fp32 rows)", value);
     c->h16_guard = iv; return VV_OK; }},
  LAST("last_h16", c->last_h16), LAST("h16_fallback", c->h16_fallback), LAST("h16_flagged_step", c->h16_flag_step),
  LAST("h16_flagged_saturated", c->h16_flag_sat), LAST("h16_flagged_faint_rows", c->h16_flag_faint),
  FLAG("slab16", slab16), FLAG("v16", v16), FLAG("fuse_update", fuse_update),
  INT("fwd_lead", ko.fwd_lead), FLAG("wgrad_tr", ko.wgrad_tr), INT("score_pf", ko.score_pf), INT("wgrad_lean", ko.wgrad_lean),
  FLAG("comm_gate", comm_gate), FLAG("comm_inline", comm_inline), FLAG("wgrad_update", wgrad_update),
  {"comm_chunks", OptKind::Settable, RD(c->n_chunks), WR(c->n_chunks = std::max(1, std::min(W_CHUNKS_MAX, iv)))},
  INT("comm_test_delay_us", comm_test_delay_us),
  {"nearest_select_min_k", OptKind::Settable, RD(c->nearest_select_min_k), [](vv_ctx* c, double, int iv) -> int {
     if (iv < 1 || iv > RT_MAX_K + 1) return fail(VV_ERR_ARG, "vv_set_option: nearest_select_min_k = %d is outside 1 .. %d", iv, RT_MAX_K + 1);
     c->nearest_select_min_k = iv; return VV_OK; }},
  {"cls_pass_tiles", OptKind::Settable, RD(c->cls_pass_tiles), [](vv_ctx* c, double, int iv) -> int {
     if (iv < 1 || iv > 65535) return fail(VV_ERR_ARG, "vv_set_option: cls_pass_tiles = %d is outside 1 .. 65535", iv);
     c->cls_pass_tiles = iv; return VV_OK; }},
  {"cls_block_cols", OptKind::Settable, RD(c->cls_block_cols), [](vv_ctx* c, double, int iv) -> int {
     if (iv < 0) return fail(VV_ERR_ARG, "vv_set_option: cls_block_cols = %d is negative", iv);
     c->cls_block_cols = iv; return VV_OK; }},
  LAST("last_cls_passes", c->last_cls_passes), LAST("last_cls_segments", c->last_cls_segments), LAST("last_cls_blocks", c->last_cls_blocks),
  LAST("last_cls_row_ms", c->last_cls_row_ms), LAST("last_cls_count_ms", c->last_cls_count_ms),
  {"lin_split_rows", OptKind::Settable, RD(c->lin_split_rows), [](vv_ctx* c, double, int iv) -> int {
     if (iv < 0) return fail(VV_ERR_ARG, "vv_set_option: lin_split_rows = %d is negative", iv);
     c->lin_split_rows = iv; return VV_OK; }},
  LAST("last_lin_splits", c->last_lin_splits), LAST("last_lin_blocks", c->last_lin_blocks), LAST("last_lin_gather", c->last_lin_gather),
  LAST("last_lin_fwd_ms", c->last_lin_ms[0]), LAST("last_lin_softmax_ms", c->last_lin_ms[1]), LAST("last_lin_wgrad_ms", c->last_lin_ms[2]),
  LAST("last_lin_update_ms", c->last_lin_ms[3]),
  LAST("last_hinge_form", c->last_hinge_form), LAST("last_hinge_nonfinite", c->last_hinge_nonfinite), LAST("last_knn_form", c->last_knn_form),
  {"km_block_rows", OptKind::Settable, RD(c->km_block_rows), [](vv_ctx* c, double, int iv) -> int {
     if (iv < 0) return fail(VV_ERR_ARG, "vv_set_option: km_block_rows = %d is negative", iv);
     c->km_block_rows = iv; return VV_OK; }},
  LAST("last_km_blocks", c->last_km_blocks), LAST("last_km_chunks", c->last_km_chunks), LAST("last_km_assign_form", c->last_km_assign_form),
  LAST("last_km_sim_ms", c->last_km_ms[0]), LAST("last_km_assign_ms", c->last_km_ms[1]), LAST("last_km_group_ms", c->last_km_ms[2]),
  LAST("last_km_update_ms", c->last_km_ms[3]),
  {"ivf_block_rows", OptKind::Settable, RD(c->ivf_block_rows), [](vv_ctx* c, double, int iv) -> int {
     if (iv < 0) return fail(VV_ERR_ARG, "vv_set_option: ivf_block_rows = %d is negative", iv);
     c->ivf_block_rows = iv; return VV_OK; }},
  {"ivf_grid_wgs", OptKind::Settable, RD(c->ivf_grid_wgs), [](vv_ctx* c, double, int iv) -> int {
     if (iv < 0 || iv > IVF_GRID_MAX) return fail(VV_ERR_ARG, "vv_set_option: ivf_grid_wgs = %d is outside 0 .. %d", iv, IVF_GRID_MAX);
     c->ivf_grid_wgs = iv; return VV_OK; }},
  LAST("last_fwd_tile_rows", c->ko.last_fwd_tile_rows), LAST("last_wgrad_splits", c->ko.last_wgrad_splits),
  LAST("last_update_form", c->ko.last_update_form), LAST("last_score_form", c->ko.last_score_form),
  {"last_grad_shift", OptKind::ReadOnly, [](vv_ctx* c, double* v) -> int { return last_grad(c, 0, v); }, nullptr},
  {"last_grad_shift_round1", OptKind::ReadOnly, [](vv_ctx* c, double* v) -> int { return last_grad(c, 1, v); }, nullptr},
  {"last_grad_repeat", OptKind::ReadOnly, [](vv_ctx* c, double* v) -> int { return last_grad(c, 2, v); }, nullptr},
  {"ablate", OptKind::Lab, nullptr, WR(c->ko.ablate = iv)}, {"lab_fwd_abl", OptKind::Lab, nullptr, WR(c->ko.lab_fwd_abl = iv)},
  {"lab_wg_abl", OptKind::Lab, nullptr, WR(c->ko.lab_wg_abl = iv)}, {"ph_mq", OptKind::Lab, nullptr, WR(c->ko.ph_mq = iv)},
};
#undef RD
#undef WR
#undef FLAG
#undef INT
#undef LAST
static const Option* find_option(const char* name) {
  for (const Option& o : kOptions) {
#ifndef VV_LAB
    if (o.kind == OptKind::Lab) continue;
#endif
    if (!strcmp(o.name, name)) return &o;
  }
  return nullptr;
}

int vv_set_option(vv_ctx* c, const char* name, double value) {
  if (!c || !name) return fail(VV_ERR_ARG, "vv_set_option: ctx / name is NULL");
  const Option* o = find_option(name);
  const int iv = (int)value;
  if (!o) return fail(VV_ERR_ARG, "vv_set_option: unknown option '%s'", name);
  if (o->kind == OptKind::Retired) {
    if (iv == 0) return VV_OK;
    return fail(VV_ERR_ARG, "vv_set_option: option '%s' is retired; only its fixed value 0 is accepted", name);
  }
  if (o->kind == OptKind::ReadOnly) return fail(VV_ERR_ARG, "vv_set_option: '%s' is read-only (what the launchers last chose)", name);
  return o->set(c, value, iv);
}

int vv_get_option(vv_ctx* c, const char* name, double* value) {
  if (!c || !name || !value) return fail(VV_ERR_ARG, "vv_get_option: NULL argument");
  const Option* o = find_option(name);
  if (!o || !o->get) return fail(VV_ERR_ARG, "vv_get_option: unknown option '%s'", name);
  return o->get(c, value);
}

int vv_set_dedup(vv_ctx* c, int on) {
  if (!c) return fail(VV_ERR_ARG, "vv_set_dedup: ctx is NULL");
  c->dedup = on != 0;
  c->sg_adj = 0; c->gg_seq0 = 0;                                                  // a fresh start for the gradient scale
  return VV_OK;
}

int vv_dedup_stats(vv_ctx* c, int64_t* rows, int64_t* unique_rows) {
  if (!c) return fail(VV_ERR_ARG, "vv_dedup_stats: ctx is NULL");
  if (!grad_exists(c->grad) && !c->last_fwd_only) return fail(VV_ERR_STATE, "vv_dedup_stats: no forward pass yet");
  VV_ENTER(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  int32_t U = c->R;
  if (c->last_dedup) HIPCHK(hipMemcpy(&U, c->dd_info, sizeof(U), hipMemcpyDeviceToHost));
  if (rows) *rows = c->R;
  if (unique_rows) *unique_rows = U;
  return VV_OK;
}

int vv_h16_stats(vv_ctx* c, vv_h16_report* out) {
  if (!c || !out) return fail(VV_ERR_ARG, "vv_h16_stats: ctx / out is NULL");
  if (!grad_exists(c->grad) && !c->last_fwd_only) return fail(VV_ERR_STATE, "vv_h16_stats: no forward pass yet");
  VV_ENTER(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  out->saturated = out->faint_rows = 0;
  if (c->last_h16_counted) {          // the last step's per-workgroup partials, as its kernel left them (whether or not its report has been folded yet)
    std::vector<uint32_t> part((size_t)2 * SEGB_BLOCKS);
    HIPCHK(hipMemcpy(part.data(), c->h16_cnt, part.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < SEGB_BLOCKS; ++i) { out->saturated += part[2 * i]; out->faint_rows += part[2 * i + 1]; }
  }
  out->flagged_steps = c->h16_flagged_steps;
  out->first_flagged_step = c->h16_first_flagged;
  out->fallback = c->h16_fallback ? 1 : 0;
  out->rows_f16 = c->last_h16 ? 1 : 0;
  return VV_OK;
}

int vv_grad_scale_stats(vv_ctx* c, int64_t* repeats, float* scale) {
  if (!c) return fail(VV_ERR_ARG, "vv_grad_scale_stats: ctx is NULL");
  if (repeats) *repeats = c->gg_repeats;
  if (scale) *scale = c->sg;
  return VV_OK;
}

int vv_set_stream(vv_ctx* c, void* s) {
  if (!c) return fail(VV_ERR_ARG, "vv_set_stream: ctx is NULL");
  { const int rcj = vv_comm_join(c); if (rcj) return rcj; }
  HIPCHK(hipStreamSynchronize(c->stream));
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return VV_OK;
}

int vv_synchronize(vv_ctx* c) {
  if (!c) return fail(VV_ERR_ARG, "vv_synchronize: ctx is NULL");
  { const int rcj = vv_comm_join(c); if (rcj) return rcj; }
  HIPCHK(hipStreamSynchronize(c->stream));
  return VV_OK;
}

// ------------------------------------------------------------------------------- table --------
static int table_alloc(vv_ctx* c, int64_t n_rows, int F) {
  if (n_rows <= 0 || F <= 0) return fail(VV_ERR_ARG, "table: n_rows=%lld F=%d", (long long)n_rows, F);
  if (n_rows >= (1ll << 31) - 1) return fail(VV_ERR_ARG, "table: too many rows for int32 indices");
  VV_ENTER(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->D && F != c->F) return fail(VV_ERR_STATE, "table: F=%d differs from the parameters' F=%d", F, c->F);
  dfree(c->table); c->table = nullptr; c->patch_cap = 0;
  c->n_rows = n_rows; c->F = F; c->Fp = (int)round_up(F, F_ALIGN);
  const size_t bytes = (size_t)(n_rows + 1) * c->Fp * sizeof(uint16_t);   // +1: the all-zero row
  HIPCHK(hipMalloc(&c->table, bytes));
  HIPCHK(hipMemsetAsync(c->table, 0, bytes, c->stream));
  return VV_OK;
}

static int set_sx(vv_ctx* c, float sx) {
  c->sx = sx;
  c->ema_packed = false;                     // (the average's 16-bit view carries the table's scale too)
  HIPCHK(hipMemcpyAsync(&c->scales->sx, &c->sx, sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return VV_OK;
}

int vv_table_set(vv_ctx* c, const float* rows, int64_t n_rows, int32_t F) {
  if (!c || !rows) return fail(VV_ERR_ARG, "vv_table_set: NULL argument");
  int rc = table_alloc(c, n_rows, F);
  if (rc) return rc;
  // range guard for f16: keep max|x|*sx inside [2^-8, 2^14]; otherwise move it to ~2^8
  float mx = 0.f;
  {
    // one pass over the host table for max|x| and the first non-finite value; split over a few threads (the scan of a
    // 100 GB table on one core is the longest part of set-up)
    const int64_t total = n_rows * F;
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(16, std::thread::hardware_concurrency()), total >> 22));
    std::vector<float> part_mx(nt, 0.f);
    std::vector<int64_t> part_bad(nt, -1);
    auto scan = [&](int t) {
      const int64_t lo = total * t / nt, hi = total * (t + 1) / nt;
      float m = 0.f; int64_t bad = -1;
      for (int64_t i = lo; i < hi; ++i) {
        const float v = fabsf(rows[i]);
        if (!(v <= 3.0e38f)) { bad = i; break; }
        if (v > m) m = v;
      }
      part_mx[t] = m; part_bad[t] = bad;
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(scan, t);
    scan(0);
    for (auto& x : th) x.join();
    for (int t = 0; t < nt; ++t) {
      if (part_bad[t] >= 0) return fail(VV_ERR_ARG, "vv_table_set: non-finite feature at %lld", (long long)part_bad[t]);
      mx = std::max(mx, part_mx[t]);
    }
  }
  float sx = 1.f;
  if (c->prec == VV_PREC_F16 && mx > 0.f && (mx > 16384.f || mx < 1.f / 256.f)) {
    int e; frexpf(mx, &e); sx = ldexpf(1.f, 8 - e);
  }
  if ((rc = set_sx(c, sx))) return rc;
  const int64_t chunk_rows = std::max<int64_t>(1, (64ll << 20) / ((int64_t)F * 4));
  DevTmp<float> stage;
  HIPCHK(stage.alloc((size_t)chunk_rows * F));
  for (int64_t r0 = 0; r0 < n_rows; r0 += chunk_rows) {
    const int64_t nr = std::min(chunk_rows, n_rows - r0);
    HIPCHK(hipMemcpyAsync(stage, rows + r0 * F, (size_t)nr * F * sizeof(float), hipMemcpyHostToDevice, c->stream));
    launch_table_convert(c->prec, stage, c->table + r0 * c->Fp, nr, F, c->Fp, sx, c->stream);
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  HIPCHK(hipGetLastError());
  return VV_OK;
}

int vv_table_synth(vv_ctx* c, uint64_t seed, int64_t n_rows, int32_t F) {
  if (!c) return fail(VV_ERR_ARG, "vv_table_synth: ctx is NULL");
  int rc = table_alloc(c, n_rows, F);
  if (rc) return rc;
  if ((rc = set_sx(c, 1.f))) return rc;
  launch_table_synth(c->prec, c->table, seed, n_rows, F, c->Fp, 1.f, c->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return VV_OK;
}

int vv_table_get(vv_ctx* c, const int32_t* rows, int64_t n, float* out) {
  if (!c || !out || n <= 0) return fail(VV_ERR_ARG, "vv_table_get: bad argument");
  if (!c->table) return fail(VV_ERR_STATE, "vv_table_get: no table");
  VV_ENTER(c);
  DevTmp<int32_t> drows; DevTmp<float> dout;
  if (rows) {
    for (int64_t i = 0; i < n; ++i)
      if (rows[i] < 0 || rows[i] >= c->n_rows) return fail(VV_ERR_ARG, "vv_table_get: row %d out of range", rows[i]);
    HIPCHK(drows.alloc((size_t)n));
    HIPCHK(hipMemcpy(drows, rows, n * sizeof(int32_t), hipMemcpyHostToDevice));
  } else if (n > c->n_rows) return fail(VV_ERR_ARG, "vv_table_get: n > n_rows");
  HIPCHK(dout.alloc((size_t)n * c->F));
  launch_table_read(c->prec, c->table, drows, n, c->F, c->Fp, 1.f / c->sx, dout, c->stream);
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out, dout, (size_t)n * c->F * sizeof(float), hipMemcpyDeviceToHost));
  return VV_OK;
}

// ------------------------------------------------------------------------------- params -------
int vv_params_set(vv_ctx* c, int32_t D, const float* W, const float* b, const float* hW,
                  const float* hb) {
  if (!c || !W || D <= 0) return fail(VV_ERR_ARG, "vv_params_set: bad argument");
  if (!c->table) return fail(VV_ERR_STATE, "vv_params_set: set the feature table first (defines F)");
  if (c->ema_in_use) return fail(VV_ERR_STATE, "vv_params_set: %s", kEmaInUse);
  VV_ENTER(c);
  { const int rcj = vv_comm_join(c); if (rcj) return rcj; }
  HIPCHK(hipStreamSynchronize(c->stream));
  const int F = c->F;
  const size_t nW = (size_t)D * F;
  if (D != c->D && c->comm) return fail(VV_ERR_STATE, "vv_params_set: the communicator was sized for D = %d (vv_comm_destroy first)", c->D);
  if (D != c->D) {
    dfree(c->W); dfree(c->b); dfree(c->hW); dfree(c->hb); dfree(c->hW2); dfree(c->hb2); dfree(c->Wh); dfree(c->grads_own);
    dfree(c->bank_rec); c->bank_rec = nullptr; c->bank = nullptr;      // (the bank has the gradient buffer's size: the next vv_grads_bank allocates it anew)
    dfree(c->upd_shadow); c->upd_shadow = nullptr;                     // (... and so has vv_debug_mark_update's shadow)
    vv_ema_release(c);                                                    // (... and the moving average: allocated anew below while it is active)
    c->W = c->b = c->hW = c->hb = c->hW2 = c->hb2 = nullptr; c->Wh = nullptr; c->grads = c->grads_own = nullptr;
    c->D = D; c->Dp = (int)round_up(D, D_ALIGN);
#ifdef VV_LAB
    // (lab: VV_LAB_PARAM_ARENA="skew_hW,skew_Wh" bytes -- W, its history and the 16-bit copy in ONE allocation, the second and third a
    // 2-MiB multiple + the given skew behind the first: does the update-in-the-epilogue kernel's speed depend on their relative placement?
    // The arena is never freed: lab processes exit.)
    if (const char* e = getenv("VV_LAB_PARAM_ARENA")) {
      const size_t S = round_up(nW * 4, (size_t)2 << 20);
      const size_t sk1 = (size_t)atoll(e), sk2 = strchr(e, ',') ? (size_t)atoll(strchr(e, ',') + 1) : 0;
      char* arena = nullptr;
      HIPCHK(hipMalloc(&arena, 3 * S + ((size_t)16 << 20)));
      c->W = (float*)arena; c->hW = (float*)(arena + S + sk1); c->Wh = (uint16_t*)(arena + 2 * S + ((size_t)4 << 20) + sk2);
      HIPCHK(hipMalloc(&c->b, D * 4)); HIPCHK(hipMalloc(&c->hb, D * 4));
      fprintf(stderr, "[vv lab] parameter arena: W %p hW %p Wh %p\n", (void*)c->W, (void*)c->hW, (void*)c->Wh);
    } else
#endif
    {
    HIPCHK(hipMalloc(&c->W, nW * 4)); HIPCHK(hipMalloc(&c->hW, nW * 4));
    HIPCHK(hipMalloc(&c->b, D * 4)); HIPCHK(hipMalloc(&c->hb, D * 4));
    HIPCHK(hipMalloc(&c->Wh, (size_t)c->Dp * c->Fp * 2));
    }
    HIPCHK(hipMemset(c->Wh, 0, (size_t)c->Dp * c->Fp * 2));
    HIPCHK(hipMalloc(&c->grads_own, (nW + D) * 4));
    HIPCHK(hipMemset(c->grads_own, 0, (nW + D) * 4));
    c->grads = c->grads_own;
#ifdef VV_LAB
    if (getenv("VV_DEBUG_PTRS")) fprintf(stderr, "[vv ptrs] W %p hW %p Wh %p grads %p (D %d F %d)\n", (void*)c->W, (void*)c->hW, (void*)c->Wh, (void*)c->grads_own, D, c->F);
#endif
    vv_free_batch(c);
  }
  HIPCHK(hipMemcpy(c->W, W, nW * 4, hipMemcpyHostToDevice));
  if (b) HIPCHK(hipMemcpy(c->b, b, D * 4, hipMemcpyHostToDevice)); else HIPCHK(hipMemset(c->b, 0, D * 4));
  if (hW) HIPCHK(hipMemcpy(c->hW, hW, nW * 4, hipMemcpyHostToDevice)); else HIPCHK(hipMemset(c->hW, 0, nW * 4));
  if (hb) HIPCHK(hipMemcpy(c->hb, hb, D * 4, hipMemcpyHostToDevice)); else HIPCHK(hipMemset(c->hb, 0, D * 4));
  // new parameters start a new run of the two-history solver: its second history and its update count go back to zero
  if (c->hW2) { HIPCHK(hipMemset(c->hW2, 0, nW * 4)); HIPCHK(hipMemset(c->hb2, 0, D * 4)); }
  c->adam_t = 0; c->hist2_partial = false;
  c->bank_count = 0; c->grad_banked = false; c->fb_hinted = false;      // banked gradients belonged to the old parameters (vv_grads_bank_reset)
  c->upd_marked = false;                     // (vv_debug_mark_update's shadow too)
  // scale for the half copy from max|W|, then convert (a scale update still pending from an earlier SGD step is void)
  c->scale_pending = false;
  // (a gradient nobody asked for goes with the parameters it belonged to, when the call has succeeded: grad_discard below)
  // ... and so does a hinted step that was waiting for its vv_apply_update (its half-applied update is overwritten here) and a hint not yet
  // consumed (the context was stuck -- every later vv_forward_backward refused, vv_apply_update failing on "no gradients")
  c->upd_hint = false;
  HIPCHK(hipMemsetAsync(&c->scales->wmax_bits, 0, sizeof(unsigned), c->stream));
  launch_absmax(c->W, (int64_t)nW, &c->scales->wmax_bits, c->stream);
  launch_scale_update(c->prec, c->scales, nullptr, 0, c->stream);
  launch_w_convert(c->prec, c->W, c->Wh, D, F, c->Dp, c->Fp, c->scales, c->stream);
  c->params_partial = false;                 // (every rank is given the whole matrix)
  // seed the running max for the first SGD step's scale update
  launch_absmax(c->W, (int64_t)nW, &c->scales->wmax_bits, c->stream);
  c->wmax_seed_live = true;
  HIPCHK(hipGetLastError());
  if (c->ema_decay >= 0.f) { const int rce = vv_ema_init(c); if (rce) return rce; }      // the average starts again from the new values
  HIPCHK(hipStreamSynchronize(c->stream));
  grad_discard(c->grad);
  c->grad_unapplied = false;
  return VV_OK;
}

// Sharded update: every rank holds the fp32 master rows and the history of ITS shard only.  Gathers them -- a COLLECTIVE: every rank of
// the communicator makes the call that leads here (vv_params_get as the facade's Snapshot does, vv_comm_schedule, vv_comm_destroy): one
// grouped all-gather of W, hW and hb (b is complete already).
extern "C++" int vv_gather_params(vv_ctx* c) {
  if (!c->params_partial || !c->comm) { c->params_partial = false; return VV_OK; }
  { const int rcj = vv_comm_join(c); if (rcj) return rcj; }
  const int world = vv::comm_world(c->comm), rps = c->D / world;
  void* bufs[3] = {c->W, c->hW, c->hb};
  const size_t sbytes[3] = {(size_t)rps * c->F * 4, (size_t)rps * c->F * 4, (size_t)rps * 4};
  HIPCHK(hipEventRecord(c->ev_chunk, c->stream));
  HIPCHK(hipStreamWaitEvent(vv::comm_stream(c->comm), c->ev_chunk, 0));
  if (vv::comm_allgather(c->comm, bufs, sbytes, 3, 1)) return fail(VV_ERR_HIP, "all-gather of the parameters: %s", vv::comm_error(c->comm));
  if (c->hist2_partial && c->hW2) {          // (a sharded Adam update: every rank took it, so every rank gathers the second history too)
    void* bufs2[2] = {c->hW2, c->hb2};
    if (vv::comm_allgather(c->comm, bufs2, sbytes + 1, 2, 1)) return fail(VV_ERR_HIP, "all-gather of the second history: %s", vv::comm_error(c->comm));
  }
  c->hist2_partial = false;
  if (vv::comm_record_done(c->comm)) return fail(VV_ERR_HIP, "all-gather of the parameters: %s", vv::comm_error(c->comm));
  HIPCHK(hipStreamWaitEvent(c->stream, vv::comm_done_event(c->comm), 0));
  c->params_partial = false;
  return VV_OK;
}

int vv_params_get(vv_ctx* c, float* W, float* b, float* hW, float* hb) {
  if (!c) return fail(VV_ERR_ARG, "vv_params_get: ctx is NULL");
  { const int rcg = vv_upd_pending_guard(c, "vv_params_get"); if (rcg) return rcg; }
  if (!c->W) return fail(VV_ERR_STATE, "vv_params_get: no parameters");
  VV_ENTER(c);
  { const int rcj = vv_comm_join(c); if (rcj) return rcj; }
  { const int rcg = vv_gather_params(c); if (rcg) return rcg; }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->comm && vv::comm_failed(c->comm)) return fail(VV_ERR_HIP, "vv_params_get: the data-parallel exchange failed: %s", vv::comm_error(c->comm));   // (what the update in flight ran into)
  const size_t nW = (size_t)c->D * c->F;
  if (W) HIPCHK(hipMemcpy(W, c->W, nW * 4, hipMemcpyDeviceToHost));
  if (b) HIPCHK(hipMemcpy(b, c->b, c->D * 4, hipMemcpyDeviceToHost));
  if (hW) HIPCHK(hipMemcpy(hW, c->hW, nW * 4, hipMemcpyDeviceToHost));
  if (hb) HIPCHK(hipMemcpy(hb, c->hb, c->D * 4, hipMemcpyDeviceToHost));
  return VV_OK;
}

// Joins the communication stream: after this, everything the library queued there -- the F-chunks of an overlapped
// update: all-reduce, SGD, publish -- is ordered before whatever the compute stream is given next.  Every entry point
// that reads or writes the parameters, their half copy, the momentum or the gradient buffer goes through here first;
// the one reader that does not is the next step's forward GEMM, which waits chunk by chunk inside the kernel instead.
extern "C++" int vv_comm_join(vv_ctx* c) {
  // UpdSync::Gated: the gated forward GEMM has consumed the update chunk by chunk, but nothing on the compute stream waits for
  // the END of the update's kernels (their plain stores -- W, the history -- are released at that end, not at the gate)
  if (c->comm && c->upd_sync != UpdSync::Joined) {
    HIPCHK(hipStreamWaitEvent(c->stream, vv::comm_done_event(c->comm), 0));
    upd_joined(c->upd_sync);
  }
  if (c->gate_err && *(volatile int32_t*)c->gate_err) {
    *c->gate_err = 0;
    return fail(VV_ERR_STATE, "a forward pass gave up waiting for the overlapped parameter update (a rank failed, or the communication stream stalled)");
  }
  return VV_OK;
}


int vv_loss_get(vv_ctx* c, float* loss, float* violations) {
  if (!c) return fail(VV_ERR_ARG, "vv_loss_get: ctx is NULL");
  if (!grad_exists(c->grad)) return fail(VV_ERR_STATE, "vv_loss_get: no forward pass yet");
  VV_ENTER(c);
  if (c->gate_err && *(volatile int32_t*)c->gate_err) { const int rcj = vv_comm_join(c); if (rcj) return rcj; }
  { const int rcr = vv_reduce_now(c); if (rcr) return rcr; }
  float h[2];
  HIPCHK(hipMemcpyAsync(h, c->loss2, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (loss) *loss = h[0];
  if (violations) *violations = h[1];
  return VV_OK;
}

int vv_grads_device(vv_ctx* c, void** dev_ptr, int64_t* n_floats) {
  if (!c || !dev_ptr || !n_floats) return fail(VV_ERR_ARG, "vv_grads_device: NULL argument");
  { const int rcg = vv_upd_pending_guard(c, "vv_grads_device"); if (rcg) return rcg; }
  if (!c->grads) return fail(VV_ERR_STATE, "vv_grads_device: no parameters");
  { const int rcr = vv_reduce_now(c); if (rcr) return rcr; }      // (whoever reads the buffer on the stream finds the gradient queued in front)
  c->grads_exposed = true;                                     // ... and every later one at the end of its vv_forward_backward
  *dev_ptr = c->grads;
  *n_floats = (int64_t)c->D * c->F + c->D;
  return VV_OK;
}

int vv_grads_bind(vv_ctx* c, void* dev_ptr) {
  { const int rcg = vv_upd_pending_guard(c, "vv_grads_bind"); if (rcg) return rcg; }
  if (!c) return fail(VV_ERR_ARG, "vv_grads_bind: ctx is NULL");
  if (!c->grads_own) return fail(VV_ERR_STATE, "vv_grads_bind: no parameters");
  // no synchronisation: kernels already queued keep the pointer they were launched with; the next
  // vv_forward_backward writes, and the next vv_apply_update reads, the newly bound buffer
  { const int rcr = vv_reduce_now(c); if (rcr) return rcr; }      // (a reduction still due goes to the buffer it was computed for)
  c->grads = dev_ptr ? (float*)dev_ptr : c->grads_own;
  return VV_OK;
}

int vv_grads_get(vv_ctx* c, float* dW, float* db) {
  { const int rcg = vv_upd_pending_guard(c, "vv_grads_get"); if (rcg) return rcg; }
  if (!c) return fail(VV_ERR_ARG, "vv_grads_get: ctx is NULL");
  if (!grad_exists(c->grad)) return fail(VV_ERR_STATE, "vv_grads_get: no backward pass yet");
  VV_ENTER(c);
  { const int rcj = vv_comm_join(c); if (rcj) return rcj; }       // block-wise all-reduces in flight: the buffer is read whole
  { const int rcr = vv_reduce_now(c); if (rcr) return rcr; }
  HIPCHK(hipStreamSynchronize(c->stream));
  const size_t nW = (size_t)c->D * c->F;
  const GradLayout layout = c->grad.buf.layout;
  if (layout == GradLayout::Sharded) {              // shard-major buffer (ReduceArgs::shard_rows) -> the blob's [dW | db]
    const int rps = c->D / vv::comm_world(c->comm);
    const size_t sf = (size_t)rps * c->F + rps;
    std::vector<float> tmp(nW + c->D);
    HIPCHK(hipMemcpy(tmp.data(), c->grads, tmp.size() * 4, hipMemcpyDeviceToHost));
    for (int s = 0; s * rps < c->D; ++s) {
      if (dW) memcpy(dW + (size_t)s * rps * c->F, tmp.data() + s * sf, (size_t)rps * c->F * 4);
      if (db) memcpy(db + (size_t)s * rps, tmp.data() + s * sf + (size_t)rps * c->F, (size_t)rps * 4);
    }
    return VV_OK;
  }
  if (dW && layout != GradLayout::Chunked) HIPCHK(hipMemcpy(dW, c->grads, nW * 4, hipMemcpyDeviceToHost));
  if (dW && layout == GradLayout::Chunked) {        // chunk-major buffer (ReduceArgs::n_chunks) -> the blob's row-major D x F
    std::vector<float> tmp(nW);
    HIPCHK(hipMemcpy(tmp.data(), c->grads, nW * 4, hipMemcpyDeviceToHost));
    const int nch = vv_chunk_plan(c);
    for (int k = 0; k < nch; ++k) {
      const int c0 = std::min(c->F, c->chunk_kt[k] * BK), c1 = std::min(c->F, c->chunk_kt[k + 1] * BK);
      for (int d = 0; d < c->D && c1 > c0; ++d)
        memcpy(dW + (size_t)d * c->F + c0, tmp.data() + (size_t)c->D * c0 + (size_t)d * (c1 - c0), (size_t)(c1 - c0) * 4);
    }
  }
  if (db) HIPCHK(hipMemcpy(db, c->grads + nW, c->D * 4, hipMemcpyDeviceToHost));
  return VV_OK;
}

int vv_blobs_get(vv_ctx* c, float* ip2, float* target_score, float* negative_scores, float* ip1_diff) {
  if (!c) return fail(VV_ERR_ARG, "vv_blobs_get: ctx is NULL");
  if (!grad_exists(c->grad) && !c->last_fwd_only) return fail(VV_ERR_STATE, "vv_blobs_get: no forward pass yet");
  if (ip1_diff && c->last_fwd_only) return fail(VV_ERR_STATE, "vv_blobs_get: ip1_diff after vv_forward -- the forward-only pass computes no gradient (until the next backward pass)");
  VV_ENTER(c);
  { const int rcj = vv_comm_join(c); if (rcj) return rcj; }
  HIPCHK(hipStreamSynchronize(c->stream));
  const int B = c->B, CN = c->C + c->Nn, D = c->D, Nn = c->Nn;
  const size_t n = (size_t)c->R * D;
  auto reorder = [&](const std::vector<float>& src, float* dst) {   // (b*CN+ch) -> (ch*B+b)
    for (int bb = 0; bb < B; ++bb)
      for (int ch = 0; ch < CN; ++ch)
        memcpy(dst + ((size_t)ch * B + bb) * D, src.data() + ((size_t)bb * CN + ch) * D, (size_t)D * 4);
  };
  if (ip2) {
    std::vector<float> tmp(n);
    if (c->last_dedup) {               // expand the per-slot rows back to one row per instance
      DevTmp<float> d;
      HIPCHK(d.alloc(n));
      if (c->last_drop.mode) launch_gather_rows_dropout(c->H, c->dd_map, c->R, D, c->last_drop, d, c->stream, c->last_h16);    // the instance's own mask on the shared row
      else launch_gather_rows_f32(c->H, c->dd_map, c->R, D, d, c->stream, c->last_h16);
      HIPCHK(hipStreamSynchronize(c->stream));
      HIPCHK(hipMemcpy(tmp.data(), d, n * 4, hipMemcpyDeviceToHost));
    } else {
      HIPCHK(hipMemcpy(tmp.data(), c->H, n * 4, hipMemcpyDeviceToHost));
    }
    reorder(tmp, ip2);
  }
  if (target_score) {
    std::vector<float> st(B);
    HIPCHK(hipMemcpy(st.data(), c->s_true, (size_t)B * 4, hipMemcpyDeviceToHost));
    for (int bb = 0; bb < B; ++bb) for (int k = 0; k < Nn; ++k) target_score[(size_t)bb * Nn + k] = st[bb];
  }
  if (negative_scores) HIPCHK(hipMemcpy(negative_scores, c->s_bogus, (size_t)B * Nn * 4, hipMemcpyDeviceToHost));
  if (ip1_diff) {
    DevTmp<float> d;
    HIPCHK(d.alloc(n));
    DevTmp<uint16_t> ungrouped;
    // the scale the step's 16-bit gradients really carry: the host's sg times what the guard's repeats took off
    float sgf = c->sg;
    if (c->prec == VV_PREC_F16) {
      GradGuard gh;
      HIPCHK(hipMemcpy(&gh, c->gg, sizeof(gh), hipMemcpyDeviceToHost));
      sgf *= gh.mul;
    }
    DevTmp<float> yrows; DevTmp<uint16_t> dyrows;
    bool expanded = false;
    const int score_form = c->ko.last_score_form;     // ("last_score_form" names the forward pass's kernel, not this accessor's)
    if (c->last_seg_bwd && (c->last_drop.mode || c->last_h16)) {
      // ... with dropout: the instances' masked rows are materialised (item-major) and the per-instance kernel runs on them as on a
      // dense batch whose forward pass applied the mask -- its gradient rows come out per instance, nothing to ungroup
      // (... and with ip2 stored as f16: the per-instance kernel reads fp32 rows -- the instances' rows are materialised as such)
      HIPCHK(yrows.alloc(n));
      HIPCHK(dyrows.alloc((size_t)(c->Rp + BK) * c->Dp));
      if (c->last_drop.mode) launch_gather_rows_dropout(c->H, c->dd_map, c->R, D, c->last_drop, yrows, c->stream, c->last_h16);
      else launch_gather_rows_f32(c->H, c->dd_map, c->R, D, yrows, c->stream, c->last_h16);
      ScoreArgs la = c->last_score;
      la.H = yrows; la.dYh = dyrows; la.map = nullptr; la.seg_start = nullptr; la.ord = nullptr; la.V = nullptr; la.rec = nullptr;
      la.drop = DropSpec(); la.bound_out = nullptr; la.h16 = 0;
      la.sg = sgf; la.guard = GuardArgs();
      launch_score_loss(c->prec, la, c->stream);
      c->ko.last_score_form = score_form;
      expanded = true;
    } else if (c->last_seg_bwd) {
      // the step kept its backward factored: produce the per-instance rows now (same forward values; the loss partials
      // it rewrites are the ones already there, its bias partials go to the buffer the step did not use)
      ScoreArgs la = c->last_score;
      la.sg = sgf; la.guard = GuardArgs();
      launch_score_loss(c->prec, la, c->stream);
      c->ko.last_score_form = score_form;
    }
    if (expanded) {
      launch_dyh_to_float(c->prec, dyrows, c->R, D, c->Dp, 1.f / sgf, d, c->stream);
      HIPCHK(hipStreamSynchronize(c->stream));
      std::vector<float> tmp(n);
      HIPCHK(hipMemcpy(tmp.data(), d, n * 4, hipMemcpyDeviceToHost));
      reorder(tmp, ip1_diff);
      return VV_OK;
    }
    if (c->last_dedup) {
      HIPCHK(ungrouped.alloc((size_t)c->R * c->Dp));
      DedupArgs da;
      memset(&da, 0, sizeof(da));
      da.map = c->dd_map; da.ord = c->dd_ord; da.seg_start = c->dd_seg; da.pos = c->dd_pos; da.R = c->R;
      launch_dedup_pos(da, c->stream);
      launch_gather_rows_u16(c->dYh, c->dd_pos, c->R, c->Dp, ungrouped, c->stream);
    }
    launch_dyh_to_float(c->prec, ungrouped.p ? ungrouped.p : c->dYh, c->R, D, c->Dp, 1.f / sgf, d, c->stream);
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<float> tmp(n);
    HIPCHK(hipMemcpy(tmp.data(), d, n * 4, hipMemcpyDeviceToHost));
    reorder(tmp, ip1_diff);
  }
  return VV_OK;
}

// ---- magnitude statistics (the reference's debug_info: Net::ForwardDebugInfo / BackwardDebugInfo / UpdateDebugInfo, net.cpp:580-636,
// over Blob::asum_data / asum_diff, blob.cpp:138-165)
static_assert(sizeof(vv_abs_stat) == sizeof(AbsRec) && offsetof(vv_abs_stat, amax) == offsetof(AbsRec, amax) &&
              offsetof(vv_abs_stat, count) == offsetof(AbsRec, count) && offsetof(vv_abs_stat, nonfinite) == offsetof(AbsRec, nonfinite),
              "k_abs_stats writes the ABI's records");
static constexpr int kStatRecs = VV_STAT_N + 1;              // the named entries, then vv_op_asum's own
static constexpr size_t kStatParts = (size_t)STAT_SEGS * STAT_BLOCKS;
// the record block: here on the first call that measures, never on the step path afterwards
static int stats_ensure(vv_ctx* c) {
  if (c->stat_rec) return VV_OK;
  const size_t bytes = kStatRecs * sizeof(AbsRec) + kStatParts * (sizeof(double) + sizeof(unsigned long long) + sizeof(float)) + 16;
  HIPCHK(hipMalloc((void**)&c->stat_rec, bytes));
  HIPCHK(hipMemset(c->stat_rec, 0, bytes));
  HIPCHK(hipDeviceSynchronize());            // (the fill is complete before a kernel of any stream reads it)
  return VV_OK;
}
static AbsStatsArgs stats_args(vv_ctx* c) {
  AbsStatsArgs a;
  memset(&a, 0, sizeof(a));
  a.rec = c->stat_rec;
  a.part_sum = (double*)(c->stat_rec + kStatRecs);
  a.part_nf = (unsigned long long*)(a.part_sum + kStatParts);
  a.part_max = (float*)(a.part_nf + kStatParts);
  a.arrived = (uint32_t*)(a.part_max + kStatParts);
  return a;
}
int vv_op_asum(vv_ctx* c, const float* x_dev, int64_t n, vv_abs_stat* out) {
  if (!c || !x_dev || !out) return fail(VV_ERR_ARG, "vv_op_asum: NULL argument");
  if (n < 1) return fail(VV_ERR_ARG, "vv_op_asum: n = %lld (at least one element)", (long long)n);
  VV_ENTER(c);
  int rc = stats_ensure(c);
  if (rc) return rc;
  AbsStatsArgs a = stats_args(c);
  a.seg[0] = {x_dev, nullptr, n, STAT_F32, VV_STAT_N};
  a.nseg = 1;
  PROFILED(c, "abs_stats", launch_abs_stats(a, c->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, c->stat_rec + VV_STAT_N, sizeof(*out), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return VV_OK;
}
static inline size_t shadow_b_off(const vv_ctx* c) { return round_up((size_t)c->D * c->F, (size_t)4); }      // b's copy: on a 16-byte boundary, as b itself
static const char* const kStatSharded = "the sharded schedule (2) is selected -- the fp32 master copy and the history are complete on their owner only (vv_comm_schedule(0))";
int vv_debug_mark_update(vv_ctx* c) {
  if (!c) return fail(VV_ERR_ARG, "vv_debug_mark_update: ctx is NULL");
  if (!c->W) return fail(VV_ERR_STATE, "vv_debug_mark_update: no parameters");
  if (c->comm_sharded) return fail(VV_ERR_STATE, "vv_debug_mark_update: %s", kStatSharded);
  int rc = vv_upd_pending_guard(c, "vv_debug_mark_update");       // (a hinted step's parameters are half-way until its vv_apply_update)
  if (rc) return rc;
  VV_ENTER(c);
  if ((rc = vv_comm_join(c))) return rc;
  if (!c->upd_shadow) {                      // the one allocation: here, never on the step path afterwards
    HIPCHK(hipMalloc((void**)&c->upd_shadow, (shadow_b_off(c) + c->D) * sizeof(float)));
    HIPCHK(hipDeviceSynchronize());
  }
  HIPCHK(hipMemcpyAsync(c->upd_shadow, c->W, (size_t)c->D * c->F * 4, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->upd_shadow + shadow_b_off(c), c->b, (size_t)c->D * 4, hipMemcpyDeviceToDevice, c->stream));
  c->upd_marked = true;
  return VV_OK;
}
int vv_debug_stats_queue(vv_ctx* c, uint32_t mask) {
  if (!c) return fail(VV_ERR_ARG, "vv_debug_stats_queue: ctx is NULL");
  if (mask == 0 || mask >= (1u << VV_STAT_N)) return fail(VV_ERR_ARG, "vv_debug_stats_queue: mask 0x%x names no entry, or one past VV_STAT_N", mask);
  auto has = [&](int e) { return (mask >> e & 1u) != 0; };
  const bool want_grad = has(VV_STAT_DW) || has(VV_STAT_DB), want_score = has(VV_STAT_TARGET_SCORE) || has(VV_STAT_NEGATIVE_SCORES);
  const bool want_upd = has(VV_STAT_UPD_W) || has(VV_STAT_UPD_B);
  const bool want_master = has(VV_STAT_W) || has(VV_STAT_HIST_W) || has(VV_STAT_HIST_B) || want_upd;
  const bool want_param = want_master || has(VV_STAT_B);
  if ((want_param || want_grad) && !c->W) return fail(VV_ERR_STATE, "vv_debug_stats_queue: no parameters");
  int rc;
  if (want_master) if (c->comm_sharded) return fail(VV_ERR_STATE, "vv_debug_stats_queue: W / history entries while %s", kStatSharded);
  if (want_param && (rc = vv_upd_pending_guard(c, "vv_debug_stats_queue"))) return rc;
  if (want_upd && !c->upd_marked) return fail(VV_ERR_STATE, "vv_debug_stats_queue: UPD_W / UPD_B without a vv_debug_mark_update in front of the update");
  if (want_score && !grad_exists(c->grad) && !c->last_fwd_only) return fail(VV_ERR_STATE, "vv_debug_stats_queue: score entries before any forward pass");
  if (want_grad) {
    if (!grad_exists(c->grad)) return fail(VV_ERR_STATE, "vv_debug_stats_queue: gradient entries before any backward pass");
    if (c->fb_hinted || c->grad.at == GradAt::SlabsWUpdated || c->grad.at == GradAt::Lost)
      return fail(VV_ERR_STATE, "vv_debug_stats_queue: gradient entries of a step announced by vv_update_hint: its gradient is not kept (run the step without the hint to measure it)");
    if (c->grad.at == GradAt::Buffer && c->grad.buf.layout != GradLayout::Flat)
      return fail(VV_ERR_STATE, "vv_debug_stats_queue: this step's gradient was laid out chunk- or shard-major for the overlapped / sharded schedule (vv_comm_schedule(0))");
  }
  VV_ENTER(c);
  if ((rc = vv_comm_join(c))) return rc;
  if ((rc = stats_ensure(c))) return rc;
  if (want_grad && (rc = vv_reduce_now(c))) return rc;            // the gradient into the flat buffer, as any reader brings it (vv_grads_get)
  const int64_t nW = (int64_t)c->D * c->F, D = c->D, B = c->B;
  const float* const sh = c->upd_shadow;
  const AbsSeg all[VV_STAT_N] = {
    {c->W, nullptr, nW, STAT_F32, VV_STAT_W}, {c->b, nullptr, D, STAT_F32, VV_STAT_B},
    {c->hW, nullptr, nW, STAT_F32, VV_STAT_HIST_W}, {c->hb, nullptr, D, STAT_F32, VV_STAT_HIST_B},
    {c->grads, nullptr, nW, STAT_F32, VV_STAT_DW}, {c->grads ? c->grads + nW : nullptr, nullptr, D, STAT_F32, VV_STAT_DB},
    {c->s_true, nullptr, B, STAT_F32, VV_STAT_TARGET_SCORE}, {c->s_bogus, nullptr, B * c->Nn, STAT_F32, VV_STAT_NEGATIVE_SCORES},
    {sh, c->W, nW, STAT_F32, VV_STAT_UPD_W}, {sh ? sh + shadow_b_off(c) : nullptr, c->b, D, STAT_F32, VV_STAT_UPD_B}};
  AbsStatsArgs a = stats_args(c);
  for (int e = 0; e < VV_STAT_N; ++e) {
    if (!has(e)) continue;
    if (!all[e].p || all[e].n < 1) return fail(VV_ERR_STATE, "vv_debug_stats_queue: entry %d has no buffer yet", e);
    a.seg[a.nseg++] = all[e];
    if (a.nseg == STAT_SEGS) { PROFILED(c, "abs_stats", launch_abs_stats(a, c->stream)); a.nseg = 0; }      // (more than STAT_SEGS entries: a second launch behind the first)
  }
  if (a.nseg) PROFILED(c, "abs_stats", launch_abs_stats(a, c->stream));
  HIPCHK(hipGetLastError());
  return VV_OK;
}
int vv_debug_stats_get(vv_ctx* c, vv_abs_stat* out) {
  if (!c || !out) return fail(VV_ERR_ARG, "vv_debug_stats_get: ctx / out is NULL");
  memset(out, 0, VV_STAT_N * sizeof(*out));
  if (!c->stat_rec) return VV_OK;              // nothing was ever queued
  VV_ENTER(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out, c->stat_rec, VV_STAT_N * sizeof(*out), hipMemcpyDeviceToHost));
  return VV_OK;
}

// debug / test accessor: the grouping of the last de-duplicated step as the kernels left it, from the set that step used (read-only:
// the one launch is k_dd_pos into the debug buffer, as vv_blobs_get(ip1_diff) does)
int vv_dedup_groups_get(vv_ctx* c, int32_t* rows, int32_t* uniq_rows, int32_t* map, int32_t* ord, int32_t* cnt, int32_t* seg_start,
                        int32_t* pos, float* dyu, float* scale) {
  if (!c) return fail(VV_ERR_ARG, "vv_dedup_groups_get: ctx is NULL");
  if (c->last_fwd_only) return fail(VV_ERR_STATE, "vv_dedup_groups_get: the last forward pass was vv_forward's -- its grouping belongs to no backward pass (until the next one)");
  if (!grad_exists(c->grad)) return fail(VV_ERR_STATE, "vv_dedup_groups_get: no forward pass yet");
  if (!c->last_dedup) return fail(VV_ERR_STATE, "vv_dedup_groups_get: the last forward pass was dense (vv_set_dedup, dropout)");
  VV_ENTER(c);
  { const int rcj = vv_comm_join(c); if (rcj) return rcj; }
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipStreamSynchronize(c->dd_stream));
  const size_t R = (size_t)c->R, Rp = (size_t)c->Rp;
  int32_t U = 0;
  HIPCHK(hipMemcpy(&U, c->dd_info, sizeof(U), hipMemcpyDeviceToHost));
  if (U < 0 || (size_t)U > R) return fail(VV_ERR_STATE, "internal error: the grouping reports %d distinct rows of %d", (int)U, c->R);
  if (rows) HIPCHK(hipMemcpy(rows, c->dd_rows, Rp * 4, hipMemcpyDeviceToHost));
  if (uniq_rows) HIPCHK(hipMemcpy(uniq_rows, c->dd_uniq, Rp * 4, hipMemcpyDeviceToHost));
  if (map) HIPCHK(hipMemcpy(map, c->dd_map, R * 4, hipMemcpyDeviceToHost));
  if (ord) HIPCHK(hipMemcpy(ord, c->dd_ord, R * 4, hipMemcpyDeviceToHost));
  if (cnt) HIPCHK(hipMemcpy(cnt, c->dd_cnt, Rp * 4, hipMemcpyDeviceToHost));
  if (seg_start) HIPCHK(hipMemcpy(seg_start, c->dd_seg, ((size_t)U + 1) * 4, hipMemcpyDeviceToHost));
  if (pos) {
    DedupArgs da;
    memset(&da, 0, sizeof(da));
    da.map = c->dd_map; da.ord = c->dd_ord; da.seg_start = c->dd_seg; da.pos = c->dd_pos; da.R = c->R;
    launch_dedup_pos(da, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(pos, c->dd_pos, R * 4, hipMemcpyDeviceToHost));
  }
  // the scale the step's 16-bit gradients really carry: the host's sg times what the guard's repeats took off
  float sgf = c->sg;
  if ((dyu || scale) && c->prec == VV_PREC_F16) {
    GradGuard gh;
    HIPCHK(hipMemcpy(&gh, c->gg, sizeof(gh), hipMemcpyDeviceToHost));
    sgf *= gh.mul;
  }
  if (dyu) {
    DevTmp<float> d;
    HIPCHK(d.alloc(Rp * c->D));
    launch_dyh_to_float(c->prec, c->dYu, c->Rp, c->D, c->Dp, 1.f / sgf, d, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(dyu, d, Rp * c->D * 4, hipMemcpyDeviceToHost));
  }
  if (scale) *scale = sgf;
  return VV_OK;
}

// ------------------------------------------------------------------------------- embed --------
// The two embedding forms with the result left on the device (dout: fp32 [n][D], the caller's): vv_embed / vv_embed_mean
// download it, vv_gallery_from_table keeps it.  `who` names the entry point in messages.
// the common end of the two forms: the plain projection of n table rows (drows: device, padded to R_ALIGN) into dout, normalised on request; synchronises
static int embed_project(vv_ctx* c, const int32_t* drows, int64_t n, int relu, int l2norm, float* dout) {
  ParamView pv;                                // (the training parameters, or under vv_ema_use(1) the average's)
  { const int rcv = vv_param_view(c, &pv); if (rcv) return rcv; }
  FwdArgs fa;
  fa.table = c->table; fa.rows = drows; fa.Wh = pv.Wh; fa.bias = pv.b; fa.scales = pv.scales;
  fa.H = dout; fa.R = (int)n; fa.D = c->D; fa.Fp = c->Fp; fa.relu = relu ? 1 : 0; fa.zero_row = (int32_t)c->n_rows;
  fa.drop_ratio = 0.f; fa.mask = nullptr; fa.drop_seed = 0; fa.B = 1; fa.CN = 1;
  launch_fwd_gemm(c->prec, fa, c->stream);
  if (l2norm) launch_row_normalize(dout, (int)n, c->D, c->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return VV_OK;
}

extern "C++" int vv_embed_rows_device(vv_ctx* c, const char* who, const int32_t* rows, int64_t n, int relu, int l2norm, float* dout) {
  const int Rp = (int)round_up(n, R_ALIGN);
  std::vector<int32_t> h(Rp, (int32_t)c->n_rows);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t r = rows ? rows[i] : i;
    if (r < 0 || r >= c->n_rows) return fail(VV_ERR_ARG, "%s: row %lld out of range", who, (long long)r);
    h[i] = (int32_t)r;
  }
  DevTmp<int32_t> drows;
  HIPCHK(drows.alloc((size_t)Rp));
  HIPCHK(hipMemcpyAsync(drows, h.data(), (size_t)Rp * 4, hipMemcpyHostToDevice, c->stream));
  return embed_project(c, drows, n, relu, l2norm, dout);
}

extern "C++" int vv_embed_mean_device(vv_ctx* c, const char* who, const int32_t* rows, int64_t n, int32_t k, const float* coeff,
                                      int relu, int l2norm, float* dout) {
  for (int64_t i = 0; i < n * k; ++i)
    if (rows[i] < 0 || rows[i] >= c->n_rows) return fail(VV_ERR_ARG, "%s: row %d out of range", who, rows[i]);
  int rc = vv_ensure_scratch_rows(c, n);
  if (rc) return rc;
  std::vector<float> hc(k);
  for (int j = 0; j < k; ++j) hc[j] = coeff ? coeff[j] : 1.0f / k;
  const int Rp = (int)round_up(n, R_ALIGN);
  std::vector<int32_t> h(Rp, (int32_t)c->n_rows);
  for (int64_t i = 0; i < n; ++i) h[i] = (int32_t)(c->n_rows + 1 + i);
  DevTmp<int32_t> drows_in, drows; DevTmp<float> dcoeff;
  HIPCHK(drows_in.alloc((size_t)n * k)); HIPCHK(drows.alloc((size_t)Rp));
  HIPCHK(dcoeff.alloc((size_t)k));
  HIPCHK(hipMemcpyAsync(drows_in, rows, (size_t)n * k * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(drows, h.data(), (size_t)Rp * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dcoeff, hc.data(), (size_t)k * 4, hipMemcpyHostToDevice, c->stream));
  launch_mean_rows(c->prec, c->table, drows_in, n, k, dcoeff, c->n_rows + 1, c->Fp, c->stream);
  return embed_project(c, drows, n, relu, l2norm, dout);
}

int vv_embed(vv_ctx* c, const int32_t* rows, int64_t n, int relu, int l2norm, float* out) {
  if (!c || !out || n <= 0) return fail(VV_ERR_ARG, "vv_embed: bad argument");
  if (!c->table || !c->W) return fail(VV_ERR_STATE, "vv_embed: table and parameters must be set first");
  if (n > (1ll << 30)) return fail(VV_ERR_ARG, "vv_embed: n too large");
  { const int rcg = vv_upd_pending_guard(c, "vv_embed"); if (rcg) return rcg; }     // (a hinted step half-way: new half copy, old bias)
  VV_ENTER(c);
  { const int rcj = vv_comm_join(c); if (rcj) return rcj; }
  DevTmp<float> dout;
  HIPCHK(dout.alloc((size_t)n * c->D));
  const int rc = vv_embed_rows_device(c, "vv_embed", rows, n, relu, l2norm, dout);
  if (rc) return rc;
  HIPCHK(hipMemcpy(out, dout, (size_t)n * c->D * 4, hipMemcpyDeviceToHost));
  return VV_OK;
}

int vv_embed_mean(vv_ctx* c, const int32_t* rows, int64_t n, int32_t k, const float* coeff, int relu,
                  int l2norm, float* out) {
  if (!c || !rows || !out || n <= 0 || k <= 0) return fail(VV_ERR_ARG, "vv_embed_mean: bad argument");
  if (!c->table || !c->W) return fail(VV_ERR_STATE, "vv_embed_mean: table and parameters must be set first");
  if (n > (1ll << 24)) return fail(VV_ERR_ARG, "vv_embed_mean: n too large");
  { const int rcg = vv_upd_pending_guard(c, "vv_embed_mean"); if (rcg) return rcg; }     // (a hinted step half-way: new half copy, old bias)
  VV_ENTER(c);
  { const int rcj = vv_comm_join(c); if (rcj) return rcj; }
  DevTmp<float> dout;
  HIPCHK(dout.alloc((size_t)n * c->D));
  const int rc = vv_embed_mean_device(c, "vv_embed_mean", rows, n, k, coeff, relu, l2norm, dout);
  if (rc) return rc;
  HIPCHK(hipMemcpy(out, dout, (size_t)n * c->D * 4, hipMemcpyDeviceToHost));
  return VV_OK;
}

// ------------------------------------------------------------------------------- data parallel -
int vv_comm_init(vv_ctx* c, int32_t world, int32_t rank, const char* id_path, int32_t transport) {
  if (!c) return fail(VV_ERR_ARG, "vv_comm_init: ctx is NULL");
  if (world < 1 || rank < 0 || rank >= world) return fail(VV_ERR_ARG, "vv_comm_init: rank %d of %d", rank, world);
  if (world > 1 && (!id_path || !*id_path)) return fail(VV_ERR_ARG, "vv_comm_init: id_path is required for world > 1");
  if (transport != VV_COMM_RCCL && transport != VV_COMM_SHM && transport != VV_COMM_PEER) return fail(VV_ERR_ARG, "vv_comm_init: unknown transport %d", transport);
  if (!c->W) return fail(VV_ERR_STATE, "vv_comm_init: set the parameters first (they size the gradient buffer)");
  if (c->comm) return fail(VV_ERR_STATE, "vv_comm_init: a communicator already exists");
  { const int rcg = vv_upd_pending_guard(c, "vv_comm_init"); if (rcg) return rcg; }
  VV_ENTER(c);
  std::string err;
  c->comm = vv::comm_create(world, rank, id_path ? id_path : "", transport, (size_t)c->D * c->F + c->D, &err);
  if (!c->comm) return fail(VV_ERR_HIP, "vv_comm_init: %s", err.c_str());
  if (!c->ev_chunk) HIPCHK(hipEventCreateWithFlags(&c->ev_chunk, hipEventDisableTiming));
  return VV_OK;
}

int vv_comm_overlap(vv_ctx* c, int on) {
  if (!c) return fail(VV_ERR_ARG, "vv_comm_overlap: ctx is NULL");
  if (on) if (const char* why = vv_sync_only_feature(c)) return fail(VV_ERR_STATE, "vv_comm_overlap: %s", why);
  if (c->comm_sharded) if (on && c->params_partial) { VV_ENTER(c); const int rcg = vv_gather_params(c); if (rcg) return rcg; }   // (collective, as in vv_comm_schedule: leaving the sharded schedule)
  c->comm_overlap = on != 0;
  if (on) c->comm_sharded = false;
  return VV_OK;
}

int vv_comm_schedule(vv_ctx* c, int schedule) {
  if (!c) return fail(VV_ERR_ARG, "vv_comm_schedule: ctx is NULL");
  if (schedule < 0 || schedule > 2) return fail(VV_ERR_ARG, "vv_comm_schedule: 0 sync, 1 overlap, 2 sharded");
  if (schedule != 0) if (const char* why = vv_sync_only_feature(c)) return fail(VV_ERR_STATE, "vv_comm_schedule: %s", why);
  { const int rcg = vv_upd_pending_guard(c, "vv_comm_schedule"); if (rcg) return rcg; }
  if (schedule != 2 && c->params_partial) { VV_ENTER(c); const int rcg = vv_gather_params(c); if (rcg) return rcg; }     // (collective: the other schedules update the whole matrix)
  c->comm_overlap = schedule == 1;
  c->comm_sharded = schedule == 2;
  return VV_OK;
}

int vv_allreduce_grads(vv_ctx* c) {
  { const int rcg = vv_upd_pending_guard(c, "vv_allreduce_grads"); if (rcg) return rcg; }
  if (!c) return fail(VV_ERR_ARG, "vv_allreduce_grads: ctx is NULL");
  if (!c->comm) { grad_summed(c->grad); return VV_OK; }
  if (!grad_exists(c->grad)) return fail(VV_ERR_STATE, "vv_allreduce_grads: no gradients (call vv_forward_backward)");
  if (!grad_sum_due(c->grad)) return VV_OK;                    // already summed
  if (c->grad.buf.layout != GradLayout::Flat) return VV_OK;    // overlapped / sharded schedule: vv_apply_update runs the exchange
  VV_ENTER(c);
  // synchronous schedule over RCCL: the collective goes straight into the compute stream (nothing would run beside it)
  const int rc = vv::comm_allreduce_inline(c->comm, c->grads, (size_t)c->D * c->F + c->D, c->stream);
  if (rc < 0) return fail(VV_ERR_HIP, "all-reduce: %s", vv::comm_error(c->comm));
  if (rc == 0) { grad_summed(c->grad); return VV_OK; }
  HIPCHK(hipEventRecord(c->ev_chunk, c->stream));
  if (vv::comm_allreduce(c->comm, c->grads, 0, (size_t)c->D * c->F + c->D, c->ev_chunk))
    return fail(VV_ERR_HIP, "all-reduce: %s", vv::comm_error(c->comm));
  HIPCHK(hipStreamWaitEvent(c->stream, vv::comm_done_event(c->comm), 0));   // the update waits for the sum; the host does not
  grad_summed(c->grad);
  return VV_OK;
}

int vv_comm_destroy(vv_ctx* c) {
  if (!c) return VV_OK;
  if (c->comm) {
    (void)hipSetDevice(c->device);
    (void)vv_gather_params(c);                    // (collective: a sharded update leaves the master parameters whole again)
    (void)vv_comm_join(c); (void)hipStreamSynchronize(c->stream); vv::comm_destroy(c->comm); c->comm = nullptr;
  }
  grad_comm_destroyed(c->grad); upd_joined(c->upd_sync); c->params_partial = false;
  return VV_OK;
}

// ------------------------------------------------------------------------------- profiling ----
int vv_profile_enable(vv_ctx* c, int on) {
  if (!c) return fail(VV_ERR_ARG, "vv_profile_enable: ctx is NULL");
  HIPCHK(hipStreamSynchronize(c->stream));
  c->prof_map.clear();
  c->ev_used = 0;
  c->prof = on != 0;
  c->prof_every = on > 1 ? on : 1;
  c->prof_calls = 0;
  return VV_OK;
}

int vv_profile_select(vv_ctx* c, const char* kernels) {
  if (!c) return fail(VV_ERR_ARG, "vv_profile_select: ctx is NULL");
  c->prof_only = (kernels && *kernels) ? "," + std::string(kernels) + "," : std::string();
  return VV_OK;
}

int vv_profile_get(vv_ctx* c, const char* kernel, double* avg_ms, int64_t* launches) {
  if (!c || !kernel) return fail(VV_ERR_ARG, "vv_profile_get: NULL argument");
  HIPCHK(hipStreamSynchronize(c->stream));
  auto it = c->prof_map.find(kernel);
  double tot = 0; int64_t n = 0;
  if (it != c->prof_map.end())
    for (auto& e : it->second.ev) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) { tot += ms; ++n; }
    }
  if (avg_ms) *avg_ms = n ? tot / n : 0.0;
  if (launches) *launches = n;
  return VV_OK;
}

}  // extern "C"
