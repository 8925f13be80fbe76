// api.hip -- implementation of the C ABI in include/videovec.h (gfx950 / HIP only; there is no CPU fallback: every entry point fails with
// VV_ERR_NOGPU / VV_ERR_HIP when no device is usable): the context, the options, the table, the step.  The solver's half is solver.hip.
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
// environment of a PRODUCT option (read once per context) / of a lab switch (ignored unless the library was built with -DVV_LAB)
static inline const char* opt_env(const char* name) { return getenv(name); }
#ifdef VV_LAB
static inline const char* lab_env(const char* name) { return getenv(name); }
#else
static inline const char* lab_env(const char*) { return nullptr; }
#endif
using namespace vv;

static inline int upd_pending_guard(vv_ctx* c, const char* who) { return vv_upd_pending_guard(c, who); }      // (vv_update_hint, below)
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
static inline int comm_join(vv_ctx* c) { return vv_comm_join(c); }
static inline int reduce_now(vv_ctx* c) { return vv_reduce_now(c); }

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

static void free_batch(vv_ctx* c) {
  dfree(c->idx_dev); dfree(c->rows); dfree(c->H); dfree(c->dYh); dfree(c->dbp); dfree(c->slab_sc); c->slab_sc = nullptr;
  dfree(c->loss_part); dfree(c->viol_part); dfree(c->s_true); dfree(c->s_bogus);
  dfree(c->coeff); dfree(c->slabs); dfree(c->item_w); c->item_w = nullptr;
  if (c->dd_stream) (void)hipStreamSynchronize(c->dd_stream);
  dfree(c->dd_agg); dfree(c->dd_pos); dfree(c->dYu);
  for (int i = 0; i < vv_ctx::kDdAll; ++i) {
    vv_ctx::DdSet& d = c->dd_set[i];
    dfree(d.rows); dfree(d.slot_of); dfree(d.uniq); dfree(d.map); dfree(d.ord); dfree(d.cnt); dfree(d.seg);
    d.rows = d.slot_of = d.uniq = d.map = d.ord = d.cnt = d.seg = nullptr; d.used_seq = 0;
  }
  dfree(c->eval_loss_part); dfree(c->eval_viol_part); c->eval_loss_part = c->eval_viol_part = nullptr;
  c->eval_set_used = false; c->last_fwd_only = false;
  c->dd_rows = nullptr;
  dfree(c->segV); dfree(c->seg_rec); dfree(c->seg_dbp); dfree(c->gg_slots); dfree(c->h16_cnt);
  c->segV = nullptr; c->seg_rec = nullptr; c->seg_dbp = nullptr; c->gg_slots = nullptr; c->gg_nslot = 0; c->h16_cnt = nullptr;
  c->last_h16 = c->last_h16_counted = false;
  c->sg_adj = 0; c->gg_seq0 = 0;
  c->dd_agg = nullptr; c->dd_slot_of = c->dd_uniq = c->dd_map = c->dd_ord = c->dd_cnt = c->dd_seg = c->dd_pos = nullptr;
  c->dYu = nullptr;
  c->idx_dev = c->rows = nullptr; c->H = nullptr; c->dYh = nullptr; c->dbp = nullptr;
  c->loss_part = c->viol_part = c->s_true = c->s_bogus = c->coeff = nullptr; c->slabs = nullptr;
  c->slab_bytes = 0; c->B = c->C = c->Nn = c->R = c->Rp = 0; c->coeff_host.clear();
  grad_discard(c->grad);                      // (a reduction that was still due named the buffers just freed: red_args)
  c->grad_unapplied = false;
}

int vv_destroy(vv_ctx* c) {
  if (!c) return VV_OK;
  (void)hipSetDevice(c->device);
  if (vv::g_ko == &c->ko) vv::g_ko = nullptr;        // (this thread's launcher options pointed into the context)
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm) { vv::comm_destroy(c->comm); c->comm = nullptr; }    // drains the communication stream: before any buffer it uses goes
  vv_ops_release(c);
  free_batch(c);
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
  { const int rcj = comm_join(c); if (rcj) return rcj; }
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
  { const int rcj = comm_join(c); if (rcj) return rcj; }
  HIPCHK(hipStreamSynchronize(c->stream));
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return VV_OK;
}

int vv_synchronize(vv_ctx* c) {
  if (!c) return fail(VV_ERR_ARG, "vv_synchronize: ctx is NULL");
  { const int rcj = comm_join(c); if (rcj) return rcj; }
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
  { const int rcj = comm_join(c); if (rcj) return rcj; }
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
    free_batch(c);
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
  { const int rcj = comm_join(c); if (rcj) return rcj; }
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
  { const int rcg = upd_pending_guard(c, "vv_params_get"); if (rcg) return rcg; }
  if (!c->W) return fail(VV_ERR_STATE, "vv_params_get: no parameters");
  VV_ENTER(c);
  { const int rcj = comm_join(c); if (rcj) return rcj; }
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

// ------------------------------------------------------------------------------- step ---------
extern "C++" int vv_ensure_batch(vv_ctx* c, int B, int C, int Nn) {
  if (B == c->B && C == c->C && Nn == c->Nn && c->H) return VV_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  free_batch(c);
  const int CN = C + Nn;
  const int64_t R64 = (int64_t)B * CN;
  if (R64 > (1ll << 30)) return fail(VV_ERR_ARG, "batch too large");
  c->B = B; c->C = C; c->Nn = Nn; c->R = (int)R64; c->Rp = (int)round_up(R64, R_ALIGN);
  const int D = c->D;
  HIPCHK(hipMalloc(&c->idx_dev, (size_t)c->R * 4));
  HIPCHK(hipMalloc(&c->rows, (size_t)c->Rp * 4));
  HIPCHK(hipMalloc(&c->H, (size_t)c->R * D * 4));
  // + BK rows of slack: the phase-staggered weight-gradient kernel may read one padded K-tile past the last row
  HIPCHK(hipMalloc(&c->dYh, (size_t)(c->Rp + BK) * c->Dp * 2));
  HIPCHK(hipMemset(c->dYh, 0, (size_t)(c->Rp + BK) * c->Dp * 2));     // padding rows / columns stay zero
  HIPCHK(hipMalloc(&c->dbp, (size_t)B * D * 4));
  HIPCHK(hipMalloc(&c->loss_part, (size_t)B * 4));
  HIPCHK(hipMalloc(&c->viol_part, (size_t)B * 4));
  HIPCHK(hipMalloc(&c->s_true, (size_t)B * 4));
  HIPCHK(hipMalloc(&c->s_bogus, (size_t)B * std::max(Nn, 1) * 4));
  HIPCHK(hipMalloc(&c->coeff, (size_t)std::max(C - 1, 1) * 4));
  HIPCHK(hipMalloc(&c->item_w, (size_t)B * 4));
  // split-K so that tiles * S is about one wave of workgroups over the 256 CUs
  const int tiles = (c->Dp / BM) * (c->Fp / BN);
  const int total_steps = c->Rp / BK;
  int S = (256 + tiles - 1) / tiles;
  if (S > total_steps) S = total_steps;
  if (S < 1) S = 1;
  c->S = S; c->kps = (total_steps + S - 1) / S;
  c->slab_bytes = (size_t)S * (size_t)slab_pitch(c->Dp, c->Fp) * 4;
  HIPCHK(hipMalloc(&c->slabs, c->slab_bytes));
  HIPCHK(hipMalloc(&c->slab_sc, (size_t)8 * tiles * sizeof(float)));
  HIPCHK(hipMemset(c->slab_sc, 0, (size_t)8 * tiles * sizeof(float)));
  // de-duplication work arrays
  c->dd_agg_stride = c->R / 1024 + 2;
  HIPCHK(hipMalloc(&c->dd_agg, (size_t)2 * c->dd_agg_stride * sizeof(unsigned long long)));
  HIPCHK(hipMemset(c->dd_agg, 0, (size_t)2 * c->dd_agg_stride * sizeof(unsigned long long)));
  HIPCHK(hipMalloc(&c->eval_loss_part, (size_t)B * 4));
  HIPCHK(hipMalloc(&c->eval_viol_part, (size_t)B * 4));
  for (int i = 0; i < vv_ctx::kDdAll; ++i) {
    vv_ctx::DdSet& d = c->dd_set[i];
    HIPCHK(hipMalloc(&d.rows, (size_t)c->Rp * 4));
    HIPCHK(hipMalloc(&d.slot_of, (size_t)c->Rp * 4));
    HIPCHK(hipMalloc(&d.uniq, (size_t)c->Rp * 4));
    HIPCHK(hipMalloc(&d.map, (size_t)c->Rp * 4));
    HIPCHK(hipMalloc(&d.ord, (size_t)c->Rp * 4));
    HIPCHK(hipMalloc(&d.cnt, (size_t)c->Rp * 4));
    HIPCHK(hipMalloc(&d.seg, (size_t)(c->Rp + 1) * 4));
  }
  HIPCHK(hipMalloc(&c->dd_pos, (size_t)c->Rp * 4));
  HIPCHK(hipMalloc(&c->dYu, (size_t)(c->Rp + BK) * c->Dp * 2));
  HIPCHK(hipMemset(c->dYu, 0, (size_t)(c->Rp + BK) * c->Dp * 2));
  HIPCHK(hipMalloc(&c->segV, (size_t)2 * B * D * 4));
  HIPCHK(hipMalloc(&c->seg_rec, (size_t)c->Rp * sizeof(SegRec)));
  HIPCHK(hipMalloc(&c->seg_dbp, (size_t)SEGB_BLOCKS * D * 4));
  HIPCHK(hipMalloc(&c->h16_cnt, (size_t)2 * SEGB_BLOCKS * sizeof(uint32_t)));
  HIPCHK(hipMemset(c->h16_cnt, 0, (size_t)2 * SEGB_BLOCKS * sizeof(uint32_t)));
  c->gg_nslot = std::max(std::max(B, SEGB_BLOCKS), (c->Rp + 3) / 4);
  HIPCHK(hipMalloc(&c->gg_slots, (size_t)3 * 2 * c->gg_nslot * 4));
  HIPCHK(hipMemset(c->gg_slots, 0, (size_t)3 * 2 * c->gg_nslot * 4));
  c->U_host[0] = c->U_host[2] = 0;        // (the distinct-row hints of the old shape: the training batches' and the forward-only passes')
  return VV_OK;
}

extern "C++" int vv_check_cfg(vv_ctx* c, const vv_step_cfg* cfg) {
  if (!c || !cfg) return fail(VV_ERR_ARG, "NULL ctx / cfg");
  if (!c->table || !c->W) return fail(VV_ERR_STATE, "table and parameters must be set first");
  if (cfg->B < 1) return fail(VV_ERR_ARG, "batch_size must be >= 1 (video_sampled_shots_data_layer.cpp:209)");
  if (cfg->C < 2) return fail(VV_ERR_ARG, "context_size must be >= 2 (video_sampled_shots_data_layer.cpp:207)");
  if (cfg->Nn < 1) return fail(VV_ERR_ARG, "num_negative_samples must be >= 1 for the ranking loss");
  if (cfg->norm != VV_NORM_L1 && cfg->norm != VV_NORM_L2) return fail(VV_ERR_ARG, "Unknown Norm (max_margin_loss_layer.cpp:120)");
  if (cfg->dropout_ratio < 0.f || cfg->dropout_ratio >= 1.f) return fail(VV_ERR_ARG, "dropout_ratio must be in [0,1)");
  if (cfg->reg != VV_REG_L1 && cfg->reg != VV_REG_L2) return fail(VV_ERR_ARG, "Unknown regularization type (solver.cpp:523)");
  if (cfg->solver_type == 4) return fail(VV_ERR_ARG, "SolverType 4 (BVLC Caffe's ADADELTA) is not implemented");
  if (cfg->solver_type < VV_SOLVER_SGD || cfg->solver_type > VV_SOLVER_ADAM) return fail(VV_ERR_ARG, "Unknown SolverType (solver.hpp:141)");
  if (cfg->solver_type == VV_SOLVER_ADAGRAD && cfg->momentum != 0.f) return fail(VV_ERR_ARG, "Momentum cannot be used with AdaGrad. (solver.hpp:121-122)");
  if (cfg->solver_type == VV_SOLVER_RMSPROP) {
    if (cfg->momentum != 0.f) return fail(VV_ERR_ARG, "Momentum cannot be used with RMSProp. (BVLC Caffe sgd_solvers.hpp, RMSPropSolver::constructor_sanity_check)");
    if (!(c->rms_decay >= 0.f && c->rms_decay < 1.f)) return fail(VV_ERR_ARG, "rms_decay should lie between 0 and 1. (BVLC Caffe sgd_solvers.hpp, RMSPropSolver::constructor_sanity_check; vv_solver_ext_set)");
  }
  if (cfg->solver_type == VV_SOLVER_ADAM) {
    if (!(cfg->momentum >= 0.f && cfg->momentum < 1.f)) return fail(VV_ERR_ARG, "Adam: momentum (beta1) must be in [0, 1)");
    if (!(c->momentum2 >= 0.f && c->momentum2 < 1.f)) return fail(VV_ERR_ARG, "Adam: momentum2 (beta2) must be in [0, 1) (vv_solver_ext_set)");
  }
  if (cfg->ip_regularization < 0.f) return fail(VV_ERR_ARG, "ip_regularization must be >= 0");
  return VV_OK;
}

// Index batches reach the GPU through kStage pinned, device-mapped buffers that the step's first kernel reads in place
// (see vv_forward_backward_ring).  Returns the slot to fill; waits until the step that last read it is past its index
// kernels (the forward GEMM stamps seq_host).
static int stage_acquire(vv_ctx* c, size_t bytes, int* slot) {
  if (bytes != c->stage_bytes) {
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < vv_ctx::kStage; ++i) {
      if (c->stage_host[i]) (void)hipHostFree(c->stage_host[i]);
      c->stage_host[i] = c->stage_dev[i] = nullptr; c->stage_seq[i] = 0;
      HIPCHK(hipHostMalloc((void**)&c->stage_host[i], bytes, hipHostMallocMapped));
      HIPCHK(hipHostGetDevicePointer((void**)&c->stage_dev[i], c->stage_host[i], 0));
    }
    c->stage_bytes = bytes;
  }
  const int sl = c->stage_next;
  c->stage_next = (c->stage_next + 1) % vv_ctx::kStage;
  const double tw0 = host_now_ms();
  for (unsigned spins = 0; (int32_t)(__atomic_load_n(c->seq_host, __ATOMIC_ACQUIRE) - c->stage_seq[sl]) < 0; ++spins) {
    if (spins > 4096) { timespec ts = {0, 20000}; nanosleep(&ts, nullptr); }
    if (hipStreamQuery(c->stream) == hipSuccess) break;     // nothing queued any more: every earlier step is done
  }
  c->wait_ms[3] += host_now_ms() - tw0;
  *slot = sl;
  return VV_OK;
}

// The report entry of step `want` in the host-visible ring (vv_internal.h: GMAX_ENTRY_WORDS; reduce_loss writes it): waits until it is there.
// false: the stream ran empty without it (a step whose reduction never ran).  kLag: how many steps behind the host reads -- fixed, so that
// whatever the reports steer (the gradient scale, the f16 rows' fallback) does not depend on host timing and runs stay bit-reproducible.
constexpr int kLag = 4;
static bool report_wait(vv_ctx* c, int32_t want, hipStream_t s) {
  volatile unsigned long long* en = c->gmax_host + GMAX_ENTRY_WORDS * (want & (GMAX_ENTRIES - 1));
  bool have = false;
  const double tw0 = host_now_ms();
  for (unsigned spins = 0; !(have = (int32_t)(uint32_t)__atomic_load_n(en, __ATOMIC_ACQUIRE) == want); ++spins) {
    if (spins > 4096) { timespec ts = {0, 20000}; nanosleep(&ts, nullptr); }
    if (hipStreamQuery(s) == hipSuccess) { have = (int32_t)(uint32_t)__atomic_load_n(en, __ATOMIC_ACQUIRE) == want; break; }
  }
  c->wait_ms[0] += host_now_ms() - tw0;
  return have;
}

// The reduction vv_forward_backward left undone (GradAt::Slabs): run it now, as the plain k_reduce -- somebody reads the
// gradient or the loss before an update.
extern "C++" int vv_reduce_now(vv_ctx* c) {
  ReduceArgs ra = c->red_args;
  switch (c->grad.at) {
    case GradAt::SlabsWUpdated:
      // (vv_loss_get between the backward pass and vv_apply_update of a step announced by vv_update_hint: the loss scalars now, from the
      // partials; the bias update and the bookkeeping stay with vv_apply_update)
      ra.parts = 2; ra.scale_sc = nullptr; ra.gmax_host = nullptr;
      launch_reduce(ra, c->stream);
      break;
    case GradAt::SlabsStale:
      // the fused update consumed the slabs without writing dW out; they are untouched since: reduce them now (dW only --
      // db, the loss and the guard's report were produced by the fused launch)
      ra.parts = 1; ra.scale_sc = nullptr; ra.gmax_host = nullptr;
      launch_reduce(ra, c->stream);
      break;
    case GradAt::Slabs:
      if (c->scale_pending) {
        ra.scale_sc = c->scales; ra.scale_wmax = c->wmax_blocks + c->wmax_cur * WMAX_SLOTS; ra.scale_n = c->wmax_n; ra.scale_prec = c->prec;
        c->scale_pending = false; c->wmax_seed_live = false;
      }
      PROFILED(c, "reduce", launch_reduce(ra, c->stream));
      break;
    default: return VV_OK;           // nothing kept in the slabs
  }
  grad_reduced(c->grad);
  HIPCHK(hipGetLastError());
  return VV_OK;
}

// F-chunks of the overlapped update: n column blocks of W whose widths fall off geometrically (ratio 0.6: e.g. 51 / 31 / 18 %
// of F for three).  The exchange is slower than the forward GEMM consumes W, so the GEMM always ends up waiting for the
// LAST chunk and then still has that chunk's K-tiles to run: a small last chunk shortens that tail, a large first chunk
// keeps the number of collectives (each with its launch latency) down.  Boundaries are even K-tiles (the gate sits in
// front of phase 3 of an even K-tile), at least 4 apart; fills c->chunk_kt[0 .. n], returns n (1 when F is too short).
extern "C++" int vv_chunk_plan(vv_ctx* c) {
  const int nk = c->Fp / BK;
  int n = std::max(1, std::min(c->n_chunks, nk / 8));
  for (;;) {
    double den = 0, r = 1;
    for (int i = 0; i < n; ++i) { den += r; r *= 0.6; }
    c->chunk_kt[0] = 0;
    double acc = 0; r = 1;
    bool ok = true;
    for (int i = 1; i < n; ++i) {
      acc += r; r *= 0.6;
      int kt = (int)(nk * acc / den + 0.5) & ~1;
      if (kt < c->chunk_kt[i - 1] + 4 || kt > nk - 4) ok = false;
      c->chunk_kt[i] = kt;
    }
    c->chunk_kt[n] = nk;
    if (ok || n == 1) return n;
    --n;
  }
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

// The grouping of one batch (k_dd_claim .. k_dd_segstart) into the next of the rotating output sets, on the grouping
// stream; *set_out = the set.  The step that consumes the set binds it and orders its stream behind set.done (fb_impl).
// eval (vv_forward): the set that never rotates (vv_ctx::kDdEval).  Its last reader was the previous forward-only pass, on the step's
// stream: the grouping stream waits for that pass's end event instead of a sequence stamp (a forward-only pass takes no sequence number),
// and the distinct-row count goes to a host word of its own, so the hint the next TRAINING forward GEMM is sized by stays the training batches'.
static int dd_issue(vv_ctx* c, const int32_t* didx, int idx_on_device, int64_t row_limit, int32_t seq, int* set_out, bool eval = false) {
  hipStream_t s = c->stream;
  const int D = c->D;
  {
    // The grouping kernels need only the indices: they run on the context's second stream, so that when the host is a
    // step ahead (the normal case: nothing in the loop waits for the GPU) the grouping of step k+1 executes beside the
    // kernels of step k and the step's own stream merely waits for an event that has long been signalled.  Three sets of
    // output arrays rotate; a set is rewritten only after the step that read it has issued its last reader.
    hipStream_t ds = c->dd_async ? c->dd_stream : s;
    if (c->dd_async && idx_on_device == 1) {
      // the caller's indices may still be in the making on the context's stream: the grouping stream waits for it
      if (!c->ev_idx) HIPCHK(hipEventCreateWithFlags(&c->ev_idx, hipEventDisableTiming));
      HIPCHK(hipEventRecord(c->ev_idx, s));
      HIPCHK(hipStreamWaitEvent(ds, c->ev_idx, 0));
    }
    const int64_t need = c->n_rows + 1 + c->patch_cap;
    if (need > c->dd_key_cap) {
      HIPCHK(hipStreamSynchronize(s));
      HIPCHK(hipStreamSynchronize(c->dd_stream));
      dfree(c->dd_key); c->dd_key = nullptr;
      HIPCHK(hipMalloc(&c->dd_key, (size_t)need * sizeof(unsigned long long)));
      HIPCHK(hipMemsetAsync(c->dd_key, 0, (size_t)need * sizeof(unsigned long long), ds));
      c->dd_key_cap = need;
    }
    if (++c->dd_epoch == 0) {        // epoch tags wrapped: start over with clean tag words
      HIPCHK(hipMemsetAsync(c->dd_key, 0, (size_t)c->dd_key_cap * sizeof(unsigned long long), ds));
      HIPCHK(hipMemsetAsync(c->dd_agg, 0, (size_t)2 * c->dd_agg_stride * sizeof(unsigned long long), ds));
      c->dd_epoch = 1;
    }
    const int si = eval ? vv_ctx::kDdEval : (int)(c->dd_step++ % vv_ctx::kDdSets);
    vv_ctx::DdSet& set = c->dd_set[si];
    *set_out = si;
    if (eval && c->dd_async && c->eval_set_used) HIPCHK(hipStreamWaitEvent(ds, c->ev_eval, 0));
    if (!eval && c->dd_async && set.used_seq) {
      // The set was last read by the step with sequence number used_seq.  The step's stream runs its kernels in order, so
      // once a kernel of ANY later step has stamped its number, every kernel of that step has finished.  The host waits
      // for that stamp (normally long there: it bounds how far the host runs ahead to kDdSets - 1 steps) -- an event
      // recorded per step for the same purpose cost ~6 us of stream time each (a queue barrier packet between two kernels).
      // In steady state this wait is what paces the host, so the grouping it queues next starts right at the stamp and
      // shares the chip with the kernel that wrote it.  Two stamps exist: the forward GEMM's (word 0, written as it starts)
      // and the score kernel's (word 1, i.e. "the forward GEMM has finished").  A/B on one box, 4 x 4000 steps each
      // (profiles/r02_step_ablations.txt): released by the forward GEMM the grouping costs that GEMM 5-6 us (0.085 against
      // 0.080 ms alone: one persistent workgroup per CU, and a CU that also hosts grouping workgroups finishes late) and the
      // step takes 0.2305 ms; released by the score kernel it costs the score and segment kernels 4.5 + 2 us and the step
      // takes 0.2337 ms.  Released after the segment kernel or later it runs into the weight-gradient GEMM, is starved there
      // (80 us instead of 33) and the next step waits for it (0.239-0.253 ms).  Default: the forward GEMM's stamp -- the
      // faster step, at the price of a forward-GEMM duration (and roofline fraction) that includes the co-running kernels.
      // VV_DEDUP_GATE=1 selects the other.
      const int gate_word = c->dd_gate_word;
      const double tw0 = host_now_ms();
      for (unsigned spins = 0; (int32_t)(__atomic_load_n(c->seq_host + gate_word, __ATOMIC_ACQUIRE) - set.used_seq) <= 0; ++spins) {
        if (spins > 4096) { timespec ts = {0, 20000}; nanosleep(&ts, nullptr); }
        if (hipStreamQuery(s) == hipSuccess) break;             // nothing queued any more: every earlier step is done
      }
      c->wait_ms[1] += host_now_ms() - tw0;
    }
    set.used_seq = seq;
    DedupArgs da;
    da.idx = didx; da.rows = set.rows; da.u_host = c->U_host_dev + (eval ? 2 : 0); da.key = c->dd_key; da.agg = c->dd_agg; da.agg_stride = c->dd_agg_stride;
    da.slot_of = set.slot_of; da.uniq_rows = set.uniq; da.map = set.map; da.ord = set.ord; da.cnt = set.cnt;
    da.seg_start = set.seg; da.pos = c->dd_pos; da.info = set.info; da.tickets = set.info + 2;
    {
      // placement of the grouping workgroups beside the forward GEMM (kernels_dedup.hip): only when that GEMM -- sized for
      // the previous step's distinct-row count, as launch_fwd_gemm will size it -- leaves at least 24 CUs idle
      const int lds_kb = c->dd_lds_kb;
      const int hint = *(volatile int32_t*)(c->U_host + (eval ? 2 : 0));
      const long tiles = fwd_gemm_plan(c->R, hint, D, nullptr);
      da.lds_bytes = lds_kb >= 0 ? lds_kb * 1024 : (c->dd_async && hint > 0 && tiles <= c->n_cu - 16 ? 36 * 1024 : 0);
    }
    da.R = c->R; da.Rp = c->Rp; da.zero_row = (int32_t)c->n_rows; da.row_limit = (int32_t)row_limit; da.epoch = c->dd_epoch;
    PROFILED(c, "dedup", (launch_dedup(da, ds), launch_dedup_groups(da, ds)));
    if (c->dd_async) HIPCHK(hipEventRecord(set.done, ds));
  }
  return VV_OK;
}

// idx_on_device: 0 host indices; 1 device indices produced on the context's stream (ordered after everything queued
// there); 2 device indices that are complete already (no ordering needed: the ring's staging slots, static batches)
// vv_update_hint: the parameter matrix of this step was updated inside the weight-gradient GEMM; until vv_apply_update has finished the step
// (bias, loss, the scale bookkeeping) the parameters are half-way -- only vv_apply_update and vv_loss_get may come next
extern "C++" int vv_upd_pending_guard(vv_ctx* c, const char* who) {
  if (!c) return VV_OK;
  switch (grad_guard(c->grad, who)) {
    case GradRefusal::NeverStored:
      return fail(VV_ERR_STATE, "%s: the last step was announced by vv_update_hint and applied its update where the gradient was produced: "
                                "that gradient was never stored (run the step without the hint to read it)", who);
    case GradRefusal::UpdateFirst:
      return fail(VV_ERR_STATE, "%s: the step announced by vv_update_hint has applied its update where the gradient was produced -- call vv_apply_update "
                                "first (the gradient of such a step is not kept; without the hint every call is allowed as before)", who);
    case GradRefusal::No: break;
  }
  return VV_OK;
}

// "One hint covers one step": the vv_forward_backward* entry point that follows vv_update_hint consumes it even when it returns early (bad
// arguments, no batch in the ring, a failed allocation) -- a hint left standing would apply an update, with a stale rate, in some later,
// unrelated backward pass.  fb_impl takes the hint first; this drops what is left when the wrapper never got there.
struct HintScope {
  vv_ctx* c;
  explicit HintScope(vv_ctx* c_) : c(c_) {}
  ~HintScope() { if (c) c->upd_hint = false; }
};

int vv_update_hint(vv_ctx* c, const vv_step_cfg* cfg) {
  int rc = vv_check_cfg(c, cfg);
  if (rc) return rc;
  if (c->bank_count > 0) return VV_OK;       // a cycle of banked gradients is open: the next pass's gradient is kept, nothing is announced
  c->upd_hint = true;
  c->upd_cfg = *cfg;
  c->upd_momentum2 = c->momentum2; c->upd_rms_decay = c->rms_decay; c->upd_clip = c->clip;
  return VV_OK;
}

// The end of a backward pass: the weight-gradient GEMM, and where its gradient goes -- it stays in the slabs (lazy; with vv_update_hint and
// one split of K the GEMM updates W as well), or k_reduce writes it to the gradient buffer, flat, chunk-major or shard-major.  wa and ra
// arrive filled in for the step; the destination is recorded in c->grad.
static int wgrad_to_destination(vv_ctx* c, WgradArgs& wa, ReduceArgs& ra, bool upd_hint) {
  hipStream_t s = c->stream;
  // Data-parallel overlap: the gradient buffer is laid out chunk-major (a few column blocks, each one contiguous
  // all-reduce message) and vv_apply_update runs the update chunk by chunk on the communication stream.
  const int shard_rows = c->comm ? c->D / vv::comm_world(c->comm) : 0;
  const bool sharded = c->comm && c->comm_sharded && c->F % 4 == 0 && c->grads == c->grads_own && !c->grads_exposed &&
                       shard_rows * vv::comm_world(c->comm) == c->D && shard_rows % 4 == 0 && vv::comm_world(c->comm) * (SGD_BLOCKS / vv::comm_world(c->comm)) <= WMAX_SLOTS;
  if (sharded) ra.shard_rows = shard_rows;
  const bool chunked = !sharded && c->comm && c->comm_overlap && c->F % 4 == 0 && c->grads == c->grads_own && !c->grads_exposed;   // (a holder of vv_grads_device's pointer reads the documented flat layout)
  if (chunked) {
    ra.n_chunks = vv_chunk_plan(c);
    for (int i = 0; i <= ra.n_chunks; ++i) ra.chunk_c0[i] = std::min(c->F, c->chunk_kt[i] * BK);
  }
  // Lazy reduction (GradAt::Slabs): with no communicator in the way, dW stays in the slabs until somebody wants it --
  // normally vv_apply_update, which reduces and updates in one launch.  VV_FUSE_UPDATE=0: reduce here, as ever.
  const bool fuse_on = c->fuse_update;
  const bool lazy = fuse_on && !c->comm && !c->grads_exposed && c->grads == c->grads_own && c->F % 4 == 0 && c->S <= 8;
  // the W -> half scale update the previous vv_apply_update left pending rides in this step's reduction launch
  if (!lazy && c->scale_pending) {
    ra.scale_sc = c->scales; ra.scale_wmax = c->wmax_blocks + c->wmax_cur * WMAX_SLOTS; ra.scale_n = c->wmax_n; ra.scale_prec = c->prec;
    c->scale_pending = false; c->wmax_seed_live = false;
  }
  // vv_update_hint + one split of K: the tile in the weight-gradient GEMM's accumulators IS the gradient -- the solver's rule is applied
  // there (WgradUpd) and the 4 D F bytes of dW are neither written nor read back (the shipped configuration: D = F = 4096, 134 MB of the
  // update's 370).  vv_apply_update then runs only the bias / loss workgroups.
  // (Adam keeps two histories: the epilogue declines it, the step takes k_reduce_sgd -- the hint changes nothing, as for several splits.
  // Gradient clipping announced with the hint: the update needs the whole gradient's norm first -- the hint changes nothing either.)
  c->upd_announced = upd_hint;
  c->fb_hinted = upd_hint; c->grad_banked = false;       // (vv_grads_bank: a new gradient, bankable once unless it was announced)
  c->grad_unapplied = true;
  const bool fuse_w = upd_hint && c->wgrad_update && lazy && c->S == 1 && wgrad_can_fuse_update() && !c->fuse_keep_grads &&
                      (c->Dp / BM) * (c->Fp / BN) <= WMAX_SLOTS && c->upd_cfg.solver_type != VV_SOLVER_ADAM && !(c->upd_clip >= 0.f);
  if (fuse_w) {
    WgradUpd& u = wa.upd;
    wa.fuse_upd = 1;
    u.W = c->W; u.hW = c->hW; u.Wh = c->Wh; u.scales = c->scales;
    u.wmax_blocks = c->wmax_blocks + (1 - c->wmax_cur) * WMAX_SLOTS;
    u.wmax_prev = c->wmax_blocks + c->wmax_cur * WMAX_SLOTS; u.wmax_prev_n = c->wmax_n;
    u.recompute_scale = c->scale_pending ? 1 : 0; u.prec = c->prec;
    u.D = c->D; u.F = c->F;
    u.rule = vv_solver_rule(c->upd_cfg, c->upd_momentum2, c->upd_rms_decay);
    u.sg = ra.sg; u.gg = ra.gg; u.ip_scale = ra.ip_scale;
  }
  // f16 split-K partial products (option "slab16"): the phase-staggered kernel with several splits only (one split: the update rides in the
  // epilogue or the slab is the gradient); whoever reduces the slabs -- k_reduce, k_reduce_sgd, now or lazily -- reads the same flag
  if (c->slab16 && !fuse_w && c->S > 1 && c->S <= 8 && c->F % 8 == 0 && wgrad_can_fuse_update()) {
    wa.slab16 = 1; wa.slab_sc = c->slab_sc;
    ra.slab16 = 1; ra.slab_sc = c->slab_sc;
  }
  PROFILED(c, "wgrad_gemm", launch_wgrad_gemm(c->prec, wa, s));     // (the slabs now hold this step's gradient)
  if (lazy) {
    if (fuse_w) {
      HIPCHK(vv_clear_wmax_seed(c, wa.upd.recompute_scale, s));
      c->upd_wgrad_blocks = (c->Dp / BM) * (c->Fp / BN);
    }
    c->red_args = ra;
    HIPCHK(hipGetLastError());
    grad_to_slabs(c->grad, fuse_w);
    return VV_OK;
  }
  const bool chunk0 = chunked && ra.n_chunks > 1 && ra.chunk_c0[1] < c->F;
  if (chunk0) {
    // the first F-chunk is reduced by a launch of its own and an event marks it: the communication stream starts on
    // chunk 0 (all-reduce, SGD) while the other chunks, db and the loss are still being reduced here
    ReduceArgs r0 = ra;
    r0.f_begin = 0; r0.f_count = ra.chunk_c0[1]; r0.parts = 1; r0.gmax_host = nullptr;
    PROFILED(c, "reduce", launch_reduce(r0, s));
    HIPCHK(hipEventRecord(c->ev_chunk0, s));
    ra.scale_sc = nullptr;
    ra.f_begin = ra.chunk_c0[1]; ra.f_count = c->F - ra.f_begin;
    launch_reduce(ra, s);
  } else {
    PROFILED(c, "reduce", launch_reduce(ra, s));
  }
  HIPCHK(hipGetLastError());
  // (the sum over the ranks is due with a communicator -- a one-rank communicator still runs its collective: same code path)
  grad_to_buffer(c->grad, sharded ? GradLayout::Sharded : chunked ? GradLayout::Chunked : GradLayout::Flat, !c->comm, chunk0);
  return VV_OK;
}

// ---- the stages of a pass over one batch.  The training pass (fb_impl) and the forward-only pass (vv_forward) are sequences of these; what
// differs between the two stands at the two call sites.

// Host indices: checked while they are copied into a pinned staging slot that the first kernel reads in place.  The slot is the caller's
// (training slots are released by sequence stamps, evaluation slots by events).
static int stage_indices(vv_ctx* c, const int32_t* idx, int64_t row_limit, int32_t* dst) {
  int bad = -1;
  for (int i = 0; i < c->R; ++i) { const int32_t v = idx[i]; dst[i] = v; if (v < -1 || v >= row_limit) bad = i; }
  if (bad >= 0) return fail(VV_ERR_ARG, "idx[%d] = %d out of range [-1, %lld)", bad, idx[bad], (long long)c->n_rows);
  return VV_OK;
}

// The cfg's host inputs, onto the device on the context's stream: the eltwise coefficients (cached on the device until they change -- the one
// synchronise), the item weights, an explicit dropout mask.  The device copies are the step's own, read by kernels queued in front.
static int stage_cfg_inputs(vv_ctx* c, const vv_step_cfg* cfg) {
  const int B = c->B, C = c->C;
  hipStream_t s = c->stream;
  std::vector<float> coeff(C - 1);
  for (int j = 0; j < C - 1; ++j) coeff[j] = cfg->ctx_coeff ? cfg->ctx_coeff[j] : 1.0f / (C - 1);
  if (coeff != c->coeff_host) {
    HIPCHK(hipMemcpyAsync(c->coeff, coeff.data(), coeff.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    c->coeff_host = coeff;
  }
  if (cfg->item_weight) {
    for (int i = 0; i < B; ++i)
      if (!(cfg->item_weight[i] >= 0.f)) return fail(VV_ERR_ARG, "item_weight[%d] = %g: All weights should be greater than 0 (max_margin_loss_layer.cpp:34)", i, (double)cfg->item_weight[i]);
    HIPCHK(hipMemcpyAsync(c->item_w, cfg->item_weight, (size_t)B * 4, hipMemcpyHostToDevice, s));
  }
  if (cfg->dropout_ratio > 0.f && cfg->dropout_mask) {
    const size_t nb = (size_t)c->R * c->D;
    if (nb > c->mask_bytes) { dfree(c->mask); c->mask = nullptr; HIPCHK(hipMalloc(&c->mask, nb)); c->mask_bytes = nb; }
    HIPCHK(hipMemcpyAsync(c->mask, cfg->dropout_mask, nb, hipMemcpyHostToDevice, s));
  }
  return VV_OK;
}

// The execution of this pass (vv_pass_plan.h), from the context's options and the cfg
static PassPlan plan_pass(const vv_ctx* c, const vv_step_cfg* cfg, bool fwd_only) {
  PassPlanIn in;
  in.dedup = c->dedup; in.seg_bwd = c->seg_bwd; in.drop_dedup = c->drop_dedup; in.h16 = c->h16; in.h16_fallback = c->h16_fallback; in.v16 = c->v16;
  in.ablate = ablate_on(); in.D = c->D; in.C = c->C; in.Nn = c->Nn; in.dropout = cfg->dropout_ratio > 0.f; in.fwd_only = fwd_only;
  return pass_plan(in);
}

// The dropout mask of this pass as a function (vv_internal.h: DropSpec; mode 0 without dropout).  The counter c->iter is read, not advanced:
// vv_apply_update advances it, so a forward-only pass draws the mask the next training step will draw and leaves it to that step.
static DropSpec make_drop_spec(const vv_ctx* c, const vv_step_cfg* cfg) {
  DropSpec dsp;
  if (cfg->dropout_ratio > 0.f) {
    dsp.mode = cfg->dropout_mask ? 2 : 1; dsp.thr = (uint32_t)(cfg->dropout_ratio * 65536.f + 0.5f);
    dsp.s32 = (uint32_t)(mix64(cfg->dropout_seed * 0x9E3779B97F4A7C15ull + c->iter, 0x5eedull) >> 32);
    dsp.scale = 1.f / (1.f - cfg->dropout_ratio);
    dsp.mask = cfg->dropout_mask ? c->mask : nullptr;
    dsp.B = c->B; dsp.CN = c->C + c->Nn; dsp.D = c->D;
  }
  return dsp;
}

// what the accessors of the last forward pass's values read (vv_blobs_get, vv_dedup_stats, vv_h16_stats, option "last_h16")
static void record_plan(vv_ctx* c, const PassPlan& p, const DropSpec& dsp) {
  c->last_drop = p.drop_rides_dd ? dsp : DropSpec(); c->last_dedup = p.dd; c->last_h16 = p.h16;
}

// the grouping set this pass reads (dd_issue)
static void bind_dd_set(vv_ctx* c, const vv_ctx::DdSet& set) {
  c->dd_rows = set.rows; c->dd_slot_of = set.slot_of; c->dd_uniq = set.uniq; c->dd_map = set.map; c->dd_ord = set.ord;
  c->dd_cnt = set.cnt; c->dd_seg = set.seg; c->dd_info = set.info;
}

// The forward GEMM of a pass: the batch's rows (distinct rows when de-duplicated, R_hint of them expected) through pv's parameters into ip2.
// A training step adds its sequence stamp and, under an overlapped update, the gate.
static FwdArgs fwd_args(const vv_ctx* c, const vv_step_cfg* cfg, const PassPlan& p, const ParamView& pv, int R_hint) {
  FwdArgs fa;
  fa.table = c->table; fa.rows = p.dd ? c->dd_uniq : c->rows; fa.Wh = pv.Wh; fa.bias = pv.b; fa.scales = pv.scales;
  fa.H = c->H; fa.R = c->R; fa.D = c->D; fa.Fp = c->Fp; fa.relu = 1; fa.zero_row = (int32_t)c->n_rows;
  fa.n_dev = p.dd ? c->dd_info : nullptr; fa.R_hint = p.dd ? R_hint : 0; fa.h16 = p.h16 ? 1 : 0;
  fa.drop_ratio = p.drop_rides_dd ? 0.f : cfg->dropout_ratio;      // (de-duplicated: H holds the shared pre-dropout rows, the instances mask them)
  fa.mask = (!p.drop_rides_dd && cfg->dropout_ratio > 0.f && cfg->dropout_mask) ? c->mask : nullptr;
  fa.drop_seed = cfg->dropout_seed * 0x9E3779B97F4A7C15ull + c->iter;
  fa.B = c->B; fa.CN = c->C + c->Nn;
  return fa;
}

// the loss terms the gradient is normalised by: the caller's count over all ranks, or this batch's own B Nn
static inline int64_t global_count(const vv_ctx* c, const vv_step_cfg* cfg) { return cfg->global_count > 0 ? cfg->global_count : (int64_t)c->B * c->Nn; }

// The score kernels' arguments that every pass fills alike.  The caller adds where the gradient and the loss partials go (dYh, dbp, loss_part,
// viol_part), the gradient scale sg, and what only one of the passes has: the stamp and v16 (training), fwd_only.
static ScoreArgs score_args(const vv_ctx* c, const vv_step_cfg* cfg, const PassPlan& p, const DropSpec& dsp) {
  ScoreArgs sa{};
  sa.H = c->H; sa.s_true = c->s_true; sa.s_bogus = c->s_bogus; sa.coeff = c->coeff;
  sa.B = c->B; sa.C = c->C; sa.Nn = c->Nn; sa.D = c->D; sa.Dp = c->Dp;
  sa.margin = cfg->margin; sa.norm = cfg->norm; sa.grad_scale = cfg->loss_weight / (float)global_count(c, cfg);
  sa.drop_scale = cfg->dropout_ratio > 0.f ? 1.f / (1.f - cfg->dropout_ratio) : 1.f;
  sa.map = p.dd ? c->dd_map : nullptr; sa.seg_start = p.dd ? c->dd_seg : nullptr; sa.ord = p.dd ? c->dd_ord : nullptr;
  sa.item_w = cfg->item_weight ? c->item_w : nullptr;
  if (p.drop_rides_dd) sa.drop = dsp;
  sa.h16 = p.h16 ? 1 : 0;
  return sa;
}

// ---- what only a training step does: its stream behind its grouping (DdSet::done).
// The grouping takes ~30 us on an idle second stream and the host is normally several steps ahead of the GPU: it
// can afford to watch the event for a moment.  Once the event has fired nothing needs to be put into the step's
// stream at all (a wait packet in front of the forward GEMM costs ~6 us of stream time even when already satisfied);
// otherwise the stream waits as usual.
static int dd_wait(vv_ctx* c, vv_ctx::DdSet& set, hipStream_t s) {
  bool fired = hipEventQuery(set.done) == hipSuccess;
  // (an idle step stream -- the first step after a synchronisation -- means a grouping just queued cannot have run yet:
  // watching it would hold the host for its whole 40 us while the GPU then waits for the step's launches; queue the wait)
  if (!fired && c->dd_spin_us > 0 && hipStreamQuery(s) != hipSuccess) {
    const double t0 = host_now_ms();
    do { fired = hipEventQuery(set.done) == hipSuccess; } while (!fired && (host_now_ms() - t0) * 1e3 < c->dd_spin_us);
    c->wait_ms[2] += host_now_ms() - t0;
  }
  if (!fired) HIPCHK(hipStreamWaitEvent(s, set.done, 0));
  return VV_OK;
}

// The f16 rows' range loss (option "h16_guard"): a step that stored f16 rows had them counted (k_seg_bwd_cnt), its counts ride in its report
// entry, and the entry of step seq - kLag is read HERE, at a fixed lag like the gradient scale's, so that whatever it steers -- value 2: this
// and every later step store fp32 rows, exactly the execution of h16 = 0, until the caller sets h16 again -- does not depend on host timing.
// Up to kLag steps have trained on the flagged rows by then: the price of never stalling a host that runs ahead; it is reported.
// Runs before the step is planned: the plan reads the fallback this may switch.
static void h16_guard_read(vv_ctx* c, int32_t seq, hipStream_t s) {
  if (c->h16_guard >= 1 && c->h16_counted[(seq - kLag) & (GMAX_ENTRIES - 1)] == seq - kLag) {
    const int32_t want = seq - kLag;
    if (report_wait(c, want, s)) {
      const volatile unsigned long long* en = c->gmax_host + GMAX_ENTRY_WORDS * (want & (GMAX_ENTRIES - 1));
      const long long sat = (long long)en[2], faint = (long long)en[3];
      if (sat | faint) {
        ++c->h16_flagged_steps;
        if (c->h16_first_flagged < 0) c->h16_first_flagged = want - 1;      // (steps count from 0, sequence numbers from 1)
        const bool sw = c->h16_guard == 2 && !c->h16_fallback && want > c->h16_arm_seq;
        if (sw) c->h16_fallback = true;
        if (sw || c->h16_flag_step < 0) { c->h16_flag_step = want - 1; c->h16_flag_sat = sat; c->h16_flag_faint = faint; }
      }
    }
    c->h16_counted[(seq - kLag) & (GMAX_ENTRIES - 1)] = INT32_MIN;
  }
}

// Data-parallel overlap: the previous step's update is still arriving on the communication stream, F-chunk by
// F-chunk.  The forward GEMM starts anyway and waits per chunk inside the kernel -- provided its persistent
// workgroups leave compute units free for the update's own kernels (all-reduce, SGD: they must be able to run
// BESIDE the waiting GEMM, or nothing would ever release it); otherwise the stream joins here, as without overlap.
static int fwd_gate_or_join(vv_ctx* c, FwdArgs& fa, bool dd) {
  const long tiles = fwd_gemm_plan(c->R, dd ? fa.R_hint : 0, c->D, nullptr);
  const bool no_gate = !c->comm_gate;
  if (!no_gate && !ablate_on() && fwd_gemm_can_gate(fa) && (!dd || fa.R_hint > 0) && tiles <= c->n_cu - 16) {
    fa.gate = c->w_gate; fa.gate_seq = c->upd_seq; fa.gate_err = c->gate_err_dev;
    if (c->grad.buf.layout == GradLayout::Sharded) { fa.gate_n = 1; fa.gate_kt[0] = 0; fa.gate_kt[1] = c->Fp / BK; }        // the sharded update publishes once
    else { fa.gate_n = vv_chunk_plan(c); for (int i = 0; i <= fa.gate_n; ++i) fa.gate_kt[i] = c->chunk_kt[i]; }
    // whatever follows the forward GEMM on this stream follows every PUBLISHED store of the update; its plain stores (W, the history) only
    // behind the event: vv_comm_join for whoever reads those
    upd_gated(c->upd_sync);
    return VV_OK;
  }
  return comm_join(c);
}

// The half-precision gradient scale's adjustment c->sg_adj, for a step whose loss count has exponent e.  The segment-wise backward settles the scale on the device, from a bound on the step's own gradients, before it
// rounds anything (GuardArgs::proactive).  On the other paths the host's scale follows the data: every step reports its
// largest |dY| (k_reduce, a host-visible ring); when the max of step seq - 4 -- a FIXED lag, so that the scale sequence
// does not depend on host timing and runs stay bit-reproducible -- lies outside [2^4, 2^13) in the current scaled units,
// the scale moves so that it lies in [2^9, 2^10).  That only keeps the guard's repeats rare: a value past f16's range never
// reaches the weight-gradient GEMM either way (GradGuard).
static int grad_scale_steer(vv_ctx* c, int32_t seq, int e, hipStream_t s) {
  if (c->prec == VV_PREC_F16) {
    if (c->gg_seq0 == 0) c->gg_seq0 = seq;
    if (seq - c->gg_seq0 >= kLag) {
      const int32_t want = seq - kLag;
      volatile unsigned long long* en = c->gmax_host + GMAX_ENTRY_WORDS * (want & (GMAX_ENTRIES - 1));
      const bool have = report_wait(c, want, s);
      if (c->trace_waits && ++c->wait_calls % 100 == 0) {
        fprintf(stderr, "[vv waits] per step over the last 100: gradient-scale report %.3f, grouping-set gate %.3f, grouping event %.3f, staging slot %.3f ms\n",
                c->wait_ms[0] / 100, c->wait_ms[1] / 100, c->wait_ms[2] / 100, c->wait_ms[3] / 100);
        c->wait_ms[0] = c->wait_ms[1] = c->wait_ms[2] = c->wait_ms[3] = 0;
      }
      if (have) {
        const uint32_t bits = (uint32_t)(en[0] >> 32), gbits = (uint32_t)(en[1] >> 32);
        float gmax, gbound; memcpy(&gmax, &bits, 4); memcpy(&gbound, &gbits, 4);
        const uint32_t rep = (uint32_t)en[1];
        if (rep & (1u << 30)) return fail(VV_ERR_STATE, "internal error: a 16-bit gradient value passed f16's range in step %d although the "
                                                        "gradient-scale guard was active (GradGuard)", (int)want);
        if (rep & (1u << 16)) ++c->gg_repeats;
        if (gbound > 0.f) {
          // segment-wise path: nothing to steer -- k_seg_bwd settles its scale on the device from the step's own bound
        } else if (gmax > 0.f && std::isfinite(gmax)) {
          int eu; (void)frexpf(gmax, &eu);
          const int ex = eu + e + c->sg_adj;            // exponent of the max in the current scaled units
          if (ex > 13 || ex < 5) c->sg_adj += 10 - ex;
        }
      }
    }
    c->sg_adj = std::max(-100 - e, std::min(100 - e, c->sg_adj));
  }
  return VV_OK;
}

static int fb_impl(vv_ctx* c, const vv_step_cfg* cfg, const int32_t* idx, int idx_on_device, int64_t row_limit, int32_t seq = 0) {
  // ---- guards
  { const int rcg = upd_pending_guard(c, "vv_forward_backward"); if (rcg) return rcg; }
  const bool upd_hint = c && c->upd_hint;       // (consumed by this call whatever path it takes)
  if (c) c->upd_hint = false;
  if (c && c->ema_in_use) return fail(VV_ERR_STATE, "vv_forward_backward: %s", kEmaInUse);
  int rc = vv_check_cfg(c, cfg);
  if (rc) return rc;
  if (!idx) return fail(VV_ERR_ARG, "vv_forward_backward: idx is NULL");
  VV_ENTER(c);
  // (an overlapped update of the previous step may still be arriving: see the forward GEMM below)
  if (c->upd_sync == UpdSync::InFlight && (cfg->B != c->B || cfg->C != c->C || cfg->Nn != c->Nn || !c->H) && (rc = comm_join(c))) return rc;
  if ((rc = vv_ensure_batch(c, cfg->B, cfg->C, cfg->Nn))) return rc;
  const int B = c->B, D = c->D;
  hipStream_t s = c->stream;

  // ---- stage inputs: the indices (every step has a sequence number; its forward GEMM stamps it into host-visible memory), the cfg's host arrays
  const int32_t* didx = idx;
  if (!idx_on_device) {
    int sl = 0;
    if ((rc = stage_acquire(c, (size_t)c->R * 4, &sl))) return rc;
    if ((rc = stage_indices(c, idx, row_limit, c->stage_host[sl]))) return rc;
    if (!seq) seq = ++c->step_seq;
    c->stage_seq[sl] = seq;
    didx = c->stage_dev[sl];
  }
  if (!seq) seq = ++c->step_seq;
  if ((rc = stage_cfg_inputs(c, cfg))) return rc;

  // ---- plan (behind the f16 rows' lagged report: it may switch this very step to fp32 rows)
  h16_guard_read(c, seq, s);
  const PassPlan p = plan_pass(c, cfg, false);
  const DropSpec dsp = make_drop_spec(c, cfg);
  record_plan(c, p, dsp); c->last_fwd_only = false;
  const bool h16_count = c->last_h16_counted = p.h16 && c->h16_guard >= 1;
  if (h16_count) c->h16_counted[seq & (GMAX_ENTRIES - 1)] = seq;

  // ---- group: into the next of the rotating sets, stamped with this step's number; the host watches the event for a moment
  if (!p.dd) launch_map_rows(didx, c->rows, c->R, c->Rp, (int32_t)c->n_rows, (int32_t)row_limit, s);
  if (p.dd) {
    int si = 0;
    if ((rc = dd_issue(c, didx, idx_on_device, row_limit, seq, &si))) return rc;
    vv_ctx::DdSet& set = c->dd_set[si];
    set.used_seq = seq;
    bind_dd_set(c, set);
    if (c->dd_async && (rc = dd_wait(c, set, s))) return rc;
  }

  // ---- forward: the training parameters, the training batches' distinct-row hint, the sequence stamp; gated on an overlapped update or joined
  FwdArgs fa = fwd_args(c, cfg, p, ParamView{c->Wh, c->b, c->scales}, *(volatile int32_t*)c->U_host);
  fa.seq_host = c->seq_host_dev; fa.seq = seq;
  if (c->upd_sync == UpdSync::InFlight && (rc = fwd_gate_or_join(c, fa, p.dd))) return rc;
  PROFILED(c, "fwd_gemm", launch_fwd_gemm(c->prec, fa, s));

  // ---- scale.  half-precision gradient scale: a power of two near the loss count keeps dY*sg around 1
  const int64_t count = (int64_t)B * c->Nn;
  int e; frexpf((float)global_count(c, cfg), &e);
  if ((rc = grad_scale_steer(c, seq, e, s))) return rc;
  c->sg = c->prec == VV_PREC_F16 ? ldexpf(1.f, e + c->sg_adj) : 1.f;
  c->last_loss_weight = cfg->loss_weight;

  // ---- score: the gradient destinations, the scale, the stamp that releases the host to queue a later step's grouping
  ScoreArgs sa = score_args(c, cfg, p, dsp);
  sa.dYh = c->dYh; sa.dbp = c->dbp; sa.loss_part = c->loss_part; sa.viol_part = c->viol_part; sa.sg = c->sg;
  sa.gate_host = c->seq_host_dev + 1; sa.gate_seq = seq;
  sa.v16 = p.v16 ? 1 : 0;
  c->last_seg_bwd = p.seg; c->last_score = sa;

  // ---- guard rounds: the score kernels and the backward to per-row gradients
  // f16 gradient-scale guard (vv_internal.h: GradGuard): the kernels that round gradients to 16 bits are launched once as
  // usual (round 0) and once more per guard round as conditional repeats -- near-empty launches unless the round before
  // reported a value past f16's range.  Rounds: 1 where one kernel rounds (per-instance rows, or the segment sums); 2 for
  // rows + their sums (k_segsum): sums of clipped rows say nothing about the true sums, which the second round sees.
  GuardArgs gd;
  if (c->prec == VV_PREC_F16) { gd.gg = c->gg; gd.slots = c->gg_slots; gd.nslot = c->gg_nslot; gd.seq = seq; }
  c->gg_last_seq = gd.gg ? seq : 0;
  // (the segment-wise backward needs no repeat at all: its score kernel bounds every instance's gradient and k_seg_bwd
  // settles the scale before it rounds anything -- GuardArgs::proactive)
  const bool proactive_on = c->guard_proactive;   // (lab) false: the repeat form on this path too (A/B)
  const bool proactive = p.seg && proactive_on;
  const int n_rounds = c->prec != VV_PREC_F16 ? 0 : (proactive ? 0 : (p.dd && !p.seg ? 2 : 1));
  c->gg_last_rounds = n_rounds;
  gd.n_of[0] = p.seg ? 0 : B;
  gd.n_of[1] = p.seg ? SEGB_BLOCKS : (p.dd ? (c->Rp + 3) / 4 : 0);
  SegBwdArgs ba;
  SegsumArgs ga;
  if (p.seg) {
    sa.V = c->segV; sa.rec = c->seg_rec;
#ifdef VV_LAB
    if (const char* v = lab_env("VV_LAB_SCORE_HACK")) sa.lab_hack = atoi(v);
    if (lab_env("VV_LAB_SCORE_TS")) {
      // (lab) k_score_fwd's phase stamps: one buffer, every step overwrites it; tools/lab/score_ts.py reads it through vv_lab_score_ts
      static thread_local uint32_t* ts_buf = nullptr;
      if (!ts_buf) { HIPCHK(hipMalloc(&ts_buf, (size_t)65536 * 16 * 4)); HIPCHK(hipMemset(ts_buf, 0, (size_t)65536 * 16 * 4)); }
      sa.lab_ts = ts_buf; c->lab_score_ts = ts_buf;
    }
#endif
    if (gd.gg && proactive) { sa.bound_out = c->gg_bound; sa.bound_seq = seq; }
    ba.H = c->H; ba.V = c->segV; ba.rec = c->seg_rec; ba.seg_start = c->dd_seg; ba.info = c->dd_info; ba.dYu = c->dYu;
    ba.dbp = c->seg_dbp; ba.Rp = c->Rp; ba.D = D; ba.Dp = c->Dp; ba.inv_sg = 1.f / c->sg; ba.h16 = p.h16 ? 1 : 0; ba.v16 = p.v16 ? 1 : 0;
    if (h16_count) ba.h16_cnt = c->h16_cnt;
    if (p.drop_on) ba.drop = dsp;
  } else if (p.dd) {
    ga.dYh = c->dYh; ga.seg_start = c->dd_seg; ga.info = c->dd_info; ga.dYu = c->dYu; ga.Rp = c->Rp; ga.Dp = c->Dp;
  }
  for (int round = 0; round <= n_rounds; ++round) {
    gd.round = round; gd.final_round = round == n_rounds;
    if (p.seg) {
      if (round == 0) PROFILED(c, "score_loss", launch_score_fwd(sa, s));
      ba.guard = gd; ba.guard.producer = 1; ba.guard.last = 1;
      if (gd.gg && proactive) { ba.guard.proactive = 1; ba.guard.bound = c->gg_bound; ba.guard.cnt_max = c->dd_info + 1; }
      if (round == 0) PROFILED(c, "segsum", launch_seg_bwd(c->prec, ba, s));
      else PROFILED(c, "guard", launch_seg_bwd(c->prec, ba, s));
    } else {
      sa.guard = gd; sa.guard.producer = 0; sa.guard.last = p.dd ? 0 : 1;
      if (round == 0) PROFILED(c, "score_loss", launch_score_loss(c->prec, sa, s));
      else if (!p.dd) PROFILED(c, "guard", launch_score_loss(c->prec, sa, s));
      else launch_score_loss(c->prec, sa, s);
      if (p.dd) {
        ga.guard = gd; ga.guard.producer = 1; ga.guard.last = 1;
        if (round == 0) PROFILED(c, "segsum", launch_segsum(c->prec, ga, s));
        else PROFILED(c, "guard", launch_segsum(c->prec, ga, s));
      }
    }
  }

  // ---- weight gradient: its arguments and the reduction's, then wherever the gradient goes
  WgradArgs wa;
  wa.dYh = p.dd ? c->dYu : c->dYh; wa.table = c->table; wa.rows = p.dd ? c->dd_uniq : c->rows; wa.slabs = c->slabs;
  wa.Rp = c->Rp; wa.Dp = c->Dp; wa.Fp = c->Fp; wa.S = c->S; wa.ksteps_per_split = c->kps;
  wa.n_dev = p.dd ? c->dd_info : nullptr; wa.zero_row = (int32_t)c->n_rows;
  {
    const int64_t t_rows = c->n_rows + 1 + c->patch_cap;      // every row a K-tile can name: the table, its zero row, the scratch rows behind it
    wa.lean = c->ko.wgrad_lean && t_rows < (1ll << 24) && (int64_t)c->Fp * 2 < (1ll << 24) && t_rows * c->Fp * 2 + 8192 < (1ll << 32);
  }
  ReduceArgs ra;
  ra.slabs = c->slabs; ra.S = c->S; ra.Dp = c->Dp; ra.Fp = c->Fp; ra.dbp = p.seg ? c->seg_dbp : c->dbp; ra.B = B;
  ra.db_rows = p.seg ? SEGB_BLOCKS : 0;
  ra.scales = c->scales; ra.sg = c->sg; ra.grads = c->grads; ra.D = D; ra.F = c->F;
  if (gd.gg) {
    ra.gg = c->gg; ra.gmax_slots = c->gg_slots; ra.gmax_n0 = gd.n_of[0]; ra.gmax_n1 = gd.n_of[1]; ra.gmax_stride = c->gg_nslot;
    ra.gmax_host = c->gmax_host_dev; ra.seq = seq; ra.guard_last_round = n_rounds;
    if (proactive) { ra.gbound = c->gg_bound; ra.gcnt = c->dd_info + 1; }
  }
  if (h16_count) {       // (bf16 operands publish a report entry for these steps only: the rows of H are f16 there too)
    ra.gmax_host = c->gmax_host_dev; ra.seq = seq;
    ra.h16_cnt = c->h16_cnt; ra.h16_cnt_n = SEGB_BLOCKS;
  }
  ra.ip_scale = cfg->ip_regularization > 0.f ? 1.f + cfg->ip_regularization * 0.5f : 1.f;     // inner_product_layer.cpp:80-90
  ra.loss_part = c->loss_part; ra.viol_part = c->viol_part; ra.loss_scale = cfg->loss_weight / (float)count; ra.loss_out = c->loss2;

  return wgrad_to_destination(c, wa, ra, upd_hint);
}

int vv_forward_backward(vv_ctx* c, const vv_step_cfg* cfg, const int32_t* idx, int idx_on_device) {
  HintScope hint_scope(c);
  if (idx_on_device < 0 || idx_on_device > 2) return fail(VV_ERR_ARG, "vv_forward_backward: idx_on_device must be 0, 1 or 2");
  return fb_impl(c, cfg, idx, idx_on_device, c ? c->n_rows : 0);
}

// BasePrefetchingDataLayer::Forward_gpu (base_data_layer.cu:7-21) joins the prefetch thread and copies the batch to the
// device; here the batch is 4*B*(C+Nn) bytes of indices out of the sampler's ring.  They are copied into one of kStage
// pinned buffers that the GPU reads IN PLACE (the first kernel of the step, k_dd_claim / k_map_rows, reads every index
// exactly once, coalesced, straight over PCIe): no copy engine, no second stream, no event.  (An asynchronous H2D copy
// per step was measured first: ~25 us per step of queue switching between the copy and the kernels, and a one-off 6-7 ms
// host stall inside hipMemcpyAsync after a handful of copies.)  A slot is reused only after the forward GEMM of the
// step that read it has stamped its sequence number into host-visible memory.
int vv_forward_backward_ring(vv_ctx* c, const vv_step_cfg* cfg, vv_batch_ring* ring, int32_t consumer, int32_t item_begin,
                             int32_t* label_out, double timeout_s) {
  HintScope hint_scope(c);
  int rc = vv_check_cfg(c, cfg);
  if (rc) return rc;
  if (c->ema_in_use) return fail(VV_ERR_STATE, "vv_forward_backward_ring: %s", kEmaInUse);      // (before a batch is taken from the ring)
  if (!ring) return fail(VV_ERR_ARG, "vv_forward_backward_ring: ring is NULL");
  int32_t rb = 0, rcn = 0;
  if (vv_batch_ring_info(ring, &rb, &rcn, nullptr, nullptr)) return fail(VV_ERR_ARG, "vv_forward_backward_ring: bad ring");
  if (rcn != cfg->C + cfg->Nn || item_begin < 0 || item_begin + cfg->B > rb)
    return fail(VV_ERR_ARG, "vv_forward_backward_ring: the ring holds batches of %d x %d slots; asked for items [%d, %d) x %d",
                rb, rcn, item_begin, item_begin + cfg->B, cfg->C + cfg->Nn);
  VV_ENTER(c);
  const size_t bytes = (size_t)cfg->B * rcn * sizeof(int32_t);
  int sl = 0;
  const double t0 = c->trace_host_ms >= 0 ? host_now_ms() : 0.0;
  if ((rc = stage_acquire(c, bytes, &sl))) return rc;
  const double t1 = c->trace_host_ms >= 0 ? host_now_ms() : 0.0;
  if (vv_batch_ring_next(ring, consumer, item_begin, cfg->B, c->stage_host[sl], label_out, timeout_s))
    return fail(VV_ERR_STATE, "vv_forward_backward_ring: no batch (the sampler's prefetch stopped, or timeout)");
  if (c->trace_host_ms >= 0) {
    const double t2 = host_now_ms();
    if (t2 - t0 > c->trace_host_ms)
      fprintf(stderr, "[vv host] ring stage: slot wait %.3f, batch wait + copy %.3f ms (call %llu)\n", t1 - t0, t2 - t1, (unsigned long long)c->iter);
  }
  const int32_t seq = ++c->step_seq;
  c->stage_seq[sl] = seq;
  // (Issuing the grouping of the NEXT batch from here, a whole step ahead, was built and measured: 0.2345 against 0.2334 ms
  // per step over 20-step timed regions, two runs each -- the host is ahead of the GPU anyway, and the first step after a
  // synchronisation does not wait for its grouping in any noticeable way.  Taken out again.)
  return fb_impl(c, cfg, c->stage_dev[sl], 2, c->n_rows, seq);
}

// Quirk Q1 (video_sampled_shots_data_layer.cpp:492): a same-video negative is copied WITHOUT its
// last feature, which keeps whatever the prefetch slot held before.  Such a slot is described by
// (idx = row of features 0..F-2, last_src = row of feature F-1, -1 = zero).  Each one is
// materialised as a scratch row behind the table and the batch then points at the scratch row.
// scratch rows behind the table's zero row (quirk-Q1 composites, TEST-branch means)
static int ensure_scratch_rows(vv_ctx* c, int64_t need) {
  if (need <= c->patch_cap) return VV_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  const int64_t cap = std::max<int64_t>(2 * need, 1024);
  uint16_t* nt = nullptr;
  const size_t old_bytes = (size_t)(c->n_rows + 1) * c->Fp * 2;
  HIPCHK(hipMalloc(&nt, (size_t)(c->n_rows + 1 + cap) * c->Fp * 2));
  HIPCHK(hipMemcpy(nt, c->table, old_bytes, hipMemcpyDeviceToDevice));
  dfree(c->table); c->table = nt; c->patch_cap = cap;
  return VV_OK;
}

int vv_forward_backward_q1(vv_ctx* c, const vv_step_cfg* cfg, const int32_t* idx, const int32_t* last_src) {
  HintScope hint_scope(c);
  int rc = vv_check_cfg(c, cfg);
  if (rc) return rc;
  if (c->ema_in_use) return fail(VV_ERR_STATE, "vv_forward_backward_q1: %s", kEmaInUse);
  if (!idx || !last_src) return fail(VV_ERR_ARG, "vv_forward_backward_q1: NULL index array");
  VV_ENTER(c);
  const int64_t R = (int64_t)cfg->B * (cfg->C + cfg->Nn);
  // The patched indices AND the composite rows' descriptors travel in one pinned, device-mapped staging slot that the kernels read
  // in place (as vv_forward_backward_ring's indices do): no host-side copy to wait for.  (Round 3 copied the descriptors from a
  // host temporary and synchronised the stream on EVERY step: the device idled ~30 us of the shipped configuration's 0.29 ms.)
  int sl = 0;
  if ((rc = stage_acquire(c, (size_t)R * 12, &sl))) return rc;          // R indices + at most R descriptors of two words
  int32_t* dst = c->stage_host[sl];
  int32_t* desc = dst + R;
  int64_t P = 0;
  for (int64_t i = 0; i < R; ++i) {
    if (idx[i] < -1 || idx[i] >= c->n_rows || last_src[i] < -1 || last_src[i] >= c->n_rows)
      return fail(VV_ERR_ARG, "index %lld out of range", (long long)i);
    int32_t v = idx[i];
    if (idx[i] != last_src[i] && idx[i] >= 0) {
      v = (int32_t)(c->n_rows + 1 + P);
      desc[2 * P] = idx[i]; desc[2 * P + 1] = last_src[i];
      ++P;
    }
    dst[i] = v;
  }
  if (P > 0 && (rc = ensure_scratch_rows(c, P))) return rc;
  const int32_t seq = ++c->step_seq;
  c->stage_seq[sl] = seq;                                               // the slot is free again when this step's forward GEMM has started
  if (P > 0) launch_patch_rows(c->table, c->stage_dev[sl] + R, P, c->n_rows + 1, c->F, c->Fp, c->stream);
  return fb_impl(c, cfg, c->stage_dev[sl], 2, c->n_rows + 1 + P, seq);
}

// ------------------------------------------------------------------------------- forward only --
// A pinned, device-mapped staging buffer for a forward-only pass's host indices.  Two rotate, each with the event of the pass that last
// read it: the host waits only when it is two evaluation passes ahead of the GPU.  (The training slots of stage_acquire are released by
// the sequence stamps of training steps; a forward-only pass takes no sequence number.)
static int eval_stage_acquire(vv_ctx* c, size_t bytes, int* slot) {
  if (bytes != c->eval_stage_bytes) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->dd_stream) HIPCHK(hipStreamSynchronize(c->dd_stream));
    for (int i = 0; i < vv_ctx::kEvalStage; ++i) {
      if (c->eval_stage_host[i]) (void)hipHostFree(c->eval_stage_host[i]);
      c->eval_stage_host[i] = c->eval_stage_dev[i] = nullptr; c->eval_stage_busy[i] = false;
      HIPCHK(hipHostMalloc((void**)&c->eval_stage_host[i], bytes, hipHostMallocMapped));
      HIPCHK(hipHostGetDevicePointer((void**)&c->eval_stage_dev[i], c->eval_stage_host[i], 0));
      if (!c->eval_stage_done[i]) HIPCHK(hipEventCreateWithFlags(&c->eval_stage_done[i], hipEventDisableTiming));
    }
    c->eval_stage_bytes = bytes;
  }
  const int sl = c->eval_stage_next;
  c->eval_stage_next = (sl + 1) % vv_ctx::kEvalStage;
  if (c->eval_stage_busy[sl]) { HIPCHK(hipEventSynchronize(c->eval_stage_done[sl])); c->eval_stage_busy[sl] = false; }
  *slot = sl;
  return VV_OK;
}

// Net::Forward / Net::ForwardPrefilled under Caffe::set_phase(Caffe::TEST) (include/caffe/net.hpp, src/caffe/net.cpp), one of the test_iter
// passes of Solver::Test (solver.cpp:251-317): the stages of fb_impl's forward half under the same plan -- the same grouping kernels, the same
// forward GEMM launch, the same score form -- with the forward-only instantiations of the score kernels and a loss reduction of its own.  What a training step
// owns is read, never written: the gradient's place (c->grad, the slabs, dbp, the gradient buffer, the bank), the step's pending loss and
// violation partials, the sequence numbers with the two report rings behind them (gradient scale, f16 rows), c->sg, Adam's t, the
// dropout counter c->iter, the clipping and accumulation records, the rotating grouping sets and their distinct-row hint.
int vv_forward(vv_ctx* c, const vv_step_cfg* cfg, const int32_t* idx, int idx_on_device) {
  if (idx_on_device < 0 || idx_on_device > 2) return fail(VV_ERR_ARG, "vv_forward: idx_on_device must be 0, 1 or 2");
  // (between a hinted vv_forward_backward* and its vv_apply_update the parameters are half-way: "another forward pass" is refused)
  { const int rcg = upd_pending_guard(c, "vv_forward"); if (rcg) return rcg; }
  if (c && c->upd_announced && grad_exists(c->grad))      // (... whether or not the announced update could ride in the weight-gradient GEMM: one rule for every shape)
    return fail(VV_ERR_STATE, "vv_forward: the last backward pass was announced by vv_update_hint and its vv_apply_update has not run -- call vv_apply_update first");
  int rc = vv_check_cfg(c, cfg);
  if (rc) return rc;
  if (!idx) return fail(VV_ERR_ARG, "vv_forward: idx is NULL");
  VV_ENTER(c);
  const bool reshape = cfg->B != c->B || cfg->C != c->C || cfg->Nn != c->Nn || !c->H;
  // the batch buffers are shared with the training step (ip2, the score blobs, the slabs): another shape would free a gradient that
  // is still held and restart the gradient scale -- refused while a training pass's state is alive
  if (reshape && grad_exists(c->grad))
    return fail(VV_ERR_STATE, "vv_forward: a batch of %d x (%d + %d) while the training step's buffers hold %d x (%d + %d): the forward-only pass shares the "
                              "step's batch buffers and leaves its state alone -- evaluate with the training shape", cfg->B, cfg->C, cfg->Nn, c->B, c->C, c->Nn);
  // an overlapped or sharded update still in flight: this pass orders itself behind it, as every entry point that touches the parameters
  // does (the next training forward GEMM then finds the update joined and runs ungated: the same values)
  if ((rc = comm_join(c))) return rc;
  if ((rc = vv_ensure_batch(c, cfg->B, cfg->C, cfg->Nn))) return rc;
  const int B = c->B;
  hipStream_t s = c->stream;

  // ---- stage inputs: the indices into an evaluation slot (released by this pass's end event), the cfg's host arrays
  const int32_t* didx = idx;
  int stage_slot = -1;
  if (!idx_on_device) {
    if ((rc = eval_stage_acquire(c, (size_t)c->R * 4, &stage_slot))) return rc;
    if ((rc = stage_indices(c, idx, c->n_rows, c->eval_stage_host[stage_slot]))) return rc;
    didx = c->eval_stage_dev[stage_slot];
  }
  if ((rc = stage_cfg_inputs(c, cfg))) return rc;

  // ---- plan: the execution the training pass takes for this cfg.  The f16 rows' report ring is neither read nor fed: a pass counts nothing.
  const PassPlan p = plan_pass(c, cfg, true);
  const DropSpec dsp = make_drop_spec(c, cfg);
  record_plan(c, p, dsp); c->last_fwd_only = true;

  // ---- group: into the set that never rotates, with no sequence number; the step's stream always waits for it
  if (!p.dd) launch_map_rows(didx, c->rows, c->R, c->Rp, (int32_t)c->n_rows, (int32_t)c->n_rows, s);
  if (p.dd) {
    int si = 0;
    if ((rc = dd_issue(c, didx, idx_on_device, c->n_rows, 0, &si, true))) return rc;
    bind_dd_set(c, c->dd_set[si]);
    if (c->dd_async) HIPCHK(hipStreamWaitEvent(s, c->dd_set[si].done, 0));
  }

  // ---- forward: the training parameters or under vv_ema_use(1) the average's, the forward-only passes' own distinct-row hint, and no
  // sequence stamp (seq_host stays null -- the stamps release the TRAINING steps' staging slots and grouping sets)
  ParamView pv;
  if ((rc = vv_param_view(c, &pv))) return rc;
  const FwdArgs fa = fwd_args(c, cfg, p, pv, *(volatile int32_t*)(c->U_host + 2));
  PROFILED(c, "eval_fwd_gemm", launch_fwd_gemm(c->prec, fa, s));

  // ---- score: no gradient, scale 1, partials of its own, the forward-only instantiations
  ScoreArgs sa = score_args(c, cfg, p, dsp);
  sa.dYh = nullptr; sa.dbp = nullptr; sa.loss_part = c->eval_loss_part; sa.viol_part = c->eval_viol_part; sa.sg = 1.f;
  sa.fwd_only = 1;
  if (p.seg) PROFILED(c, "eval_score", launch_score_fwd(sa, s));
  else PROFILED(c, "eval_score", launch_score_loss(c->prec, sa, s));
  // the loss as the training path's loss workgroup folds it (ReduceArgs::loss_scale: this batch's own B Nn), and the record
  const int64_t terms = (int64_t)B * c->Nn;
  PROFILED(c, "eval_loss", launch_eval_loss(c->eval_loss_part, c->eval_viol_part, B, cfg->loss_weight / (float)terms, terms, c->eval_rec, s));
  HIPCHK(hipGetLastError());
  if (p.dd && c->dd_async) { HIPCHK(hipEventRecord(c->ev_eval, s)); c->eval_set_used = true; }
  if (stage_slot >= 0) { HIPCHK(hipEventRecord(c->eval_stage_done[stage_slot], s)); c->eval_stage_busy[stage_slot] = true; }
  return VV_OK;
}

int vv_eval_reset(vv_ctx* c) {
  if (!c) return fail(VV_ERR_ARG, "vv_eval_reset: ctx is NULL");
  VV_ENTER(c);
  HIPCHK(hipMemsetAsync(c->eval_rec, 0, sizeof(EvalRec), c->stream));      // (behind the passes already queued, in front of the next)
  return VV_OK;
}

int vv_eval_stats(vv_ctx* c, vv_eval_report* out) {
  if (!c || !out) return fail(VV_ERR_ARG, "vv_eval_stats: ctx / out is NULL");
  VV_ENTER(c);
  EvalRec r;
  HIPCHK(hipMemcpyAsync(&r, c->eval_rec, sizeof(r), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  out->passes = r.passes; out->terms = r.terms; out->loss_sum = r.loss_sum; out->viol_sum = r.viol_sum;
  out->last_loss = r.last_loss; out->last_violations = r.last_viol;
  out->mean_loss = r.passes > 0 ? (float)(r.loss_sum / (double)r.passes) : 0.f;
  out->mean_violations = r.passes > 0 ? (float)(r.viol_sum / (double)r.passes) : 0.f;
  return VV_OK;
}


int vv_loss_get(vv_ctx* c, float* loss, float* violations) {
  if (!c) return fail(VV_ERR_ARG, "vv_loss_get: ctx is NULL");
  if (!grad_exists(c->grad)) return fail(VV_ERR_STATE, "vv_loss_get: no forward pass yet");
  VV_ENTER(c);
  if (c->gate_err && *(volatile int32_t*)c->gate_err) { const int rcj = comm_join(c); if (rcj) return rcj; }
  { const int rcr = reduce_now(c); if (rcr) return rcr; }
  float h[2];
  HIPCHK(hipMemcpyAsync(h, c->loss2, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (loss) *loss = h[0];
  if (violations) *violations = h[1];
  return VV_OK;
}

int vv_grads_device(vv_ctx* c, void** dev_ptr, int64_t* n_floats) {
  if (!c || !dev_ptr || !n_floats) return fail(VV_ERR_ARG, "vv_grads_device: NULL argument");
  { const int rcg = upd_pending_guard(c, "vv_grads_device"); if (rcg) return rcg; }
  if (!c->grads) return fail(VV_ERR_STATE, "vv_grads_device: no parameters");
  { const int rcr = reduce_now(c); if (rcr) return rcr; }      // (whoever reads the buffer on the stream finds the gradient queued in front)
  c->grads_exposed = true;                                     // ... and every later one at the end of its vv_forward_backward
  *dev_ptr = c->grads;
  *n_floats = (int64_t)c->D * c->F + c->D;
  return VV_OK;
}

int vv_grads_bind(vv_ctx* c, void* dev_ptr) {
  { const int rcg = upd_pending_guard(c, "vv_grads_bind"); if (rcg) return rcg; }
  if (!c) return fail(VV_ERR_ARG, "vv_grads_bind: ctx is NULL");
  if (!c->grads_own) return fail(VV_ERR_STATE, "vv_grads_bind: no parameters");
  // no synchronisation: kernels already queued keep the pointer they were launched with; the next
  // vv_forward_backward writes, and the next vv_apply_update reads, the newly bound buffer
  { const int rcr = reduce_now(c); if (rcr) return rcr; }      // (a reduction still due goes to the buffer it was computed for)
  c->grads = dev_ptr ? (float*)dev_ptr : c->grads_own;
  return VV_OK;
}

int vv_grads_get(vv_ctx* c, float* dW, float* db) {
  { const int rcg = upd_pending_guard(c, "vv_grads_get"); if (rcg) return rcg; }
  if (!c) return fail(VV_ERR_ARG, "vv_grads_get: ctx is NULL");
  if (!grad_exists(c->grad)) return fail(VV_ERR_STATE, "vv_grads_get: no backward pass yet");
  VV_ENTER(c);
  { const int rcj = comm_join(c); if (rcj) return rcj; }       // block-wise all-reduces in flight: the buffer is read whole
  { const int rcr = reduce_now(c); if (rcr) return rcr; }
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
  { const int rcj = comm_join(c); if (rcj) return rcj; }
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
  int rc = upd_pending_guard(c, "vv_debug_mark_update");       // (a hinted step's parameters are half-way until its vv_apply_update)
  if (rc) return rc;
  VV_ENTER(c);
  if ((rc = comm_join(c))) return rc;
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
  if (want_master && c->comm_sharded) return fail(VV_ERR_STATE, "vv_debug_stats_queue: W / history entries while %s", kStatSharded);
  if (want_param && (rc = upd_pending_guard(c, "vv_debug_stats_queue"))) return rc;
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
  if ((rc = comm_join(c))) return rc;
  if ((rc = stats_ensure(c))) return rc;
  if (want_grad && (rc = reduce_now(c))) return rc;            // the gradient into the flat buffer, as any reader brings it (vv_grads_get)
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
  { const int rcj = comm_join(c); if (rcj) return rcj; }
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
  int rc = ensure_scratch_rows(c, n);
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
  { const int rcg = upd_pending_guard(c, "vv_embed"); if (rcg) return rcg; }     // (a hinted step half-way: new half copy, old bias)
  VV_ENTER(c);
  { const int rcj = comm_join(c); if (rcj) return rcj; }
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
  { const int rcg = upd_pending_guard(c, "vv_embed_mean"); if (rcg) return rcg; }     // (a hinted step half-way: new half copy, old bias)
  VV_ENTER(c);
  { const int rcj = comm_join(c); if (rcj) return rcj; }
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
  { const int rcg = upd_pending_guard(c, "vv_comm_init"); if (rcg) return rcg; }
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
  if (on && c->comm_sharded && c->params_partial) { VV_ENTER(c); const int rcg = vv_gather_params(c); if (rcg) return rcg; }   // (collective, as in vv_comm_schedule: leaving the sharded schedule)
  c->comm_overlap = on != 0;
  if (on) c->comm_sharded = false;
  return VV_OK;
}

int vv_comm_schedule(vv_ctx* c, int schedule) {
  if (!c) return fail(VV_ERR_ARG, "vv_comm_schedule: ctx is NULL");
  if (schedule < 0 || schedule > 2) return fail(VV_ERR_ARG, "vv_comm_schedule: 0 sync, 1 overlap, 2 sharded");
  if (schedule != 0) if (const char* why = vv_sync_only_feature(c)) return fail(VV_ERR_STATE, "vv_comm_schedule: %s", why);
  { const int rcg = upd_pending_guard(c, "vv_comm_schedule"); if (rcg) return rcg; }
  if (schedule != 2 && c->params_partial) { VV_ENTER(c); const int rcg = vv_gather_params(c); if (rcg) return rcg; }     // (collective: the other schedules update the whole matrix)
  c->comm_overlap = schedule == 1;
  c->comm_sharded = schedule == 2;
  return VV_OK;
}

int vv_allreduce_grads(vv_ctx* c) {
  { const int rcg = upd_pending_guard(c, "vv_allreduce_grads"); if (rcg) return rcg; }
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
    (void)comm_join(c); (void)hipStreamSynchronize(c->stream); vv::comm_destroy(c->comm); c->comm = nullptr;
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

#ifdef VV_LAB
// (lab) copies the 16-word stamp records of the last k_score_fwd launch (VV_LAB_SCORE_TS=1) to `out` (n_items x 16 uint32)
extern "C" int vv_lab_score_ts(vv_ctx* c, uint32_t* out, int n_items) {
  if (!c || !c->lab_score_ts || !out) return VV_ERR_STATE;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out, c->lab_score_ts, (size_t)n_items * 16 * 4, hipMemcpyDeviceToHost));
  return VV_OK;
}
#endif
