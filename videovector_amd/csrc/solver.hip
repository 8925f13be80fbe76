// solver.hip -- the solver's side of the C ABI in include/videovec.h: its settings (vv_solver_ext_*, vv_solver_iter_*), the second history,
// gradient clipping, the moving average of the parameters, the gradient bank, the step's carried state (vv_run_state_*), and the parameter
// update in its five forms (vv_apply_update, vv_step).  The step that produces the gradient is pass.hip's; what crosses between the
// files is declared in vv_ctx.h.
#include <cmath>
#include <cstring>
#include <algorithm>

#include "vv_ctx.h"

using namespace vv;

extern "C" {

static inline int comm_join(vv_ctx* c) { return vv_comm_join(c); }
static inline int reduce_now(vv_ctx* c) { return vv_reduce_now(c); }
static inline int upd_pending_guard(vv_ctx* c, const char* who) { return vv_upd_pending_guard(c, who); }

// ---- the features that run on the sync exchange schedule only, and why: each one's entry point refuses to start under another schedule,
// vv_apply_update refuses a gradient laid out for one, and vv_comm_overlap / vv_comm_schedule refuse to leave sync while one is active
static const char* const kClipSchedule = "gradient clipping runs on the sync exchange schedule only (it needs the summed gradient's norm before the first "
                                         "chunk or shard is updated): vv_clip_gradients_set(< 0) or vv_comm_schedule(0)";
static const char* const kBankSchedule = "gradients are banked on the sync exchange schedule only (the bank is exchanged whole, once per cycle, before the first "
                                         "chunk or shard is updated): vv_grads_bank_reset or vv_comm_schedule(0)";
static const char* const kEmaSchedule = "the moving average runs on the sync exchange schedule only (every rank averages the whole, identical parameter "
                                        "matrix behind its update): vv_ema_set(< 0) or vv_comm_schedule(0)";
// the message of the first active one -- clipping, the bank, the moving average -- or nullptr
extern "C++" const char* vv_sync_only_feature(const vv_ctx* c) {
  return c->clip >= 0.f ? kClipSchedule : c->bank_count > 0 ? kBankSchedule : c->ema_decay >= 0.f ? kEmaSchedule : nullptr;
}

// ---- the solvers beyond the reference's three (BVLC Caffe's RMSPropSolver / AdamSolver): what vv_step_cfg has no field for
int vv_solver_ext_set(vv_ctx* c, float momentum2, float rms_decay) {
  if (!c) return fail(VV_ERR_ARG, "vv_solver_ext_set: ctx is NULL");
  if (!(momentum2 == momentum2) || !(rms_decay == rms_decay)) return fail(VV_ERR_ARG, "vv_solver_ext_set: NaN");
  c->momentum2 = momentum2; c->rms_decay = rms_decay;      // (their ranges are checked with the rule that uses them: vv_check_cfg)
  return VV_OK;
}
int vv_solver_ext_get(vv_ctx* c, float* momentum2, float* rms_decay) {
  if (!c) return fail(VV_ERR_ARG, "vv_solver_ext_get: ctx is NULL");
  if (momentum2) *momentum2 = c->momentum2;
  if (rms_decay) *rms_decay = c->rms_decay;
  return VV_OK;
}
int vv_solver_iter_set(vv_ctx* c, int64_t t) {
  if (!c || t < 0) return fail(VV_ERR_ARG, "vv_solver_iter_set: bad argument");
  c->adam_t = t;
  return VV_OK;
}
int vv_solver_iter_get(vv_ctx* c, int64_t* t) {
  if (!c || !t) return fail(VV_ERR_ARG, "vv_solver_iter_get: NULL argument");
  *t = c->adam_t;
  return VV_OK;
}
// ---- the step's carried state (vv_run_state_*): what a training step reads that earlier steps left and no other getter returns.
// DESIGN.md, "Resume bit for bit", lists every member with the line that reads it.
namespace {
constexpr uint64_t kRunMagic = 0x3154534e55525656ull;        // "VVRUNST1"
constexpr uint32_t kRunVersion = 1;
struct RunHdr {
  uint64_t magic; uint32_t version, hdr_bytes;
  int64_t total_bytes;
  int32_t D, F, Dp, Fp, prec, pad0_;
  int32_t B, C, Nn, pad2_;                                   // the batch shape the per-shape members below belong to (0: no step yet)
  uint64_t iter;                                             // the dropout counter (the counter mask's argument)
  int32_t step_seq, gg_seq0, sg_adj, h16_arm_seq;            // the steps' sequence numbers; the gradient scale's steering
  float sg; int32_t h16_fallback;
  int64_t gg_repeats, h16_flagged_steps, h16_first_flagged, h16_flag_step, h16_flag_sat, h16_flag_faint;
  int32_t h16_counted[GMAX_ENTRIES];                         // which report entries the f16 rows' guard still has to read
  int32_t u_hint[3], wmax_cur;                               // the distinct-row hints; the per-block maxima buffer the last update wrote
  int32_t wmax_n, scale_pending, wmax_seed_live, pad1_;
  Scales scales;                                             // device: sw_cur / sw_next lag max |W| by one update
  GradGuard gg;                                              // device
  unsigned long long gmax[GMAX_ENTRIES * GMAX_ENTRY_WORDS];  // the report ring both guards read at a fixed lag
};
static_assert(sizeof(RunHdr) % 8 == 0, "RunHdr");
int64_t run_state_bytes(const vv_ctx* c) { return (int64_t)sizeof(RunHdr) + (int64_t)2 * WMAX_SLOTS * 4 + (int64_t)c->Dp * c->Fp * 2; }
// where neither call has a defined answer
int run_state_guard(vv_ctx* c, const char* who, bool put) {
  if (!c->W) return fail(VV_ERR_STATE, "%s: no parameters", who);
  if (put ? grad_exists(c->grad) : c->grad_unapplied)
    return fail(VV_ERR_STATE, put ? "%s: a gradient is held: the state goes into a context fresh from vv_params_set" : "%s: a gradient is held that no update has consumed: the state would miss it (vv_apply_update first)", who);
  if (c->upd_hint || c->upd_announced) return fail(VV_ERR_STATE, "%s: a step announced by vv_update_hint is under way", who);
  if (c->bank_count > 0) return fail(VV_ERR_STATE, "%s: %d gradients are banked (vv_apply_update or vv_grads_bank_reset first)", who, c->bank_count);
  if (c->comm_overlap || c->comm_sharded || c->upd_sync != UpdSync::Joined || c->params_partial)
    return fail(VV_ERR_STATE, "%s: the overlapped / sharded schedule keeps an update in flight between steps (vv_comm_schedule(0) first)", who);
  if (c->ema_in_use) return fail(VV_ERR_STATE, "%s: %s", who, kEmaInUse);
  return VV_OK;
}
}  // namespace

int vv_run_state_size(vv_ctx* c, int64_t* bytes) {
  if (!c || !bytes) return fail(VV_ERR_ARG, "vv_run_state_size: NULL argument");
  if (!c->W) return fail(VV_ERR_STATE, "vv_run_state_size: no parameters (the size depends on D and F)");
  *bytes = run_state_bytes(c);
  return VV_OK;
}

int vv_run_state_get(vv_ctx* c, void* buf, int64_t cap, int64_t* written) {
  if (!c || !buf) return fail(VV_ERR_ARG, "vv_run_state_get: NULL argument");
  if (written) *written = 0;
  { const int rcg = run_state_guard(c, "vv_run_state_get", false); if (rcg) return rcg; }
  const int64_t need = run_state_bytes(c);
  if (cap < need) return fail(VV_ERR_ARG, "vv_run_state_get: %lld bytes of room, the state has %lld", (long long)cap, (long long)need);
  VV_ENTER(c);
  { const int rcj = comm_join(c); if (rcj) return rcj; }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->dd_stream) HIPCHK(hipStreamSynchronize(c->dd_stream));
  RunHdr h; memset(&h, 0, sizeof(h));
  h.magic = kRunMagic; h.version = kRunVersion; h.hdr_bytes = (uint32_t)sizeof(RunHdr); h.total_bytes = need;
  h.D = c->D; h.F = c->F; h.Dp = c->Dp; h.Fp = c->Fp; h.prec = c->prec;
  h.B = c->B; h.C = c->C; h.Nn = c->Nn;
  h.iter = c->iter;
  h.step_seq = c->step_seq; h.gg_seq0 = c->gg_seq0; h.sg_adj = c->sg_adj; h.h16_arm_seq = c->h16_arm_seq;
  h.sg = c->sg; h.h16_fallback = c->h16_fallback ? 1 : 0;
  h.gg_repeats = c->gg_repeats; h.h16_flagged_steps = c->h16_flagged_steps; h.h16_first_flagged = c->h16_first_flagged;
  h.h16_flag_step = c->h16_flag_step; h.h16_flag_sat = c->h16_flag_sat; h.h16_flag_faint = c->h16_flag_faint;
  memcpy(h.h16_counted, c->h16_counted, sizeof(h.h16_counted));
  for (int i = 0; i < 3; ++i) h.u_hint[i] = *(volatile int32_t*)(c->U_host + i);
  h.wmax_cur = c->wmax_cur; h.wmax_n = c->wmax_n; h.scale_pending = c->scale_pending ? 1 : 0; h.wmax_seed_live = c->wmax_seed_live ? 1 : 0;
  HIPCHK(hipMemcpy(&h.scales, c->scales, sizeof(Scales), hipMemcpyDeviceToHost));
  if (c->gg) HIPCHK(hipMemcpy(&h.gg, c->gg, sizeof(GradGuard), hipMemcpyDeviceToHost));
  for (int i = 0; i < GMAX_ENTRIES * GMAX_ENTRY_WORDS; ++i) h.gmax[i] = __atomic_load_n(c->gmax_host + i, __ATOMIC_ACQUIRE);
  unsigned char* q = (unsigned char*)buf;
  memcpy(q, &h, sizeof(h)); q += sizeof(h);
  HIPCHK(hipMemcpy(q, c->wmax_blocks, (size_t)2 * WMAX_SLOTS * 4, hipMemcpyDeviceToHost)); q += (size_t)2 * WMAX_SLOTS * 4;
  HIPCHK(hipMemcpy(q, c->Wh, (size_t)c->Dp * c->Fp * 2, hipMemcpyDeviceToHost));
  if (written) *written = need;
  return VV_OK;
}

int vv_run_state_put(vv_ctx* c, const void* buf, int64_t bytes) {
  if (!c || !buf) return fail(VV_ERR_ARG, "vv_run_state_put: NULL argument");
  { const int rcg = run_state_guard(c, "vv_run_state_put", true); if (rcg) return rcg; }
  if (bytes < (int64_t)sizeof(RunHdr)) return fail(VV_ERR_ARG, "vv_run_state_put: %lld bytes hold no header", (long long)bytes);
  RunHdr h; memcpy(&h, buf, sizeof(h));
  if (h.magic != kRunMagic) return fail(VV_ERR_ARG, "vv_run_state_put: not a run state (magic)");
  if (h.version != kRunVersion || h.hdr_bytes != sizeof(RunHdr)) return fail(VV_ERR_ARG, "vv_run_state_put: state version %u, this library reads %u", h.version, kRunVersion);
  if (h.D != c->D || h.F != c->F) return fail(VV_ERR_ARG, "vv_run_state_put: the state was taken at D = %d, F = %d, this context has D = %d, F = %d", h.D, h.F, c->D, c->F);
  if (h.prec != c->prec) return fail(VV_ERR_ARG, "vv_run_state_put: the state was taken with operand type %d, this context has %d", h.prec, c->prec);
  if (h.Dp != c->Dp || h.Fp != c->Fp || h.total_bytes != run_state_bytes(c) || bytes != h.total_bytes)
    return fail(VV_ERR_ARG, "vv_run_state_put: %lld bytes given, the state of this context has %lld (truncated or over-long)", (long long)bytes, (long long)run_state_bytes(c));
  if (h.wmax_cur < 0 || h.wmax_cur > 1 || h.wmax_n < 0 || h.wmax_n > WMAX_SLOTS) return fail(VV_ERR_ARG, "vv_run_state_put: damaged state (per-block maxima)");
  if (h.B < 0 || h.C < 0 || h.Nn < 0 || (h.B > 0 && h.C < 2)) return fail(VV_ERR_ARG, "vv_run_state_put: damaged state (batch shape)");
  VV_ENTER(c);
  { const int rcj = comm_join(c); if (rcj) return rcj; }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->dd_stream) HIPCHK(hipStreamSynchronize(c->dd_stream));
  // The gradient scale's steering and the distinct-row hints belong to a batch shape: sizing the batch buffers starts them afresh
  // (free_batch, vv_ensure_batch).  So the buffers are sized for the state's shape FIRST -- the resumed run's first step then finds them
  // as the interrupted run's next step would have -- and the state is written over the fresh start.
  if (h.B > 0) { const int rcb = vv_ensure_batch(c, h.B, h.C, h.Nn); if (rcb) return rcb; }
  c->iter = h.iter;
  c->step_seq = h.step_seq; c->gg_seq0 = h.gg_seq0; c->sg_adj = h.sg_adj; c->h16_arm_seq = h.h16_arm_seq;
  c->sg = h.sg; c->h16_fallback = h.h16_fallback != 0;
  c->gg_repeats = h.gg_repeats; c->h16_flagged_steps = h.h16_flagged_steps; c->h16_first_flagged = h.h16_first_flagged;
  c->h16_flag_step = h.h16_flag_step; c->h16_flag_sat = h.h16_flag_sat; c->h16_flag_faint = h.h16_flag_faint;
  memcpy(c->h16_counted, h.h16_counted, sizeof(h.h16_counted));
  for (int i = 0; i < 3; ++i) c->U_host[i] = h.u_hint[i];
  c->wmax_cur = h.wmax_cur; c->wmax_n = h.wmax_n; c->scale_pending = h.scale_pending != 0; c->wmax_seed_live = h.wmax_seed_live != 0;
  // every earlier step is over: both stamps stand at the last sequence number, as they would behind a synchronised run
  c->seq_host[0] = c->seq_host[1] = h.step_seq;
  for (int i = 0; i < vv_ctx::kDdAll; ++i) c->dd_set[i].used_seq = 0;
  for (int i = 0; i < vv_ctx::kStage; ++i) c->stage_seq[i] = h.step_seq;
  h.scales.sx = c->sx;                                       // (the table is this context's own)
  HIPCHK(hipMemcpy(c->scales, &h.scales, sizeof(Scales), hipMemcpyHostToDevice));
  if (c->gg) HIPCHK(hipMemcpy(c->gg, &h.gg, sizeof(GradGuard), hipMemcpyHostToDevice));
  c->gg_last_seq = 0;                                        // (the launch records speak of steps of this context: none since the state was set)
  for (int i = 0; i < GMAX_ENTRIES * GMAX_ENTRY_WORDS; ++i) __atomic_store_n(c->gmax_host + i, h.gmax[i], __ATOMIC_RELEASE);
  const unsigned char* q = (const unsigned char*)buf + sizeof(RunHdr);
  HIPCHK(hipMemcpy(c->wmax_blocks, q, (size_t)2 * WMAX_SLOTS * 4, hipMemcpyHostToDevice)); q += (size_t)2 * WMAX_SLOTS * 4;
  HIPCHK(hipMemcpy(c->Wh, q, (size_t)c->Dp * c->Fp * 2, hipMemcpyHostToDevice));
  HIPCHK(hipDeviceSynchronize());
  c->ema_packed = false;
  return VV_OK;
}

// the second history, zero-filled, on the first use of a two-history solver (or vv_history2_set): the only allocation a step may make
static int ensure_history2(vv_ctx* c) {
  if (c->hW2) return VV_OK;
  const size_t nW = (size_t)c->D * c->F;
  HIPCHK(hipMalloc(&c->hW2, nW * 4)); HIPCHK(hipMalloc(&c->hb2, (size_t)c->D * 4));
  HIPCHK(hipMemset(c->hW2, 0, nW * 4)); HIPCHK(hipMemset(c->hb2, 0, (size_t)c->D * 4));
  HIPCHK(hipDeviceSynchronize());            // (the fills are complete before a kernel of any stream reads them)
  return VV_OK;
}
int vv_history2_set(vv_ctx* c, const float* vW, const float* vb) {
  if (!c) return fail(VV_ERR_ARG, "vv_history2_set: ctx is NULL");
  { const int rcg = upd_pending_guard(c, "vv_history2_set"); if (rcg) return rcg; }
  if (!c->W) return fail(VV_ERR_STATE, "vv_history2_set: no parameters");
  VV_ENTER(c);
  { const int rcj = comm_join(c); if (rcj) return rcj; }
  HIPCHK(hipStreamSynchronize(c->stream));
  { const int rce = ensure_history2(c); if (rce) return rce; }
  const size_t nW = (size_t)c->D * c->F;
  if (vW) HIPCHK(hipMemcpy(c->hW2, vW, nW * 4, hipMemcpyHostToDevice)); else HIPCHK(hipMemset(c->hW2, 0, nW * 4));
  if (vb) HIPCHK(hipMemcpy(c->hb2, vb, (size_t)c->D * 4, hipMemcpyHostToDevice)); else HIPCHK(hipMemset(c->hb2, 0, (size_t)c->D * 4));
  HIPCHK(hipDeviceSynchronize());
  c->hist2_partial = false;                  // (every rank is given the whole history)
  return VV_OK;
}
int vv_history2_get(vv_ctx* c, float* vW, float* vb) {
  if (!c) return fail(VV_ERR_ARG, "vv_history2_get: ctx is NULL");
  { const int rcg = upd_pending_guard(c, "vv_history2_get"); if (rcg) return rcg; }
  if (!c->W) return fail(VV_ERR_STATE, "vv_history2_get: no parameters");
  VV_ENTER(c);
  { const int rcj = comm_join(c); if (rcj) return rcj; }
  { const int rcg = vv_gather_params(c); if (rcg) return rcg; }
  HIPCHK(hipStreamSynchronize(c->stream));
  const size_t nW = (size_t)c->D * c->F;
  if (!c->hW2) {                             // no two-history update yet: the history is zero
    if (vW) memset(vW, 0, nW * 4);
    if (vb) memset(vb, 0, (size_t)c->D * 4);
    return VV_OK;
  }
  if (vW) HIPCHK(hipMemcpy(vW, c->hW2, nW * 4, hipMemcpyDeviceToHost));
  if (vb) HIPCHK(hipMemcpy(vb, c->hb2, (size_t)c->D * 4, hipMemcpyDeviceToHost));
  return VV_OK;
}

// ---- gradient clipping by the global L2 norm (BVLC Caffe's SGDSolver::ClipGradients, sgd_solver.cpp; the reference tree has none)
int vv_clip_gradients_set(vv_ctx* c, float clip) {
  if (!c) return fail(VV_ERR_ARG, "vv_clip_gradients_set: ctx is NULL");
  if (!(clip == clip)) return fail(VV_ERR_ARG, "vv_clip_gradients_set: NaN");
  if (clip >= 0.f && (c->comm_overlap || c->comm_sharded)) return fail(VV_ERR_STATE, "vv_clip_gradients_set: %s", kClipSchedule);
  if (clip >= 0.f && !c->clip_rec) {         // the record, the partial sums, the arrival counter: here, never on the step path
    VV_ENTER(c);
    const size_t bytes = sizeof(ClipRec) + (size_t)CLIP_BLOCKS * sizeof(double) + 16;
    HIPCHK(hipMalloc((void**)&c->clip_rec, bytes));
    HIPCHK(hipMemset(c->clip_rec, 0, bytes));
    HIPCHK(hipDeviceSynchronize());            // (the fill is complete before a kernel of any stream reads it)
  }
  c->clip = clip;
  return VV_OK;
}
int vv_clip_gradients_get(vv_ctx* c, float* clip) {
  if (!c || !clip) return fail(VV_ERR_ARG, "vv_clip_gradients_get: NULL argument");
  *clip = c->clip;
  return VV_OK;
}
int vv_clip_stats(vv_ctx* c, vv_clip_report* out) {
  if (!c || !out) return fail(VV_ERR_ARG, "vv_clip_stats: ctx / out is NULL");
  out->norm = 0.f; out->scale = 1.f; out->clipped = 0; out->updates = out->clipped_updates = 0;
  if (!c->clip_rec) return VV_OK;              // clipping was never active
  VV_ENTER(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  ClipRec r;
  HIPCHK(hipMemcpy(&r, c->clip_rec, sizeof(r), hipMemcpyDeviceToHost));
  if (r.updates > 0) { out->norm = r.norm; out->scale = r.scale; out->clipped = r.clipped; }
  out->updates = r.updates; out->clipped_updates = r.clipped_updates;
  return VV_OK;
}
// ClipGradients on the gradient buffer: k_grad_sumsq, then k_grad_scale (with a communicator the buffer holds the sum over the ranks:
// every rank reads identical buffers)
static void clip_buffer(vv_ctx* c) {
  ClipArgs a;
  a.g = c->grads; a.n = (int64_t)c->D * c->F + c->D; a.clip = c->clip;
  a.rec = c->clip_rec; a.part = (double*)(c->clip_rec + 1); a.arrived = (uint32_t*)(a.part + CLIP_BLOCKS);
  a.skip_if = c->comm ? vv::comm_fail_flag(c->comm) : nullptr;
  PROFILED(c, "grad_sumsq", launch_grad_sumsq(a, c->stream));
  PROFILED(c, "grad_scale", launch_grad_scale(a, c->stream));
}

// ---- the exponential moving average of the parameters (this project's own: neither the reference tree nor BVLC Caffe keeps one)
extern "C++" void vv_ema_release(vv_ctx* c) {
  dfree(c->eW);
  c->eW = c->eb = nullptr; c->escales = nullptr; c->eWh = nullptr; c->ema_packed = false;
}
// the one allocation (per D) and the start of the average: a device copy of W and b as they stand behind everything queued
extern "C++" int vv_ema_init(vv_ctx* c) {
  static_assert(sizeof(Scales) == 16, "the average's 16-bit copy starts on a 16-byte boundary behind its Scales block");
  const size_t nW = (size_t)c->D * c->F, off_b = (size_t)round_up((int64_t)nW, 4), off_s = off_b + (size_t)round_up(c->D, 4);
  if (!c->eW) {
    const size_t bytes = off_s * 4 + sizeof(Scales) + (size_t)c->Dp * c->Fp * 2;
    HIPCHK(hipMalloc((void**)&c->eW, bytes));
    HIPCHK(hipMemset(c->eW, 0, bytes));          // (the padding of the 16-bit copy reads zero, as Wh's)
    HIPCHK(hipDeviceSynchronize());              // (the fill is complete before a kernel of any stream reads it)
    c->eb = c->eW + off_b; c->escales = (Scales*)(c->eW + off_s); c->eWh = (uint16_t*)(c->escales + 1);
  }
  HIPCHK(hipMemcpyAsync(c->eW, c->W, nW * 4, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->eb, c->b, (size_t)c->D * 4, hipMemcpyDeviceToDevice, c->stream));
  c->ema_packed = false;
  return VV_OK;
}
int vv_ema_set(vv_ctx* c, float decay) {
  if (!c) return fail(VV_ERR_ARG, "vv_ema_set: ctx is NULL");
  if (!(decay == decay) || decay >= 1.f) return fail(VV_ERR_ARG, "vv_ema_set: decay must be < 0 (off) or in [0, 1)");
  if (decay < 0.f) {
    if (c->ema_in_use) return fail(VV_ERR_STATE, "vv_ema_set: the averaged parameters are in use (vv_ema_use(0) first)");
    if (c->eW) { VV_ENTER(c); HIPCHK(hipStreamSynchronize(c->stream)); vv_ema_release(c); }      // (a k_ema still queued writes it)
    c->ema_decay = -1.f;
    return VV_OK;
  }
  if (c->comm_overlap || c->comm_sharded) return fail(VV_ERR_STATE, "vv_ema_set: %s", kEmaSchedule);
  if (c->ema_decay < 0.f) {                    // activation: the average starts from the parameters as they stand
    if (!c->W) return fail(VV_ERR_STATE, "vv_ema_set: no parameters (vv_params_set first: the average starts from them)");
    { const int rcg = upd_pending_guard(c, "vv_ema_set"); if (rcg) return rcg; }      // (a hinted step half-way: new matrix, old bias)
    VV_ENTER(c);
    int rc = comm_join(c);                     // (an overlapped update of an earlier schedule may still be writing W)
    if (rc) return rc;
    if (c->params_partial && (rc = vv_gather_params(c))) return rc;
    if ((rc = vv_ema_init(c))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->ema_updates = 0;
  }
  c->ema_decay = decay;                        // (another decay while active: the average is kept)
  return VV_OK;
}
int vv_ema_get_decay(vv_ctx* c, float* decay) {
  if (!c || !decay) return fail(VV_ERR_ARG, "vv_ema_get_decay: NULL argument");
  *decay = c->ema_decay;
  return VV_OK;
}
int vv_ema_get(vv_ctx* c, float* W, float* b) {
  if (!c) return fail(VV_ERR_ARG, "vv_ema_get: ctx is NULL");
  if (c->ema_decay < 0.f) return fail(VV_ERR_STATE, "vv_ema_get: the moving average is off (vv_ema_set)");
  VV_ENTER(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (W) HIPCHK(hipMemcpy(W, c->eW, (size_t)c->D * c->F * 4, hipMemcpyDeviceToHost));
  if (b) HIPCHK(hipMemcpy(b, c->eb, (size_t)c->D * 4, hipMemcpyDeviceToHost));
  return VV_OK;
}
int vv_ema_put(vv_ctx* c, const float* W, const float* b) {
  if (!c) return fail(VV_ERR_ARG, "vv_ema_put: ctx is NULL");
  if (c->ema_decay < 0.f) return fail(VV_ERR_STATE, "vv_ema_put: the moving average is off (vv_ema_set)");
  VV_ENTER(c);
  HIPCHK(hipStreamSynchronize(c->stream));     // (a k_ema still queued reads and writes it)
  if (W) HIPCHK(hipMemcpy(c->eW, W, (size_t)c->D * c->F * 4, hipMemcpyHostToDevice));
  if (b) HIPCHK(hipMemcpy(c->eb, b, (size_t)c->D * 4, hipMemcpyHostToDevice));
  c->ema_packed = false;
  return VV_OK;
}
// The 16-bit copy of the average and its scale, as vv_params_set makes W's: max |e| -> the power-of-two scale -> round to nearest even.
// Cached until the next k_ema (or re-initialisation, or another table scale).
static int ema_pack(vv_ctx* c) {
  if (c->ema_packed) return VV_OK;
  hipStream_t s = c->stream;
  HIPCHK(hipMemcpyAsync(&c->escales->sx, &c->scales->sx, sizeof(float), hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemsetAsync(&c->escales->wmax_bits, 0, sizeof(unsigned), s));
  launch_absmax(c->eW, (int64_t)c->D * c->F, &c->escales->wmax_bits, s);
  launch_scale_update(c->prec, c->escales, nullptr, 0, s);
  PROFILED(c, "ema_pack", launch_w_convert(c->prec, c->eW, c->eWh, c->D, c->F, c->Dp, c->Fp, c->escales, s));
  HIPCHK(hipGetLastError());
  c->ema_packed = true;
  return VV_OK;
}
int vv_ema_use(vv_ctx* c, int on) {
  if (!c) return fail(VV_ERR_ARG, "vv_ema_use: ctx is NULL");
  if (!on) { c->ema_in_use = false; return VV_OK; }      // the training view again: nothing a step owns was moved
  if (c->ema_decay < 0.f) return fail(VV_ERR_STATE, "vv_ema_use: the moving average is off (vv_ema_set)");
  { const int rcg = upd_pending_guard(c, "vv_ema_use"); if (rcg) return rcg; }
  if (c->upd_announced && grad_exists(c->grad))
    return fail(VV_ERR_STATE, "vv_ema_use: the last backward pass was announced by vv_update_hint and its vv_apply_update has not run -- call vv_apply_update first");
  c->upd_hint = false;                         // (a hint not yet consumed announced a step that cannot come now)
  c->ema_in_use = true;
  return VV_OK;
}
int vv_ema_stats(vv_ctx* c, vv_ema_report* out) {
  if (!c || !out) return fail(VV_ERR_ARG, "vv_ema_stats: ctx / out is NULL");
  out->updates = c->ema_decay >= 0.f ? c->ema_updates : 0; out->decay = c->ema_decay; out->in_use = c->ema_in_use ? 1 : 0;
  return VV_OK;
}
extern "C++" int vv_param_view(vv_ctx* c, ParamView* v) {
  if (!c->ema_in_use) { v->Wh = c->Wh; v->b = c->b; v->scales = c->scales; return VV_OK; }
  const int rc = ema_pack(c);
  v->Wh = c->eWh; v->b = c->eb; v->scales = c->escales;
  return rc;
}

// ---- gradient accumulation (BVLC Caffe's SolverParameter.iter_size: Solver::Step and SGDSolver::Normalize; the reference tree has none)
static inline size_t bank_floats(const vv_ctx* c) { return (size_t)c->D * c->F + c->D; }
// BVLC Solver::Step's accumulating Net::ForwardBackward: the layers add into the parameter diffs
int vv_grads_bank(vv_ctx* c) {
  if (!c) return fail(VV_ERR_ARG, "vv_grads_bank: ctx is NULL");
  if (!grad_exists(c->grad)) return fail(VV_ERR_STATE, "vv_grads_bank: no backward pass yet");
  { const int rcg = upd_pending_guard(c, "vv_grads_bank"); if (rcg) return rcg; }
  if (c->fb_hinted) return fail(VV_ERR_STATE, "vv_grads_bank: the last backward pass was announced by vv_update_hint: its gradient is not kept (run the pass without the hint to bank it)");
  if (c->grad_banked) return fail(VV_ERR_STATE, "vv_grads_bank: the gradient of the last backward pass has been banked already (one bank per vv_forward_backward)");
  if (c->comm_overlap || c->comm_sharded) return fail(VV_ERR_STATE, "vv_grads_bank: %s", kBankSchedule);
  if (c->grad.at == GradAt::Buffer && c->grad.buf.layout != GradLayout::Flat) return fail(VV_ERR_STATE, "vv_grads_bank: this step's gradient was laid out for another schedule -- %s", kBankSchedule);
  if (c->comm && c->grad.at == GradAt::Buffer && !grad_sum_due(c->grad))
    return fail(VV_ERR_STATE, "vv_grads_bank: this gradient has been summed over the ranks already (vv_allreduce_grads); the bank is exchanged once per cycle, by vv_apply_update");
  VV_ENTER(c);
  int rc = comm_join(c);                     // (an overlapped update of an earlier schedule may still be writing)
  if (rc) return rc;
  if (!c->bank_rec) {                        // the one allocation: here, never on the step path afterwards
    static_assert(sizeof(AccumRec) % 16 == 0, "the bank starts on a 16-byte boundary behind its record");
    const size_t bytes = sizeof(AccumRec) + (bank_floats(c) + 4) * sizeof(float);
    HIPCHK(hipMalloc((void**)&c->bank_rec, bytes));
    HIPCHK(hipMemset(c->bank_rec, 0, bytes));
    HIPCHK(hipDeviceSynchronize());          // (the fill is complete before a kernel of any stream reads it)
  }
  if ((rc = reduce_now(c))) return rc;       // the gradient into the buffer and the loss into its scalars, as any reader brings them
  const bool first = c->bank_count == 0;
  if (first) c->bank = (float*)(c->bank_rec + 1) + (((uintptr_t)c->grads & 15) / 4);     // one 16-byte grid in both buffers
  BankArgs a;
  a.src = c->grads; a.dst = c->bank; a.n = (int64_t)bank_floats(c);
  a.fold = 1; a.loss2 = c->loss2; a.rec = c->bank_rec;
  PROFILED(c, "grad_bank", launch_grad_bank(first ? BankOp::Store : BankOp::Add, a, c->stream));
  HIPCHK(hipGetLastError());
  c->bank_count++;
  c->grad_banked = true;
  return VV_OK;
}
// BVLC Net::ClearParamDiffs (Solver::Step's first statement)
int vv_grads_bank_reset(vv_ctx* c) {
  if (!c) return fail(VV_ERR_ARG, "vv_grads_bank_reset: ctx is NULL");
  c->bank_count = 0;                         // (the next bank stores: neither the bank nor the two sums are read again)
  return VV_OK;
}
// BVLC Solver::Step's "loss /= iter_size"
int vv_accum_stats(vv_ctx* c, vv_accum_report* out) {
  if (!c || !out) return fail(VV_ERR_ARG, "vv_accum_stats: ctx / out is NULL");
  out->banked = c->bank_count; out->last_count = 0; out->last_mean_loss = out->last_mean_violations = 0.f; out->updates = 0;
  if (!c->bank_rec) return VV_OK;              // nothing was ever banked
  VV_ENTER(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  AccumRec r;
  HIPCHK(hipMemcpy(&r, c->bank_rec, sizeof(r), hipMemcpyDeviceToHost));
  out->last_count = r.last_count; out->last_mean_loss = r.last_mean_loss; out->last_mean_violations = r.last_mean_viol; out->updates = r.updates;
  return VV_OK;
}
// BVLC SGDSolver::ApplyUpdate's first half for m banked gradients: the sum into the flat gradient buffer, its exchange, ClipGradients on
// the sum, Normalize.  Steps are one pass where the bits cannot differ: without a communicator and without clipping, the write and the
// multiply.  The regulariser and the rule follow in the plain k_sgd.
static int bank_to_buffer(vv_ctx* c, bool clip_on) {
  int rc;
  const int m = c->bank_count;
  BankArgs a;
  a.n = (int64_t)bank_floats(c); a.inv = 1.0f / (float)m; a.m = m; a.rec = c->bank_rec;
  a.skip_if = c->comm ? vv::comm_fail_flag(c->comm) : nullptr;
  const bool two_pass = c->comm || clip_on;
  if (two_pass) {
    a.src = c->bank; a.dst = c->grads;
    PROFILED(c, "grad_bank", launch_grad_bank(BankOp::Store, a, c->stream));
    grad_to_buffer(c->grad, GradLayout::Flat, !c->comm, false);     // the buffer holds this rank's sum; with a communicator the sum over the ranks is due
    if ((rc = vv_allreduce_grads(c))) return rc;                     // ONE exchange per cycle
    if (clip_on) clip_buffer(c);
  }
  a.src = two_pass ? c->grads : c->bank; a.dst = c->grads; a.fold = 2;
  PROFILED(c, "grad_bank", launch_grad_bank(BankOp::Scale, a, c->stream));
  grad_to_buffer(c->grad, GradLayout::Flat, true, false);
  HIPCHK(hipGetLastError());
  c->bank_count = 0;                         // a new cycle; the buffer holds the normalised sum, not a backward pass's gradient: grad_banked stays
  return VV_OK;
}

// The solver's parameters of a step as the update kernels read them (k_sgd, k_reduce_sgd, the weight-gradient GEMM's epilogue)
// momentum2 / rms_decay: the context's vv_solver_ext_set values (as they stood at vv_update_hint for an announced rule); t: the 1-based
// count of the Adam update this rule is for (0: none -- corr stays 1).  The 1 - x coefficients are formed here, once, in fp32.
extern "C++" SolverRule vv_solver_rule(const vv_step_cfg& cfg, float momentum2, float rms_decay, int64_t t) {
  SolverRule r;
  r.rate = cfg.lr; r.momentum = cfg.momentum; r.weight_decay = cfg.weight_decay;
  r.lr_mult_w = cfg.lr_mult[0]; r.lr_mult_b = cfg.lr_mult[1];
  r.decay_mult_w = cfg.decay_mult[0]; r.decay_mult_b = cfg.decay_mult[1];
  r.reg = cfg.reg; r.solver_type = cfg.solver_type; r.delta = cfg.delta;
  if (cfg.solver_type == VV_SOLVER_RMSPROP) { r.decay2 = rms_decay; r.om2 = 1.f - rms_decay; }
  if (cfg.solver_type == VV_SOLVER_ADAM) {
    r.decay2 = momentum2; r.om1 = 1.f - cfg.momentum; r.om2 = 1.f - momentum2;
    // BVLC AdamSolver::ComputeUpdateValue: correction = sqrt(1 - beta2^t) / (1 - beta1^t), t = iter + 1; in double, rounded once
    if (t > 0) r.corr = (float)(std::sqrt(1.0 - std::pow((double)momentum2, (double)t)) / (1.0 - std::pow((double)cfg.momentum, (double)t)));
  }
  return r;
}
// A launch just queued on s recomputed the W -> half scale (consumed: FusedUpdArgs / WgradUpd::recompute_scale) and so folded
// vv_params_set's seed in Scales::wmax_bits into it: clear the seed behind that launch
extern "C++" hipError_t vv_clear_wmax_seed(vv_ctx* c, bool consumed, hipStream_t s) {
  if (!consumed || !c->wmax_seed_live) return hipSuccess;
  const hipError_t e = hipMemsetAsync(&c->scales->wmax_bits, 0, sizeof(unsigned), s);
  if (e == hipSuccess) c->wmax_seed_live = false;
  return e;
}

// The end of every update: the n_slots per-block maxima it wrote (the buffer the previous update did not write) are what the next
// W -> half scale update folds; that update is left pending (it rides in the next reduction or is flushed by whoever needs it first)
static int finish_update(vv_ctx* c, int n_slots) {
  c->wmax_cur = 1 - c->wmax_cur; c->wmax_n = n_slots;
  c->scale_pending = true;
  if (c->adam_pending) { c->adam_t++; c->adam_pending = false; }      // the Adam update is queued: its t is taken
  c->upd_announced = false;
  c->grad_unapplied = false;
  HIPCHK(hipGetLastError());
  if (c->ema_decay >= 0.f) {                   // the moving average, once per completed update: k_ema behind it on the step's stream, reading the new W and b
    EmaArgs e;
    e.W = c->W; e.b = c->b; e.eW = c->eW; e.eb = c->eb; e.nW = (int64_t)c->D * c->F; e.nb = c->D;
    e.decay = c->ema_decay; e.om = 1.0f - c->ema_decay;
    e.skip_if = c->comm ? vv::comm_fail_flag(c->comm) : nullptr;
    PROFILED(c, "ema", launch_ema(e, c->F % 4 == 0, c->stream));
    HIPCHK(hipGetLastError());
    c->ema_updates++; c->ema_packed = false;
  }
  c->iter++;
  c->prof_calls++;
  return VV_OK;
}

static void flush_scale_update(vv_ctx* c) {
  if (!c->scale_pending) return;
  launch_scale_update(c->prec, c->scales, c->wmax_blocks + c->wmax_cur * WMAX_SLOTS, c->wmax_n, c->stream);
  c->scale_pending = false;
  c->wmax_seed_live = false;               // (the scale update folds and clears Scales::wmax_bits)
}

// The five forms of the update.  Each is handed the common SgdArgs (vv_apply_update's prologue), Adam's second history (vW / vb, or NULL)
// and ends in finish_update.

// 1: finish a step whose parameter matrix the weight-gradient GEMM has updated (GradAt::SlabsWUpdated)
static int update_finish_wgrad(vv_ctx* c, const SgdArgs& a) {
  // the parameter matrix was updated in the weight-gradient GEMM (vv_update_hint): bias, loss, the guard's report -- k_reduce_sgd's
  // special workgroups alone -- and the bookkeeping of the scale
  // (what the weight-gradient GEMM applied: WgradUpd::rule -- the bias multipliers may differ, the bias is updated here)
  const SolverRule h = vv_solver_rule(c->upd_cfg, c->upd_momentum2, c->upd_rms_decay);
  const SolverRule& r = a.rule;
  if (r.rate != h.rate || r.momentum != h.momentum || r.weight_decay != h.weight_decay || r.lr_mult_w != h.lr_mult_w ||
      r.decay_mult_w != h.decay_mult_w || r.reg != h.reg || r.solver_type != h.solver_type || r.delta != h.delta || r.decay2 != h.decay2)
    return fail(VV_ERR_ARG, "vv_apply_update: the solver parameters differ from those announced by vv_update_hint (the weights were updated with the announced ones)");
  FusedUpdArgs fa;
  fa.r = c->red_args; fa.g = a; fa.prec = c->prec; fa.no_params = 1; fa.recompute_scale = 0; fa.store_grads = 0;
  grad_update_consumed(c->grad);              // (-> Lost: dW of this step never existed outside the GEMM's registers)
  PROFILED(c, "reduce_sgd", (void)launch_reduce_sgd(fa, c->stream));
  return finish_update(c, c->upd_wgrad_blocks);
}

// 2: the reduction is still due (GradAt::Slabs): reduce and update in one launch (k_reduce_sgd)
static int update_fused(vv_ctx* c, const SgdArgs& a, float* vW, float* vb) {
  FusedUpdArgs fa;
  fa.r = c->red_args; fa.g = a; fa.prec = c->prec;
  fa.recompute_scale = c->scale_pending ? 1 : 0;
  fa.wmax_prev = c->wmax_blocks + c->wmax_cur * WMAX_SLOTS; fa.wmax_prev_n = c->wmax_n;
  fa.store_grads = c->fuse_keep_grads;
  if (fa.store_grads) grad_reduced(c->grad); else grad_update_consumed(c->grad);      // (-> Buffer, or SlabsStale: dW stays in the slabs)
  int n_new = 0;
  PROFILED(c, "reduce_sgd", (n_new = launch_reduce_sgd(fa, c->stream, vW, vb)));
  HIPCHK(vv_clear_wmax_seed(c, fa.recompute_scale, c->stream));
  return finish_update(c, n_new);
}

// 3: the sharded schedule (GradLayout::Sharded, the sum over the ranks due)
static int update_sharded(vv_ctx* c, const SgdArgs& a, float* vW, float* vb) {
  // Exact synchronous SGD, the update SHARDED over the ranks (Multi-GPU): on the communication stream, behind one event of
  // the compute stream,   reduce-scatter (fp32, shard-major buffer: 7/8 of it on the wire at N = 8, once)  ->  k_sgd on THIS rank's
  // D / N rows (1/N of the update's 46 MB)  ->  ONE grouped all-gather of what every rank's next forward pass reads: the 16-bit copy
  // of W (4 MB instead of the all-reduce's second 8.4 MB), the bias, the per-block maxima the next W -> half scale comes from  ->
  // publish.  3/4 of the all-reduce's wire bytes.  The next forward GEMM is gated on the one flag (it starts, and waits in front of
  // its first W tile); the fp32 master W and the history stay sharded until vv_params_get gathers them.
  // comm_inline (default): this schedule has ONE gate, in front of the GEMM's first W tile -- nothing of the exchange hides behind the
  // GEMM, and the second stream costs its hand-off chain (event -> wake -> ... -> publish: + 17 us on one rank).  So the
  // three steps are queued on the COMPUTE stream itself, in order, and the next forward GEMM is the plain kernel (with its sibling lead).
  const bool adam = vW != nullptr;
  const bool inl = c->comm_inline;
  hipStream_t cs = inl ? c->stream : vv::comm_stream(c->comm);
  const int world = vv::comm_world(c->comm), rank = vv::comm_rank(c->comm);
  const int rps = c->D / world;
  const size_t shard_f = (size_t)rps * c->F + rps;
  int32_t useq = c->upd_seq;
  if (!inl) { HIPCHK(hipEventRecord(c->ev_chunk, c->stream)); useq = ++c->upd_seq; }
  if (c->comm_test_delay_us > 0) { if (!inl) HIPCHK(hipStreamWaitEvent(cs, c->ev_chunk, 0)); launch_delay(c->comm_test_delay_us, cs); }
  struct StreamScope { vv::Comm* k; ~StreamScope() { vv::comm_use_stream(k, nullptr); } } scope{c->comm};
  vv::comm_use_stream(c->comm, inl ? c->stream : nullptr);
  if (vv::comm_reduce_scatter(c->comm, c->grads, shard_f, inl ? nullptr : c->ev_chunk)) return fail(VV_ERR_HIP, "reduce-scatter: %s", vv::comm_error(c->comm));
  const int nb = SGD_BLOCKS / world;
  SgdArgs g = a;                                    // the shard as a parameter matrix of its own: rps rows, its gradient buffer [dW rows | db entries]
  g.D = rps;
  g.W = c->W + (size_t)rank * rps * c->F; g.hW = c->hW + (size_t)rank * rps * c->F;
  g.b = c->b + (size_t)rank * rps; g.hb = c->hb + (size_t)rank * rps;
  g.grads = c->grads + (size_t)rank * shard_f;
  float* const svW = adam ? vW + (size_t)rank * rps * c->F : nullptr; float* const svb = adam ? vb + (size_t)rank * rps : nullptr;     // the shard owns its rows of v
  g.Wh = c->Wh + (size_t)rank * rps * c->Fp;
  g.chunked = 1; g.f_begin = 0; g.f_count = c->F; g.do_bias = 1; g.set_scale = 1;      // (chunked = 1 with the whole width: this launch's own grid and slots)
  g.blk_off = rank * nb; g.n_blk = nb;
  PROFILED(c, "sgd", launch_sgd(c->prec, g, cs, svW, svb));
  void* bufs[3] = {c->Wh, c->b, a.wmax_blocks};
  const size_t sbytes[3] = {(size_t)rps * c->Fp * 2, (size_t)rps * 4, (size_t)nb * 4};
  if (vv::comm_allgather(c->comm, bufs, sbytes, 3)) return fail(VV_ERR_HIP, "all-gather: %s", vv::comm_error(c->comm));
  if (!inl) {
    launch_publish(c->w_gate, useq, cs);
    if (vv::comm_record_done(c->comm)) return fail(VV_ERR_HIP, "all-gather: %s", vv::comm_error(c->comm));
  }
  grad_update_consumed(c->grad);
  if (!inl) upd_queued(c->upd_sync);          // (in-stream: vv_apply_update joined whatever was in flight)
  c->params_partial = world > 1;
  if (adam) c->hist2_partial = world > 1;
  return finish_update(c, nb * world);
}

// 4: the overlapped schedule (GradLayout::Chunked, the sum over the ranks due)
static int update_overlapped(vv_ctx* c, SgdArgs a, float* vW, float* vb) {
  // Exact synchronous SGD with the exchange hidden behind the NEXT step's forward GEMM: behind one event of the compute
  // stream, the communication stream runs per F-chunk  all-reduce -> SGD on the chunk's columns -> publish w_gate[chunk];
  // the next forward GEMM (fb_impl) starts right away and waits for each chunk where its K loop reaches it.  db rides
  // with the last chunk; the bias is updated there.
  hipStream_t cs = vv::comm_stream(c->comm);
  const int32_t useq = ++c->upd_seq;
  const int nch = vv_chunk_plan(c);               // (the layout k_reduce wrote: same Fp, same plan)
  const bool chunk0 = c->grad.buf.chunk0_event;
  a.pub_count = c->pub_count; a.pub_seq = useq;
  HIPCHK(hipEventRecord(c->ev_chunk, c->stream));
  for (int k = 0; k < nch; ++k) {
    // chunk 0 may start as soon as ITS reduction is done (ev_chunk0, fb_impl); the others follow the whole backward pass
    hipEvent_t after = k == 0 ? (chunk0 ? c->ev_chunk0 : c->ev_chunk) : (k == 1 && chunk0 ? c->ev_chunk : nullptr);
    const int c0 = std::min(c->F, c->chunk_kt[k] * BK), c1 = std::min(c->F, c->chunk_kt[k + 1] * BK);
    const bool last = k == nch - 1;
    const size_t off = (size_t)c->D * c0, n = (size_t)c->D * (c1 - c0) + (last ? (size_t)c->D : 0);
    const int delay_us = c->comm_test_delay_us;
    if (after) HIPCHK(hipStreamWaitEvent(cs, after, 0));
    if (delay_us > 0) launch_delay(delay_us, cs);      // test hook: a slow exchange, so that the next forward GEMM really waits at its gates
    const bool skip_ar1 = c->comm_skip_ar1;   // (lab) diagnosis: no collective call at world 1
    if (!(skip_ar1 && vv::comm_world(c->comm) == 1) && n > 0 && vv::comm_allreduce(c->comm, c->grads, off, n, nullptr))
      return fail(VV_ERR_HIP, "all-reduce: %s", vv::comm_error(c->comm));
    a.chunked = 1; a.f_begin = c0; a.f_count = c1 - c0; a.do_bias = last; a.set_scale = k == 0;
    a.blk_off = k * (SGD_BLOCKS / nch); a.n_blk = last ? SGD_BLOCKS - a.blk_off : SGD_BLOCKS / nch;      // together: every slot of wmax_blocks
    a.pub_flag = c->w_gate + k * W_GATE_STRIDE;          // the kernel's last workgroup publishes the chunk (SgdArgs::pub_flag)
    if (k == 0) PROFILED(c, "sgd", launch_sgd(c->prec, a, cs, vW, vb)); else launch_sgd(c->prec, a, cs, vW, vb);     // (an empty chunk: its wmax slots become 0, the bias if it is the last)
  }
  if (vv::comm_record_done(c->comm)) return fail(VV_ERR_HIP, "all-reduce: %s", vv::comm_error(c->comm));
  grad_update_consumed(c->grad);
  upd_queued(c->upd_sync);                    // (comm_done_event now marks the end of THIS update, behind the old one)
  return finish_update(c, SGD_BLOCKS);
}

// 5: the gradient is in the buffer, summed: plain k_sgd
static int update_plain(vv_ctx* c, const SgdArgs& a, float* vW, float* vb) {
  PROFILED(c, "sgd", launch_sgd(c->prec, a, c->stream, vW, vb));
  grad_update_consumed(c->grad);
  // The next W -> half scale (k_scale_update: folds this kernel's per-block max |w|) is needed by the NEXT k_sgd only.  It
  // is left pending and performed by one extra workgroup of the next step's k_reduce; anything else that touches the
  // scales or the parameters first flushes it as its own launch.
  return finish_update(c, SGD_BLOCKS);
}

int vv_apply_update(vv_ctx* c, const vv_step_cfg* cfg) {
  int rc = vv_check_cfg(c, cfg);
  if (rc) return rc;
  if (c->ema_in_use) return fail(VV_ERR_STATE, "vv_apply_update: %s", kEmaInUse);
  if (!grad_exists(c->grad)) return fail(VV_ERR_STATE, "vv_apply_update: no gradients (call vv_forward_backward)");
  if ((rc = upd_pending_guard(c, "vv_apply_update"))) return rc;     // (GradAt::Lost: a second update on a gradient that was never stored)
  // Banked gradients (vv_grads_bank, m >= 1): the update consumes the bank -- BVLC SGDSolver::ApplyUpdate on the accumulated diffs
  const bool banked = c->bank_count > 0;
  if (banked && !c->grad_banked)
    return fail(VV_ERR_STATE, "vv_apply_update: %d gradients are banked and the last backward pass's is not among them (vv_grads_bank it, or vv_grads_bank_reset)", c->bank_count);
  VV_ENTER(c);
  // two updates in a row: the first one completes first.  (After a gated forward GEMM -- UpdSync::Gated -- nothing is due here: the
  // new update is queued on the communication stream behind the old one, and what this step's kernels on the compute stream read
  // of the old one -- the half copy, its scale, the bias, the per-block maxima -- was stored at agent scope before the gates opened.)
  // That holds only while the new update goes to the communication stream too.  One that runs on the COMPUTE stream -- the schedule was
  // switched to `sync`, the gradient buffer was handed out or bound after an overlapped step, the sharded update runs in-stream -- reads
  // W and the history, which the previous update wrote with plain stores released only at its end: it joins first.
  const bool overlapped = c->comm && grad_sum_due(c->grad) && c->grad.buf.layout == GradLayout::Chunked;
  const bool sharded = c->comm && grad_sum_due(c->grad) && c->grad.buf.layout == GradLayout::Sharded;
  // Gradient clipping (vv_clip_gradients_set >= 0): the step's gradient goes to the buffer by the transition a reader takes (the plain
  // k_reduce), k_grad_sumsq and k_grad_scale run on it, then the plain k_sgd -- form 1 or 2; the fused forms are not used.  "Exactly
  // these solver parameters" of vv_update_hint includes the threshold.
  const bool clip_on = c->clip >= 0.f;
  if (c->upd_announced && c->clip != c->upd_clip)
    return fail(VV_ERR_ARG, "vv_apply_update: the solver parameters differ from those announced by vv_update_hint (vv_clip_gradients_set's threshold)");
  // (the bank never meets such a gradient: vv_grads_bank refuses one, and no schedule but sync can be chosen while gradients are banked)
  if (overlapped || sharded) if (const char* why = vv_sync_only_feature(c)) return fail(VV_ERR_STATE, "vv_apply_update: this step's gradient was laid out for another schedule -- %s", why);
  const bool on_comm_stream = overlapped || (sharded && !c->comm_inline);
  if ((c->upd_sync == UpdSync::InFlight || (c->upd_sync == UpdSync::Gated && !on_comm_stream)) && (rc = comm_join(c))) return rc;
  // A sharded update left the other ranks' rows of the fp32 master W and of the history stale here; an update of the WHOLE matrix needs
  // them (the step left the sharded path -- gradients exposed or bound, the schedule changed -- without a gather).  A
  // collective, like the update itself: every rank takes this branch in the same iteration.
  if (!sharded && c->params_partial && (rc = vv_gather_params(c))) return rc;
  // data-parallel: the update consumes the SUM over the ranks (of banked gradients: the bank's, exchanged by bank_to_buffer)
  if (!banked && !overlapped && !sharded && grad_sum_due(c->grad) && (rc = vv_allreduce_grads(c))) return rc;
  SgdArgs a;
  float* const wmax_new = c->wmax_blocks + (1 - c->wmax_cur) * WMAX_SLOTS;     // the buffer the previous update did not write
  a.W = c->W; a.b = c->b; a.hW = c->hW; a.hb = c->hb; a.grads = c->grads; a.Wh = c->Wh; a.scales = c->scales; a.wmax_blocks = wmax_new;
  a.D = c->D; a.F = c->F; a.Dp = c->Dp; a.Fp = c->Fp;
  // Adam: the second history (allocated by the first such update) and this update's own bias correction -- t is the library's counter of
  // Adam updates, every queued update carries its corr_t as a kernel argument and nothing synchronises
  const bool adam = cfg->solver_type == VV_SOLVER_ADAM;
  if (adam && c->grad.at == GradAt::SlabsWUpdated) return fail(VV_ERR_ARG, "vv_apply_update: the solver parameters differ from those announced by vv_update_hint (the weights were updated with the announced ones)");
  if (adam && (rc = ensure_history2(c))) return rc;
  a.rule = vv_solver_rule(*cfg, c->momentum2, c->rms_decay, adam ? c->adam_t + 1 : 0);     // (t is committed where the update is queued: finish_update)
  c->adam_pending = adam;
  float* const vW = adam ? c->hW2 : nullptr; float* const vb = adam ? c->hb2 : nullptr;
  a.skip_if = c->comm ? vv::comm_fail_flag(c->comm) : nullptr;
  if (banked) {                        // (the banks brought every gradient into the buffer: nothing is left in the slabs; form 1 or 2)
    flush_scale_update(c);
    if ((rc = bank_to_buffer(c, clip_on))) return rc;
    return update_plain(c, a, vW, vb);
  }
  if (c->grad.at == GradAt::SlabsWUpdated) return update_finish_wgrad(c, a);
  if (c->grad.at == GradAt::Slabs && !clip_on) return update_fused(c, a, vW, vb);
  if ((rc = reduce_now(c))) return rc;       // (GradAt::SlabsStale: a second update on the same gradient reads it from the buffer)
  flush_scale_update(c);               // two updates in a row without a step between them
  if (clip_on) clip_buffer(c);         // (the sum over the ranks, where one is due, is queued in front)
  if (sharded) return update_sharded(c, a, vW, vb);
  if (overlapped) return update_overlapped(c, a, vW, vb);
  return update_plain(c, a, vW, vb);
}

int vv_step(vv_ctx* c, const vv_step_cfg* cfg, const int32_t* idx, int idx_on_device) {
  if (c && c->ema_in_use) return fail(VV_ERR_STATE, "vv_step: %s", kEmaInUse);
  if (c && c->bank_count > 0)
    return fail(VV_ERR_STATE, "vv_step: %d gradients are banked and this step's would not be among them (vv_forward_backward + vv_grads_bank + vv_apply_update, or vv_grads_bank_reset)", c->bank_count);
  int rc = vv_update_hint(c, cfg);                  // (nothing reads the gradient between the two halves of this call)
  if (rc) return rc;
  rc = vv_forward_backward(c, cfg, idx, idx_on_device);
  if (rc) return rc;
  return vv_apply_update(c, cfg);
}
}  // extern "C"
