// pass.hip -- the pass over one batch behind the C ABI in include/videovec.h: the batch buffers and the index staging slots, the grouping
// issue, the stages of a pass, the training pass (fb_impl behind vv_forward_backward, _ring, _q1) up to where its gradient is left, and the
// forward-only pass (vv_forward, vv_eval_*).  What the backward half decides -- split of K, F-chunks, the gradient's destination, the
// guard's rounds -- is vv_backward_plan.h's; plan_backward fills its input from the context.  The context's life cycle, the accessors and
// vv_comm_join are api.hip's, the update solver.hip's; what crosses between the three files is declared in vv_ctx.h.
#include <cmath>
#include <cstring>
#include <algorithm>
#include <vector>

#include "vv_ctx.h"
#include "vv_backward_plan.h"

namespace vv { bool ablate_on(); }
using namespace vv;

static constexpr BackwardTiles kTiles = {BM, BN, BK, WMAX_SLOTS, SGD_BLOCKS, SEGB_BLOCKS};

// The host waits for a word the GPU writes: spins, after 4096 spins sleeps 20 us per spin, and gives up when stream s has run empty (nothing
// queued any more: every earlier step is done) -- the word is then read once more, since it may have been written just before.  Returns
// whether pred held; the time spent is added to *waited_ms (vv_ctx::wait_ms, VV_TRACE_WAITS).
template <typename Pred>
static bool host_wait(Pred pred, hipStream_t s, double* waited_ms) {
  bool held = false;
  const double tw0 = host_now_ms();
  for (unsigned spins = 0; !(held = pred()); ++spins) {
    if (spins > 4096) { timespec ts = {0, 20000}; nanosleep(&ts, nullptr); }
    if (hipStreamQuery(s) == hipSuccess) { held = pred(); break; }
  }
  *waited_ms += host_now_ms() - tw0;
  return held;
}

extern "C" {

// the per-batch buffers' release: everything vv_ensure_batch allocates, and the state that named it
extern "C++" void vv_free_batch(vv_ctx* c) {
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

// ------------------------------------------------------------------------------- step ---------
extern "C++" int vv_ensure_batch(vv_ctx* c, int B, int C, int Nn) {
  if (B == c->B && C == c->C && Nn == c->Nn && c->H) return VV_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  vv_free_batch(c);
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
  // split-K so that tiles * S is about one wave of workgroups over the 256 CUs (vv_backward_plan.h)
  const int tiles = (c->Dp / BM) * (c->Fp / BN);
  const SplitK sk = split_k_plan(c->Dp, c->Fp, c->Rp, kTiles);
  c->S = sk.S; c->kps = sk.kps;
  c->slab_bytes = (size_t)sk.S * (size_t)slab_pitch(c->Dp, c->Fp) * 4;
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

// n pinned, device-mapped staging slots of `bytes` bytes: the old ones freed, host[i] and its device alias dev[i] allocated anew.  The
// caller has synchronised with whatever read the old ones.
static int stage_slots_alloc(int32_t** host, int32_t** dev, int n, size_t bytes) {
  for (int i = 0; i < n; ++i) {
    if (host[i]) (void)hipHostFree(host[i]);
    host[i] = dev[i] = nullptr;
    HIPCHK(hipHostMalloc((void**)&host[i], bytes, hipHostMallocMapped));
    HIPCHK(hipHostGetDevicePointer((void**)&dev[i], host[i], 0));
  }
  return VV_OK;
}

// Index batches reach the GPU through kStage pinned, device-mapped buffers that the step's first kernel reads in place
// (see vv_forward_backward_ring).  Returns the slot to fill; waits until the step that last read it is past its index
// kernels (the forward GEMM stamps seq_host).
static int stage_acquire(vv_ctx* c, size_t bytes, int* slot) {
  if (bytes != c->stage_bytes) {
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < vv_ctx::kStage; ++i) c->stage_seq[i] = 0;
    { const int rc = stage_slots_alloc(c->stage_host, c->stage_dev, vv_ctx::kStage, bytes); if (rc) return rc; }
    c->stage_bytes = bytes;
  }
  const int sl = c->stage_next;
  c->stage_next = (c->stage_next + 1) % vv_ctx::kStage;
  (void)host_wait([&] { return (int32_t)(__atomic_load_n(c->seq_host, __ATOMIC_ACQUIRE) - c->stage_seq[sl]) >= 0; }, c->stream, &c->wait_ms[3]);
  *slot = sl;
  return VV_OK;
}

// The report entry of step `want` in the host-visible ring (vv_internal.h: GMAX_ENTRY_WORDS; reduce_loss writes it): waits until it is there.
// false: the stream ran empty without it (a step whose reduction never ran).  kLag: how many steps behind the host reads -- fixed, so that
// whatever the reports steer (the gradient scale, the f16 rows' fallback) does not depend on host timing and runs stay bit-reproducible.
constexpr int kLag = 4;
static bool report_wait(vv_ctx* c, int32_t want, hipStream_t s) {
  volatile unsigned long long* en = c->gmax_host + GMAX_ENTRY_WORDS * (want & (GMAX_ENTRIES - 1));
  return host_wait([&] { return (int32_t)(uint32_t)__atomic_load_n(en, __ATOMIC_ACQUIRE) == want; }, s, &c->wait_ms[0]);
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

// F-chunks of the overlapped update (vv_backward_plan.h: chunk_plan) for the current Fp: fills c->chunk_kt[0 .. n], returns n
extern "C++" int vv_chunk_plan(vv_ctx* c) { return chunk_plan(c->Fp / BK, c->n_chunks, c->chunk_kt); }

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
      (void)host_wait([&] { return (int32_t)(__atomic_load_n(c->seq_host + gate_word, __ATOMIC_ACQUIRE) - set.used_seq) > 0; }, s, &c->wait_ms[1]);
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
// arrive filled in for the step; which destination is the backward plan's (sharded, chunked, lazy, fuse_w, slab16); it is recorded in c->grad.
static int wgrad_to_destination(vv_ctx* c, const BackwardPlan& bp, WgradArgs& wa, ReduceArgs& ra, bool upd_hint) {
  hipStream_t s = c->stream;
  const bool sharded = bp.sharded, chunked = bp.chunked, lazy = bp.lazy, fuse_w = bp.fuse_w;
  if (sharded) ra.shard_rows = bp.shard_rows;
  // Data-parallel overlap: the gradient buffer is laid out chunk-major (a few column blocks, each one contiguous
  // all-reduce message) and vv_apply_update runs the update chunk by chunk on the communication stream.
  if (chunked) {
    ra.n_chunks = vv_chunk_plan(c);
    for (int i = 0; i <= ra.n_chunks; ++i) ra.chunk_c0[i] = std::min(c->F, c->chunk_kt[i] * BK);
  }
  // the W -> half scale update the previous vv_apply_update left pending rides in this step's reduction launch (a lazy reduction: in
  // whichever launch reduces the slabs later)
  if (!lazy && c->scale_pending) {
    ra.scale_sc = c->scales; ra.scale_wmax = c->wmax_blocks + c->wmax_cur * WMAX_SLOTS; ra.scale_n = c->wmax_n; ra.scale_prec = c->prec;
    c->scale_pending = false; c->wmax_seed_live = false;
  }
  c->upd_announced = upd_hint;
  c->fb_hinted = upd_hint; c->grad_banked = false;       // (vv_grads_bank: a new gradient, bankable once unless it was announced)
  c->grad_unapplied = true;
  // fuse_w: the solver's rule is applied in the weight-gradient GEMM's epilogue (WgradUpd) and the 4 D F bytes of dW are neither written
  // nor read back (the shipped configuration: D = F = 4096, 134 MB of the update's 370).  vv_apply_update then runs only the bias / loss
  // workgroups.
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
  // f16 split-K partial products (option "slab16"): whoever reduces the slabs -- k_reduce, k_reduce_sgd, now or lazily -- reads the same flag
  if (bp.slab16) {
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

// The backward half of this pass (vv_backward_plan.h), from the context, the pass plan and whether vv_update_hint announced the step: the
// one place that reads these fields for a decision
static BackwardPlan plan_backward(const vv_ctx* c, const PassPlan& p, bool upd_hint) {
  BackwardPlanIn in;
  in.comm = c->comm != nullptr; in.world = c->comm ? vv::comm_world(c->comm) : 0; in.comm_sharded = c->comm_sharded; in.comm_overlap = c->comm_overlap;
  in.D = c->D; in.F = c->F; in.Dp = c->Dp; in.Fp = c->Fp; in.Rp = c->Rp; in.B = c->B; in.S = c->S;
  in.grads_own = c->grads == c->grads_own; in.grads_exposed = c->grads_exposed;
  in.fuse_update = c->fuse_update; in.wgrad_update = c->wgrad_update; in.slab16 = c->slab16; in.wgrad_lean = c->ko.wgrad_lean != 0;
  in.guard_proactive = c->guard_proactive; in.fuse_keep_grads = c->fuse_keep_grads; in.can_fuse_update = wgrad_can_fuse_update();
  in.hinted = upd_hint; in.hint_adam = c->upd_cfg.solver_type == VV_SOLVER_ADAM; in.hint_clip = c->upd_clip >= 0.f;
  in.f16 = c->prec == VV_PREC_F16; in.dd = p.dd; in.seg = p.seg; in.table_rows = c->n_rows + 1 + c->patch_cap;
  return backward_plan(in, kTiles);
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
  return vv_comm_join(c);
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

// ---- the guard rounds of a training step: the score kernels and the backward to per-row gradients.
// f16 gradient-scale guard (vv_internal.h: GradGuard): the kernels that round gradients to 16 bits are launched once as
// usual (round 0) and once more per guard round as conditional repeats -- near-empty launches unless the round before
// reported a value past f16's range.  Rounds: 1 where one kernel rounds (per-instance rows, or the segment sums); 2 for
// rows + their sums (k_segsum): sums of clipped rows say nothing about the true sums, which the second round sees.
// gd leaves as the reduction needs it (its n_of[], gg).
static int guard_rounds(vv_ctx* c, const PassPlan& p, const BackwardPlan& bp, const DropSpec& dsp, ScoreArgs& sa, int32_t seq, bool h16_count, GuardArgs& gd) {
  hipStream_t s = c->stream;
  if (c->prec == VV_PREC_F16) { gd.gg = c->gg; gd.slots = c->gg_slots; gd.nslot = c->gg_nslot; gd.seq = seq; }
  c->gg_last_seq = gd.gg ? seq : 0;
  // (the segment-wise backward needs no repeat at all: its score kernel bounds every instance's gradient and k_seg_bwd
  // settles the scale before it rounds anything -- GuardArgs::proactive)
  // (lab: guard_proactive 0 runs the repeat form on this path too)
  const bool proactive = bp.proactive;
  const int n_rounds = bp.n_rounds;
  c->gg_last_rounds = n_rounds;
  gd.n_of[0] = bp.n_of[0];
  gd.n_of[1] = bp.n_of[1];
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
    ba.dbp = c->seg_dbp; ba.Rp = c->Rp; ba.D = c->D; ba.Dp = c->Dp; ba.inv_sg = 1.f / c->sg; ba.h16 = p.h16 ? 1 : 0; ba.v16 = p.v16 ? 1 : 0;
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
  return VV_OK;
}

// ---- the weight-gradient GEMM's arguments and the reduction's, filled in for the step (wgrad_to_destination adds where the gradient goes)
static void wgrad_reduce_args(const vv_ctx* c, const vv_step_cfg* cfg, const PassPlan& p, const BackwardPlan& bp, const GuardArgs& gd, int32_t seq, bool h16_count,
                              WgradArgs& wa, ReduceArgs& ra) {
  wa.dYh = p.dd ? c->dYu : c->dYh; wa.table = c->table; wa.rows = p.dd ? c->dd_uniq : c->rows; wa.slabs = c->slabs;
  wa.Rp = c->Rp; wa.Dp = c->Dp; wa.Fp = c->Fp; wa.S = c->S; wa.ksteps_per_split = c->kps;
  wa.n_dev = p.dd ? c->dd_info : nullptr; wa.zero_row = (int32_t)c->n_rows;
  wa.lean = bp.lean;
  ra.slabs = c->slabs; ra.S = c->S; ra.Dp = c->Dp; ra.Fp = c->Fp; ra.dbp = p.seg ? c->seg_dbp : c->dbp; ra.B = c->B;
  ra.db_rows = p.seg ? SEGB_BLOCKS : 0;
  ra.scales = c->scales; ra.sg = c->sg; ra.grads = c->grads; ra.D = c->D; ra.F = c->F;
  if (gd.gg) {
    ra.gg = c->gg; ra.gmax_slots = c->gg_slots; ra.gmax_n0 = gd.n_of[0]; ra.gmax_n1 = gd.n_of[1]; ra.gmax_stride = c->gg_nslot;
    ra.gmax_host = c->gmax_host_dev; ra.seq = seq; ra.guard_last_round = bp.n_rounds;
    if (bp.proactive) { ra.gbound = c->gg_bound; ra.gcnt = c->dd_info + 1; }
  }
  if (h16_count) {       // (bf16 operands publish a report entry for these steps only: the rows of H are f16 there too)
    ra.gmax_host = c->gmax_host_dev; ra.seq = seq;
    ra.h16_cnt = c->h16_cnt; ra.h16_cnt_n = SEGB_BLOCKS;
  }
  ra.ip_scale = cfg->ip_regularization > 0.f ? 1.f + cfg->ip_regularization * 0.5f : 1.f;     // inner_product_layer.cpp:80-90
  ra.loss_part = c->loss_part; ra.viol_part = c->viol_part; ra.loss_scale = cfg->loss_weight / (float)((int64_t)c->B * c->Nn); ra.loss_out = c->loss2;
}

static int fb_impl(vv_ctx* c, const vv_step_cfg* cfg, const int32_t* idx, int idx_on_device, int64_t row_limit, int32_t seq = 0) {
  // ---- guards
  { const int rcg = vv_upd_pending_guard(c, "vv_forward_backward"); if (rcg) return rcg; }
  const bool upd_hint = c && c->upd_hint;       // (consumed by this call whatever path it takes)
  if (c) c->upd_hint = false;
  if (c && c->ema_in_use) return fail(VV_ERR_STATE, "vv_forward_backward: %s", kEmaInUse);
  int rc = vv_check_cfg(c, cfg);
  if (rc) return rc;
  if (!idx) return fail(VV_ERR_ARG, "vv_forward_backward: idx is NULL");
  VV_ENTER(c);
  // (an overlapped update of the previous step may still be arriving: see the forward GEMM below)
  if (c->upd_sync == UpdSync::InFlight && (cfg->B != c->B || cfg->C != c->C || cfg->Nn != c->Nn || !c->H) && (rc = vv_comm_join(c))) return rc;
  if ((rc = vv_ensure_batch(c, cfg->B, cfg->C, cfg->Nn))) return rc;
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
  const BackwardPlan bp = plan_backward(c, p, upd_hint);
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
  GuardArgs gd;
  if ((rc = guard_rounds(c, p, bp, dsp, sa, seq, h16_count, gd))) return rc;

  // ---- weight gradient: its arguments and the reduction's, then wherever the gradient goes
  WgradArgs wa;
  ReduceArgs ra;
  wgrad_reduce_args(c, cfg, p, bp, gd, seq, h16_count, wa, ra);
  return wgrad_to_destination(c, bp, wa, ra, upd_hint);
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
extern "C++" int vv_ensure_scratch_rows(vv_ctx* c, int64_t need) {
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
  if (P > 0 && (rc = vv_ensure_scratch_rows(c, P))) return rc;
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
      c->eval_stage_busy[i] = false;
      if (!c->eval_stage_done[i]) HIPCHK(hipEventCreateWithFlags(&c->eval_stage_done[i], hipEventDisableTiming));
    }
    { const int rc = stage_slots_alloc(c->eval_stage_host, c->eval_stage_dev, vv_ctx::kEvalStage, bytes); if (rc) return rc; }
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
  { const int rcg = vv_upd_pending_guard(c, "vv_forward"); if (rcg) return rcg; }
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
  if ((rc = vv_comm_join(c))) return rc;
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
