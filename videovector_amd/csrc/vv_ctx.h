// vv_ctx.h -- the context object behind include/videovec.h's vv_ctx, shared by api.hip (the context, the options, the table, the
// parameters, the accessors), pass.hip (the pass over a batch: the fused training step's forward and backward), solver.hip (the
// solver's state and the parameter update), ops.hip (the per-layer operators), retrieval.hip, classify.hip, linear.hip, kmeans.hip, ivf_coarse.hip, ivf.hip and
// pq.hip (the evaluation paths); below it, what these files call of one another.  Internal.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <map>
#include <string>
#include <vector>

#include "../../include/videovec.h"
#include "vv_internal.h"
#include "vv_comm.h"
#include "vv_step_state.h"

extern thread_local char vv_g_err[512];
int vv_fail(int code, const char* fmt, ...);
#define fail vv_fail
#define HIPCHK(x)                                                                              \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess)                                                                      \
      return vv_fail(VV_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, \
                     __LINE__);                                                                \
  } while (0)
// every entry point that launches kernels: the device of the context, and ITS kernel options for the launchers on this thread
#define VV_ENTER(c) do { HIPCHK(hipSetDevice((c)->device)); vv::g_ko = &(c)->ko; \
    if ((c)->comm && vv::comm_failed((c)->comm)) return fail(VV_ERR_HIP, "the data-parallel exchange failed: %s", vv::comm_error((c)->comm)); } while (0)

inline void dfree(void* p) { if (p) (void)hipFree(p); }
// environment of a PRODUCT option (read once per context) / of a lab switch (ignored unless the library was built with -DVV_LAB)
inline const char* opt_env(const char* name) { return getenv(name); }
#ifdef VV_LAB
inline const char* lab_env(const char* name) { return getenv(name); }
#else
inline const char* lab_env(const char*) { return nullptr; }
#endif

// A device allocation that lives for one API call: released on every return path, the early error returns of HIPCHK
// included.
template <typename T>
struct DevTmp {
  T* p = nullptr;
  DevTmp() = default;
  DevTmp(const DevTmp&) = delete;
  DevTmp& operator=(const DevTmp&) = delete;
  ~DevTmp() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t count) { return hipMalloc((void**)&p, count * sizeof(T)); }
  operator T*() const { return p; }
};

// Events that live for one API call (the timed legs of kmeans.hip and ivf_coarse.hip): destroyed on every return path.
struct CallEvents {
  std::vector<hipEvent_t> e;
  CallEvents() = default;
  CallEvents(const CallEvents&) = delete;
  CallEvents& operator=(const CallEvents&) = delete;
  ~CallEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  hipError_t create(size_t count) {
    e.assign(count, nullptr);
    for (hipEvent_t& x : e) { const hipError_t rc = hipEventCreate(&x); if (rc != hipSuccess) return rc; }
    return hipSuccess;
  }
};

struct ProfEntry { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; };

struct vv_ctx {
  int device = 0, prec = 0;
  hipStream_t stream = nullptr, own_stream = nullptr;

  // feature table
  uint16_t* table = nullptr; int64_t n_rows = 0; int F = 0, Fp = 0; float sx = 1.f;
  int64_t patch_cap = 0;            // scratch rows after the zero row (quirk Q1 composites)
  int32_t* patch_desc = nullptr; int64_t patch_desc_cap = 0;
  // parameters
  int D = 0, Dp = 0;
  float *W = nullptr, *b = nullptr, *hW = nullptr, *hb = nullptr;
  // the second history (Adam's v; hW / hb hold m): allocated zero-filled by the first two-history update or by vv_history2_set, never on
  // the step path after that; vv_params_set clears it
  float *hW2 = nullptr, *hb2 = nullptr;
  float momentum2 = 0.999f, rms_decay = 0.99f;   // vv_solver_ext_set: sticky (BVLC SolverParameter's defaults)
  int64_t adam_t = 0;                       // Adam updates applied so far (the next one uses t = adam_t + 1); vv_solver_iter_set, reset by vv_params_set
  bool adam_pending = false;                // the vv_apply_update in progress is an Adam update: finish_update commits adam_t (a failed call leaves t alone)
  float upd_momentum2 = 0.f, upd_rms_decay = 0.f;   // ... as they stood when vv_update_hint announced upd_cfg
  bool hist2_partial = false;               // as params_partial, for hW2 / hb2 (a sharded Adam update ran since the last gather)
  // vv_clip_gradients_set (BVLC SolverParameter.clip_gradients): < 0 off; sticky.  While >= 0 vv_apply_update brings the gradient into the
  // buffer, runs k_grad_sumsq + k_grad_scale and then the plain k_sgd; the fused forms and the overlapped / sharded schedules are not used.
  float clip = -1.f;
  float upd_clip = -1.f;                    // ... as it stood when vv_update_hint announced upd_cfg
  bool upd_announced = false;               // the last backward pass was announced by vv_update_hint and its vv_apply_update has not run yet
  vv::ClipRec* clip_rec = nullptr;          // device: the record, then CLIP_BLOCKS partial sums and the arrival counter (one allocation, made by vv_clip_gradients_set)
  // vv_grads_bank (BVLC SolverParameter.iter_size): the bank, a second flat [dW | db] buffer.  ONE allocation made zero-filled by the first
  // bank: the record, then D F + D floats and four of slack -- `bank` starts as many floats past a 16-byte boundary as the gradient buffer
  // does (set by the first bank of every cycle), so that k_grad_bank finds one 16-byte grid in both.
  vv::AccumRec* bank_rec = nullptr; float* bank = nullptr;
  int bank_count = 0;                       // gradients in the bank (m); 0: vv_apply_update is what it always was
  bool grad_banked = false;                 // the last backward pass's gradient has been banked, or the buffer holds an accumulated update's
                                            // normalised sum in its place: not banked again (a backward pass clears it)
  bool fb_hinted = false;                   // the last backward pass was announced by vv_update_hint: its gradient is not banked
  bool grad_unapplied = false;              // a backward pass has left a gradient that no completed vv_apply_update has consumed yet (vv_run_state_get
                                            // refuses: the blob would miss it); cleared by finish_update and wherever the gradient is discarded
  // vv_op_asum / vv_debug_stats_queue (the reference's debug_info, net.cpp:580-636).  stat_rec: ONE allocation made zero-filled by the first
  // call that measures, never on the step path afterwards -- VV_STAT_N records and vv_op_asum's own, then k_abs_stats' partials and its
  // arrival counter.  upd_shadow: vv_debug_mark_update's copy of W, then (on the next 16-byte boundary) of b, allocated by the first mark.
  vv::AbsRec* stat_rec = nullptr;
  float* upd_shadow = nullptr;
  bool upd_marked = false;                  // the shadow holds the parameters of a vv_debug_mark_update (vv_params_set clears it)
  // vv_ema_set (the exponential moving average of the parameters; this project's own): < 0 off; sticky.  ONE allocation made by the
  // activation (and again by a vv_params_set of another D), never on the step path: eW [D][F], eb [D] on the next 16-byte boundary, the
  // average's own Scales block, its 16-bit copy eWh [Dp][Fp].  While active every finish_update queues k_ema behind the update.
  float ema_decay = -1.f;
  float *eW = nullptr, *eb = nullptr; vv::Scales* escales = nullptr; uint16_t* eWh = nullptr;
  bool ema_packed = false;                  // eWh / escales are those of the average as it stands (k_ema and a re-initialisation clear it)
  bool ema_in_use = false;                  // vv_ema_use(1): the forward-only readers take eWh / eb / escales; everything that trains refuses
  int64_t ema_updates = 0;                  // k_ema launches since the activation
  uint16_t* Wh = nullptr; vv::Scales* scales = nullptr; float* wmax_blocks = nullptr;
  int n_cu = 256;                           // compute units of the device
  bool scale_pending = false;               // k_sgd ran, its scale update has not (it rides in the next k_reduce)
  // wmax_blocks holds two buffers of WMAX_SLOTS per-block maxima: an update writes the one the previous update did not
  int wmax_cur = 0, wmax_n = 0;             // the buffer the latest update wrote, and how many slots of it
  bool wmax_seed_live = false;              // Scales::wmax_bits still carries vv_params_set's seed (the next scale update consumes it)
  // Where the last backward pass left its gradient, and whether an overlapped update has been joined (vv_step_state.h: written through
  // its transitions only).  red_args: the reduction of a gradient kept in the slabs; upd_wgrad_blocks: the per-block max |w| slots the
  // weight-gradient GEMM wrote when it applied the update itself.
  vv::GradState grad; vv::UpdSync upd_sync = vv::UpdSync::Joined;
  vv::ReduceArgs red_args; int upd_wgrad_blocks = 0;
  bool grads_exposed = false;               // vv_grads_device handed the buffer out: its holder may read it any time, so the reduction is eager from then on
  float* grads = nullptr;           // [D*F + D] (own buffer, or the bound external one)
  float* grads_own = nullptr;
  // per-batch buffers
  int B = 0, C = 0, Nn = 0, R = 0, Rp = 0;
  int32_t *idx_dev = nullptr, *rows = nullptr;
  float* H = nullptr; uint16_t* dYh = nullptr; float* dbp = nullptr;
  float *loss_part = nullptr, *viol_part = nullptr, *s_true = nullptr, *s_bogus = nullptr;
  float* coeff = nullptr; std::vector<float> coeff_host;
  float* item_w = nullptr;          // [B] loss-term weights of the current batch
  uint8_t* mask = nullptr; size_t mask_bytes = 0;
  float* slabs = nullptr; size_t slab_bytes = 0; int S = 1, kps = 0;
  int drop_dedup = 1;                       // option "drop_dedup" (VV_DROP_DEDUP): dropout rides the de-duplicated path -- 0 never, 1 on the register-resident shapes, 2 on every segment-path shape (score_fwd_dropout_supported)
  vv::DropSpec last_drop;                   // the last step's dropout on the de-duplicated path (mode 0: none): the blob accessors re-apply it
  float* loss2 = nullptr;           // {loss, violations}
  float sg = 1.f; float last_loss_weight = 1.f;
  uint64_t iter = 0;
  // row de-duplication (kernels_dedup.hip)
  int dedup = 1;                    // 1 = on whenever dropout is off (VV_DEDUP / vv_set_dedup)
  bool last_dedup = false;          // what the last forward/backward pass used
  // f16 gradient-scale guard (vv_internal.h: GradGuard)
  vv::GradGuard* gg = nullptr; float* gg_slots = nullptr; int gg_nslot = 0;
  unsigned long long* gg_bound = nullptr;      // GuardArgs::bound: the score kernel's (seq, largest per-instance element bound)
  unsigned long long* gmax_host = nullptr;     // pinned + mapped: GMAX_ENTRIES report entries of GMAX_ENTRY_WORDS words (vv_internal.h)
  unsigned long long* gmax_host_dev = nullptr;
  int sg_adj = 0;                   // powers of two on top of the count-based default scale (follows the reported maxima)
  int32_t gg_seq0 = 0;              // first step since the guard's state was reset (no reports older than that)
  int64_t gg_repeats = 0;           // steps whose gradients had to be produced again at a smaller scale
  int32_t gg_last_seq = 0;          // the last vv_forward_backward that ran with the guard (f16); 0: none ("last_grad_shift", ...)
  int gg_last_rounds = 0;           // ... and its guard rounds (0: the proactive form, which writes no shift[1])
  float gg_last_mul = 1.f;          // (debug accessors) final scale multiplier of the last step, read back on demand
  unsigned long long* dd_key = nullptr; int64_t dd_key_cap = 0;
  unsigned long long* dd_agg = nullptr; int dd_agg_stride = 0;
  int32_t *dd_slot_of = nullptr, *dd_uniq = nullptr, *dd_map = nullptr, *dd_ord = nullptr, *dd_cnt = nullptr,
          *dd_seg = nullptr, *dd_pos = nullptr, *dd_info = nullptr;
  uint16_t* dYu = nullptr;
  // segment-wise backward (vv_internal.h: SegRec)
  float* segV = nullptr; vv::SegRec* seg_rec = nullptr; float* seg_dbp = nullptr;
  bool seg_bwd = true;             // env VV_SEG_BWD=0: the per-instance gradient rows + k_segsum instead
  bool last_seg_bwd = false;
  bool slab16 = true;              // option "slab16" (VV_SLAB16=0: fp32): the weight gradient's split-K partial products as f16 x a power of two per (split, tile)
  float* slab_sc = nullptr;        // ... their inverse factors, [8][tiles]
  bool v16 = true;                 // option "v16" (VV_V16=0: fp32): the per-item vectors of the one-sweep score kernel (D = 1024) as f16, with h16
  bool h16 = true;                 // option "h16" (VV_H16=0: fp32 rows): ip2 as f16 between the forward GEMM and the segment-wise pair (FwdArgs::h16)
  bool last_h16 = false;           // ... and whether the last forward pass stored it that way (the accessors read H accordingly)
  // option "h16_guard" (VV_H16_GUARD): the f16 rows' range loss -- 0 off, 1 counted and reported (vv_h16_stats), 2 also falls back to fp32 rows
  int h16_guard = 1;
  uint32_t* h16_cnt = nullptr;     // [SEGB_BLOCKS][2] k_seg_bwd_cnt's per-workgroup {saturated elements, faint rows} of the last counted step
  bool last_h16_counted = false;   // the last forward/backward pass counted
  int32_t h16_counted[vv::GMAX_ENTRIES];     // [seq & 15] == seq: step seq counted, its report entry is due kLag steps later (INT32_MIN: none)
  int64_t h16_flagged_steps = 0, h16_first_flagged = -1;   // as read from the ring; the first flagged step's number
  int64_t h16_flag_step = -1, h16_flag_sat = 0, h16_flag_faint = 0;   // the step whose report started the fallback (with none: the first flagged one) and its two counts
  bool h16_fallback = false;       // guard 2 switched this context to fp32 rows (until option "h16" is set again)
  int32_t h16_arm_seq = 0;         // reports of steps up to this sequence number start no fallback (the guard was re-armed after them)
  vv::ScoreArgs last_score;            // to rebuild the per-instance gradient rows for vv_blobs_get(ip1_diff)
  int32_t* U_host = nullptr;        // pinned + mapped: k_dd_leaders stores U here every step, the launcher reads it late
  int32_t* U_host_dev = nullptr;    // device alias of U_host
  uint32_t dd_epoch = 0;
  // The grouping kernels of step k+1 run on a stream of their own while step k is still executing (they need only the
  // indices): four sets of their output arrays rotate (dd_* above point at the set of the step being issued), the forward
  // GEMM's sequence stamp says when the step that read a set is over, an event per set when its grouping is done.
  static constexpr int kDdSets = 4;
  // ... and one more set that never rotates, for the forward-only pass (vv_forward): a training step's set -- which its pending reduction
  // still names (ReduceArgs::gcnt) -- is never the one an evaluation pass regroups, however many passes run between two steps
  static constexpr int kDdEval = kDdSets, kDdAll = kDdSets + 1;
  struct DdSet {
    int32_t *rows = nullptr, *slot_of = nullptr, *uniq = nullptr, *map = nullptr, *ord = nullptr, *cnt = nullptr, *seg = nullptr,
            *info = nullptr;
    hipEvent_t done = nullptr; int32_t used_seq = 0;      // sequence number of the step that last read the set
  } dd_set[kDdAll];
  int32_t* dd_info_all = nullptr;
  int32_t* dd_rows = nullptr;      // instance -> table row of the current set (k_dd_claim's output)
  hipStream_t dd_stream = nullptr;
  uint64_t dd_step = 0;
  double dd_spin_us = 60.0;        // how long the host watches the grouping's event before queueing a stream wait (VV_DEDUP_SPIN_US)
  bool dd_async = true;            // env VV_DEDUP_ASYNC=0: the grouping kernels in the step's own stream
  int32_t step_seq = 0;
  // staging of index batches taken from a sampler's prefetch ring (vv_forward_backward_ring)
  static constexpr int kStage = 8;
  int32_t* stage_host[kStage] = {};         // pinned, mapped into the device's address space
  int32_t* stage_dev[kStage] = {};          // the device's alias of the same memory
  int32_t stage_seq[kStage] = {};           // sequence number of the step that last read the slot
  size_t stage_bytes = 0; int32_t stage_next = 0;
  // The forward-only evaluation pass (vv_forward) owns: its loss / violation partials (per batch shape; the training step's are pending
  // until its reduction runs), the record vv_eval_stats reads, the grouping set above with an event that says when the pass that read it
  // is over, and two pinned index staging buffers of its own (the training slots are released by sequence stamps a pass does not take)
  float *eval_loss_part = nullptr, *eval_viol_part = nullptr;
  vv::EvalRec* eval_rec = nullptr;
  bool last_fwd_only = false;               // the last forward pass was vv_forward's: the accessors of backward values refuse
  hipEvent_t ev_eval = nullptr; bool eval_set_used = false;
  static constexpr int kEvalStage = 2;
  int32_t* eval_stage_host[kEvalStage] = {}; int32_t* eval_stage_dev[kEvalStage] = {};
  hipEvent_t eval_stage_done[kEvalStage] = {}; bool eval_stage_busy[kEvalStage] = {};
  size_t eval_stage_bytes = 0; int eval_stage_next = 0;
  int32_t* seq_host = nullptr;              // pinned + mapped, two words.  [0]: the forward GEMM stores the step's sequence
  int32_t* seq_host_dev = nullptr;          //   number here when it starts, i.e. "the kernels that read this step's index
                                            //   batch have finished"; [1]: the score kernel does when IT starts, i.e. "this
                                            //   step's forward GEMM has finished" (the gate of the asynchronous grouping)
  // data-parallel gradient exchange (comm.hip)
  vv::Comm* comm = nullptr;
  bool comm_overlap = false;        // the update runs F-chunk by F-chunk on the communication stream (all-reduce, SGD, publish) and
                                    // the NEXT step's forward GEMM waits per chunk inside the kernel (FwdArgs::gate)
  // per-context switches (vv_set_option; environment read once, in vv_create).  Nothing of this is process-global.
  vv::KernelOpts ko;                // which kernels the launchers pick (vv_internal.h)
  bool fuse_update = true;          // "fuse_update" / VV_FUSE_UPDATE=0: reduce at the end of every backward pass, update apart
  bool comm_gate = true;            // "comm_gate" / VV_COMM_GATE=0: the overlapped update never gates the forward GEMM (the stream joins)
  // vv_update_hint: the next vv_forward_backward* is followed by vv_apply_update with these solver parameters and nothing reads the gradient
  // in between -- with one split of K the weight-gradient GEMM then applies the update itself (WgradUpd)
  bool upd_hint = false;
  bool wgrad_update = true;                 // option "wgrad_update" (VV_WGRAD_UPDATE): a hinted step with one split of K applies its update in the weight-gradient
                                            // GEMM's epilogue.  ON since the epilogue walks its row groups in an order that depends on the tile (k_wgrad_gemm_ph, UPD):
                                            // before that, two processes in sixteen ran it at half speed (182-196 us instead of 100-125), decided by where the buffers
                                            // happened to lie in physical memory; with it forty processes in forty at 95-107 us: 0.211-0.224 ms per iteration at the
                                            // shipped shape against 0.229-0.236 with the update as its own launch (profiles/r05_shipped_update.txt).
  vv_step_cfg upd_cfg;
  uint32_t* lab_score_ts = nullptr;         // (lab builds) device buffer of k_score_fwd's phase stamps, pass.hip
  bool comm_inline = true;                  // option "comm_inline" (VV_COMM_INLINE): the sharded update queued on the compute stream itself (no second stream, no gate)
  int nearest_select_min_k = 33;    // "nearest_select_min_k" / VV_NEAREST_SELECT_MIN_K: vv_gallery_nearest* use the selection form from this k on (1 .. 33)
  // vv_classification_stats: "cls_pass_tiles" (positive tiles of one counting launch, 1 .. 65535) and "cls_block_cols" (columns of one
  // block at most; 0: as many as the scratch limit admits) -- both exist so that the tests reach several passes / blocks at small shapes;
  // then what the last call ran (read-only "last_cls_*")
  int cls_pass_tiles = 16384, cls_block_cols = 0;
  int last_cls_passes = 0, last_cls_segments = 0, last_cls_blocks = 0;
  double last_cls_row_ms = 0, last_cls_count_ms = 0;
  // the linear classifier (linear.hip): "lin_split_rows" (rows of one split of the weight-gradient product; 0: the library's plan) -- it
  // exists so that the tests reach several splits and row blocks at small shapes; then what the last call ran (read-only "last_lin_*":
  // the splits of the largest row block, the row blocks of one batch, the four legs' device time in the last step of the last fit)
  int lin_split_rows = 0;
  int last_lin_splits = 0, last_lin_blocks = 0;
  int last_lin_gather = 0;          // "last_lin_gather": the form of the last batch's two products -- 0: none yet, 1: contiguous rows, 2: rows gathered by a list
  double last_lin_ms[4] = {0, 0, 0, 0};
  // k_hinge: "last_hinge_form" (1: 16-byte accesses, 2: element-wise, 0: not launched yet) of the last launch, and the rows with a
  // logit that is not finite in the last vv_op_hinge_loss ("last_hinge_nonfinite"); under the hinge loss the fit's second leg
  // ("last_lin_softmax_ms") is k_hinge's device time
  int last_hinge_form = 0;
  int64_t last_hinge_nonfinite = 0;
  int last_knn_form = 0;            // k_knn_vote: "last_knn_form" (1: 16-byte stores, 2: element-wise, 0: not launched yet) of the last launch
  // vv_gallery_kmeans (kmeans.hip): "km_block_rows" (rows of one score block; 0: the plan's choice, vv_kmeans_plan.h) -- it exists so
  // that the tests reach several blocks at small shapes; then what the last call ran (read-only "last_km_*": the blocks of one pass, the
  // chunks of the last update, k_km_assign's form -- 1: 16-byte accesses, 2: element-wise --, the four legs' device time in the last iteration)
  int km_block_rows = 0;
  int last_km_blocks = 0, last_km_chunks = 0, last_km_assign_form = 0;
  double last_km_ms[4] = {0, 0, 0, 0};
  // vv_ivf_search / vv_ivfpq_search (ivf_coarse.hip): "ivf_block_rows" (query rows of one block) and "ivf_grid_wgs" (workgroups of the grouped similarity's fixed
  // grid); 0: the plan's choice, vv_ivf_plan.h -- they exist so that the tests reach several blocks, and more tiles than workgroups, at
  // small shapes.  What the last search ran is the index's own (vv_ivf_get)
  int ivf_block_rows = 0, ivf_grid_wgs = 0;
  int comm_test_delay_us = 0;       // "comm_test_delay_us" / VV_COMM_TEST_DELAY_US: TEST HOOK -- the communication stream held this long per chunk
  // (lab) -- settable in a -DVV_LAB build only
  bool guard_proactive = true;      // VV_GUARD_PROACTIVE=0: the repeat form of the gradient-scale guard on the segment-wise path too
  bool fuse_keep_grads = false;     // VV_FUSE_KEEP_GRADS=1: the fused update also writes dW out
  bool comm_skip_ar1 = false;       // VV_COMM_SKIP_AR1=1: no collective call at world 1 (diagnosis)
  int dd_gate_word = 0;             // VV_DEDUP_GATE=1: the grouping is released by the score kernel's stamp
  int dd_lds_kb = -1;               // VV_DEDUP_LDS_KB: dynamic LDS the grouping kernels ask for (placement)
  double trace_host_ms = -1.0;      // VV_TRACE_HOST: report ABI calls that keep the host longer than this
  bool trace_waits = false;         // VV_TRACE_WAITS: where the host waits
  double wait_ms[5] = {0, 0, 0, 0, 0}; long wait_calls = 0;
  // SHARDED update (vv_comm_schedule 2): fp32 reduce-scatter of the shard-major [dW rows | db entries] buffer, the solver's rule on this
  // rank's D / world rows of W / history / bias, all-gather of the 16-bit copy + the bias + the per-block maxima that every rank's next
  // forward pass reads.  The fp32 master W and the history are complete only on their owner until vv_params_get gathers them.
  bool comm_sharded = false;
  bool params_partial = false;      // W / hW / hb rows of the other ranks' shards are stale (a sharded update ran since the last gather)
  int32_t upd_seq = 0;              // sequence number of the last overlapped update (what w_gate[c] reaches when chunk c is done)
  int32_t* w_gate = nullptr;        // device [W_CHUNKS_MAX * W_GATE_STRIDE]: one flag per 128-B line
  int n_chunks = 3;                 // F-chunks of the overlapped update (env VV_COMM_CHUNKS, 1 .. 4)
  int chunk_kt[5] = {0, 0, 0, 0, 0};    // first K-tile of each chunk for the current Fp (vv_chunk_plan)
  int32_t* pub_count = nullptr;     // device: arrival counter of the publishing SGD kernels (behind the flags)
  hipEvent_t ev_chunk0 = nullptr;   // the first F-chunk's reduction is done (recorded by fb_impl: GradBuffer::chunk0_event)
  int32_t* gate_err = nullptr; int32_t* gate_err_dev = nullptr;     // pinned + mapped: a gated forward gave up waiting
  hipEvent_t ev_chunk = nullptr;
  hipEvent_t ev_idx = nullptr;      // orders the grouping stream behind caller-produced device indices (idx_on_device = 1)
  // profiling
  bool prof = false;
  int prof_every = 1;               // record every prof_every-th forward/backward + update (vv_profile_enable's argument)
  uint64_t prof_calls = 0;
  std::map<std::string, ProfEntry> prof_map;
  std::string prof_only;            // vv_profile_select: ",name,name," -- only these kernels are timed (empty = all)
  std::vector<hipEvent_t> ev_pool; size_t ev_used = 0;    // events are reused across profiling sessions
};

// ops.hip keeps per-context scratch for the per-layer INNER_PRODUCT operators; vv_destroy releases it
void vv_ops_release(vv_ctx* c);
// api.hip: orders the compute stream behind an overlapped parameter update still on the communication stream
int vv_comm_join(vv_ctx* c);
// pass.hip: the reduction a backward pass left undone (GradAt::Slabs), now -- the gradient to the buffer, the loss to its scalars
int vv_reduce_now(vv_ctx* c);
// pass.hip: VV_ERR_STATE where the gradient's state refuses the entry point `who` (vv_step_state.h: grad_guard)
int vv_upd_pending_guard(vv_ctx* c, const char* who);
// api.hip: the embeddings of n table rows / of the (coefficient-weighted) means of n windows of k rows into dout [n][D]; `who` names the
// entry point in messages (retrieval.hip: vv_gallery_from_table)
int vv_embed_rows_device(vv_ctx* c, const char* who, const int32_t* rows, int64_t n, int relu, int l2norm, float* dout);
int vv_embed_mean_device(vv_ctx* c, const char* who, const int32_t* rows, int64_t n, int32_t k, const float* coeff, int relu, int l2norm,
                         float* dout);
// pass.hip: a step configuration the library can run, with the context's vv_solver_ext_set values where the rule reads them
int vv_check_cfg(vv_ctx* c, const vv_step_cfg* cfg);
// pass.hip: the per-batch buffers for this shape (a new shape starts the gradient scale's steering and the distinct-row hints afresh), and
// their release (vv_destroy, another D)
int vv_ensure_batch(vv_ctx* c, int B, int C, int Nn);
void vv_free_batch(vv_ctx* c);
// pass.hip: at least `need` scratch rows behind the table's zero row (quirk-Q1 composites, vv_embed_mean's window means)
int vv_ensure_scratch_rows(vv_ctx* c, int64_t need);
// pass.hip: the F-chunks of the overlapped update into c->chunk_kt; returns their number
int vv_chunk_plan(vv_ctx* c);
// api.hip: a sharded update's rows of W and the histories gathered from their owners (a collective)
int vv_gather_params(vv_ctx* c);
// api.hip: arm / collect a pair of timing events around the launcher called in between (PROFILED)
void vv_prof_begin(vv_ctx* c, const char* name, hipEvent_t* e0, hipEvent_t* e1);
void vv_prof_end(vv_ctx* c, const char* name, hipEvent_t e0, hipEvent_t e1);
// VV_TRACE_HOST=<ms>: report every launcher call that keeps the HOST longer than that (first use of a kernel variant,
// a runtime pool growing, ...) -- the GPU queue runs dry behind such a call.
inline double host_now_ms() {
  timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
#define PROFILED(c, name, call)                 \
  do {                                          \
    hipEvent_t e0_, e1_;                        \
    vv_prof_begin(c, name, &e0_, &e1_);         \
    const double th_ = (c)->trace_host_ms >= 0 ? host_now_ms() : 0.0; \
    call;                                       \
    if ((c)->trace_host_ms >= 0) { const double d_ = host_now_ms() - th_; if (d_ > (c)->trace_host_ms) fprintf(stderr, "[vv host] %s: %.3f ms (call %llu)\n", name, d_, (unsigned long long)c->iter); } \
    vv_prof_end(c, name, e0_, e1_);             \
  } while (0)
// what every entry point that trains or replaces the parameters says under vv_ema_use(1)
inline constexpr const char* kEmaInUse = "the averaged parameters are in use (vv_ema_use(1)): this call trains or replaces the parameters -- vv_ema_use(0) first";
// solver.hip: the solver's parameters of a step as the update kernels read them; the seed of vv_params_set cleared behind a launch that
// consumed it; the moving average's allocation and start, and its release
vv::SolverRule vv_solver_rule(const vv_step_cfg& cfg, float momentum2, float rms_decay, int64_t t = 0);
hipError_t vv_clear_wmax_seed(vv_ctx* c, bool consumed, hipStream_t s);
int vv_ema_init(vv_ctx* c);
void vv_ema_release(vv_ctx* c);
// solver.hip: what the forward-only readers (vv_forward, vv_embed, vv_embed_mean, vv_gallery_from_table) read: the training parameters'
// 16-bit copy, bias and scales, or under vv_ema_use(1) the average's (packed on demand, on the context's stream)
struct ParamView { const uint16_t* Wh; const float* b; const vv::Scales* scales; };
int vv_param_view(vv_ctx* c, ParamView* v);
// solver.hip: why no schedule but sync can be chosen now -- the message of the first active feature among gradient clipping, the gradient
// bank and the moving average -- or nullptr
const char* vv_sync_only_feature(const vv_ctx* c);
// kmeans.hip: vv_gallery_kmeans' body on device rows that need not be a gallery's (pq.hip: a column slice of one), bit for bit the same
// call; assign_dev_out: NULL, or device [n_ref] that takes a copy of the final assignment without a host round trip
int vv_kmeans_rows(vv_ctx* c, const vv::GalleryRows& gr, const vv_kmeans_cfg* cfg, const float* init_centroids, const int32_t* init_rows,
                   float* centroids_out, int32_t* assign_out, int32_t* counts_out, double* objective_trace, int64_t* moved_trace,
                   vv_kmeans_report* out, int32_t* assign_dev_out);
