/*
 * videovec.h -- C ABI of the MI355X-native videovec_embedding training path.
 *
 * The reference (eevignesh/videovector, a Caffe fork) has no FFI: its boundary for this path is the
 * C++ Layer / Solver class hierarchy.  This ABI is what a drop-in replacement of that path binds
 * to; every entry point names the reference interface it replaces (paths relative to the
 * reference root).  INTEGRATION.md shows the reference-side stubs (a Layer subclass, ctypes).
 *
 * Conventions: plain pointers and sizes, no C++ or torch types.  Every function returns VV_OK (0)
 * or a VV_ERR_* code; vv_last_error() gives the thread's last message.  Nothing throws across the
 * boundary.  "host" pointers are ordinary CPU memory; the context owns all device memory.
 * Errors the reference reports with CHECK/LOG(FATAL) (abort) are reported here as VV_ERR_ARG.
 */
#ifndef VIDEOVEC_H_
#define VIDEOVEC_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vv_ctx vv_ctx;

enum { VV_OK = 0, VV_ERR_ARG = 1, VV_ERR_HIP = 2, VV_ERR_STATE = 3, VV_ERR_NOGPU = 4 };

/* MFMA operand type of the two GEMMs (accumulation is always fp32). */
enum { VV_PREC_F16 = 0, VV_PREC_BF16 = 1 };

/* Loss norm: MaxMarginLossParameter.Norm (src/caffe/proto/caffe.proto:858-863). */
enum { VV_NORM_L1 = 1, VV_NORM_L2 = 2 };
/* SolverParameter.regularization_type (caffe.proto:130-132). */
enum { VV_REG_L1 = 1, VV_REG_L2 = 2 };
/* SolverParameter.solver_type (caffe.proto SolverType: SGD, NESTEROV, ADAGRAD).  RMSPROP and ADAM carry BVLC Caffe's numbers
 * (its caffe.proto SolverType: RMSPROP = 3, ADADELTA = 4, ADAM = 5); the reference tree has neither solver.  4 is not implemented. */
enum { VV_SOLVER_SGD = 0, VV_SOLVER_NESTEROV = 1, VV_SOLVER_ADAGRAD = 2, VV_SOLVER_RMSPROP = 3, VV_SOLVER_ADAM = 5 };

/* One context per process / GPU.  Replaces Caffe::SetDevice + Caffe::set_mode(GPU)
 * (src/caffe/common.cpp:127-145, tools/caffe.cpp:92-104). */
int vv_create(int device, int prec, vv_ctx** out);
/* Caffe::DeviceQuery (src/caffe/common.cpp:147-180): a text description of the device (name, architecture, compute
 * units, clocks, memory, LDS / registers per block) into buf (NUL-terminated, truncated to n). */
int vv_device_query(int device, char* buf, size_t n);
int vv_destroy(vv_ctx* ctx);
const char* vv_last_error(void);
const char* vv_version(void);
/* Run all kernels of this context on an existing hipStream_t (NULL = the context's own stream).
 * The reference has only the default CUDA stream. */
int vv_set_stream(vv_ctx* ctx, void* hip_stream);
int vv_synchronize(vv_ctx* ctx);
/* Row de-duplication (default on; also VV_DEDUP=0/1 in the environment).  The reference sampler draws
 * every item's negatives from one shared buffer (video_sampled_shots_data_layer.cpp:836-875), so the
 * (C+Nn)*B rows of a batch repeat table rows.  With de-duplication the fc projection
 * (InnerProductLayer::Forward, inner_product_layer.cu:12-27) runs once per distinct row and the gradient rows of
 * a row's instances are summed before the weight-gradient product (inner_product_layer.cu:36-42): the same
 * sums, reassociated.  Steps with dropout always take the dense path.  vv_dedup_stats reports the rows of
 * the last forward/backward pass and how many were distinct (rows == unique_rows on the dense path).  A forward-only pass (vv_forward)
 * is a forward pass: until the next vv_forward_backward* vv_dedup_stats reports ITS batch. */
int vv_set_dedup(vv_ctx* ctx, int on);
/* Per-context execution switches by name; none of them changes a result beyond rounding, none is process-global (two contexts
 * of one process keep their own).  Each also has an environment variable that sets its INITIAL value when the context is
 * created.  The reference's counterpart is Caffe::set_mode / the layer's *_param fields (include/caffe/common.hpp:108-135):
 * per-object configuration, not globals.
 *   "dedup" (VV_DEDUP, 1)            row de-duplication, as vv_set_dedup
 *   "seg_bwd" (VV_SEG_BWD, 1)        segment-wise backward of de-duplicated batches (0: per-instance gradient rows + their sums)
 *   "drop_dedup" (VV_DROP_DEDUP, 1)  on which shapes a dropout step stays de-duplicated (the score and segment kernels carry per-instance masks over the
 *                                    shared pre-dropout rows): 0 none -- dense, the mask in the forward GEMM's epilogue; 1 the shapes of the
 *                                    register-resident score kernel (D = 512, up to 55 negatives and 6 context rows); 2 every shape of the
 *                                    segment-wise path (D = 512 or 1024; the one-sweep score kernel and the two-chunk segment backward; dropout
 *                                    steps then run with "v16" off).  All three drop the same elements.  Any other value: VV_ERR_ARG (an invalid
 *                                    VV_DROP_DEDUP leaves the default)
 *   "h16" (VV_H16, 1)                ip2 stored as f16 between the forward GEMM and the segment-wise score / backward kernels (de-duplicated batches
 *                                    of D = 512 / 1024): half the bytes of the GEMM's epilogue and of every later read of a row; adds one f16 rounding
 *                                    (2^-12 relative per element; values past 65504 saturate) to the embeddings the loss is computed from --
 *                                    measured against the fp32 oracle on whole batches: rows 2.7e-4 -> 3.5e-4, scores 3.8e-5 -> 5.3e-5, loss
 *                                    unchanged to 1e-6 (inside the 1e-3 the path is held to); 0: fp32 rows (the rounds 1-5 form)
 *   "h16_guard" (VV_H16_GUARD, 1)    what watches those f16 rows' range (vv_h16_stats below): 0 nothing -- the kernels of the step are the ones without
 *                                    the option; 1 the segment-wise backward counts, per step, the saturated elements and the faint rows of the
 *                                    distinct rows it holds and the step reports them (no value of the step changes: dW, db, loss and W are
 *                                    bit-identical to 0); 2 also falls back: once the report of a step shows either count non-zero, every later
 *                                    step stores fp32 rows, exactly the execution of "h16" 0 (and "v16" with it), until "h16" is set to 1 again.
 *                                    Steps on fp32 rows (dense, other D, "h16" 0) count nothing.  Any other value: VV_ERR_ARG
 *   "slab16" (VV_SLAB16, 1)          the weight gradient's split-K partial products as f16 x one power of two per (split, 256 x 256 tile) instead of
 *                                    fp32 (half of the 134 MB they cost per step at the benchmark's shape; a second rounding, 2^-12 relative per
 *                                    partial product, in the gradient path -- every split still accumulates in fp32 and the sum over the splits is
 *                                    taken in fp32: dW against the oracle on the same operands 3.5e-4 -> 4.6e-4 on whole batches); 0: fp32 slabs
 *   "v16" (VV_V16, 1)                with h16, D = 1024 (the one-sweep score kernel: hundreds of negatives per item): the two per-item vectors the
 *                                    segment-wise backward gathers once per instance stored as f16 (one more 2^-12 in the gradient)
 *   "score_pf" (VV_SCORE_PF, 1)      the register-resident score kernel's first-round workgroups request the second round's rows into the XCD's L2
 *                                    while they compute (bit-identical results)
 *   "fuse_update" (VV_FUSE_UPDATE, 1) reduction of the split-K partials and the solver update in one launch (0: two launches)
 *   "fwd_lead" (VV_FWD_LEAD, 1)      the forward GEMM's sibling lead
 *   "wgrad_tr" (VV_WGRAD_TR, 1)      transposed LDS reads in the weight-gradient GEMM (0: the first-round kernel)
 *   "wgrad_lean" (VV_WGRAD_LEAN, 1)  the weight-gradient GEMM's lean instantiations (tables below 4 GiB: gathered rows addressed as base + 32-bit
 *                                    offset, fewer instructions in the loop's LOAD segments; bit-identical results); 0: 64-bit addresses
 *   "comm_gate" (VV_COMM_GATE, 1)    the overlapped update gates the next forward GEMM chunk by chunk (0: the stream joins)
 *   "comm_inline" (VV_COMM_INLINE, 1)  the SHARDED update's three steps (reduce-scatter, the rule on this rank's rows, all-gather) are queued
 *                                    on the compute stream itself (0: on the communication stream, the next forward GEMM gated on one flag)
 *   "wgrad_update" (VV_WGRAD_UPDATE, 1)  a step announced by vv_update_hint whose weight-gradient GEMM has one split of K applies the solver's
 *                                    rule in that GEMM's epilogue (bit-identical parameters; 0: the update as its own launch)
 *   "comm_chunks" (VV_COMM_CHUNKS, 3)  F-chunks of the overlapped update, 1 .. 4
 *   "comm_test_delay_us" (VV_COMM_TEST_DELAY_US, 0)  TEST HOOK: holds the communication stream this long in front of every chunk
 *   "nearest_select_min_k" (VV_NEAREST_SELECT_MIN_K, 33)  vv_gallery_nearest*: the smallest k that runs the selection form; 1 .. 33, anything
 *                                    else is VV_ERR_ARG.  1 runs the selection form at every k (how the tests hold the two forms against each other)
 * Read-only values (vv_get_option only; vv_set_option: VV_ERR_ARG) -- what the launchers chose for the most recent launch on this context,
 * recorded where the kernel is launched, for tests that must know which form they exercised:
 *   "last_fwd_tile_rows"             rows of the forward GEMM's tile, 128, 192 or 256, whoever launched it (a step, vv_embed*, vv_op_inner_product,
 *                                    vv_gallery_from_table); 0 before the first launch
 *   "last_wgrad_splits"              splits of K (S) of the weight-gradient GEMM (a step or vv_op_inner_product_bwd); 0 before the first launch
 *   "last_update_form"               what the last vv_apply_update ran for the parameter matrix: 1 k_sgd with 16-byte accesses (the chunked and sharded updates too), 2 k_sgd scalar (F % 4 != 0), 3 k_reduce_sgd, 4 k_reduce_sgd over f16 slabs, 5 the weight-gradient GEMM's epilogue; 0 before the first update.
 *                                    While gradient clipping is active (vv_clip_gradients_set >= 0) every update is 1 or 2: the fused forms 3 - 5 are not used;
 *                                    so is every update of banked gradients (vv_grads_bank)
 *   "last_score_form"                what the last forward pass launched for scores and loss: 1 k_score_fwd (register-resident), 2 k_score_stream at
 *                                    D = 512, 3 k_score_stream at D = 1024, 4 the per-instance kernels (dense or row-writing execution); 0 before the first step
 *   "last_h16"                       1: the last forward pass stored ip2 as f16 rows, 0: fp32 rows (or no step yet)
 *   "last_grad_shift", "last_grad_shift_round1", "last_grad_repeat"   the f16 gradient-scale guard after the last vv_forward_backward: the powers
 *                                    of two the device took off the host's scale in the end (signed: the segment-wise backward shifts both ways)
 *                                    and in the first guard round (meaningful where the step had two; 0 behind the segment-wise backward), and 1 if a conditional repeat really ran
 *                                    in that step.  0 for bf16 and before any step.  Reading them synchronises the stream (48 bytes are copied)
 *   "h16_fallback"                   1: "h16_guard" 2 has switched this context to fp32 rows (vv_h16_report::fallback, without synchronising);
 *   "h16_flagged_step", "h16_flagged_saturated", "h16_flagged_faint_rows"   the step whose report started that fallback -- with none, the first
 *                                    flagged step -- and its two counts (-1, 0, 0: none flagged so far)
 * Retired options -- "fwd_merge", "score_stream", "comm_first_inline": their alternatives were measured, lost and removed.  They read as 0,
 * the value the library always runs with; setting 0 is accepted, any other value is VV_ERR_ARG.  Their environment variables are not read.
 * Ablated / experimental kernels (timing studies whose results may be wrong) are NOT reachable through this library: they and their
 * switches exist only in the lab build (make -C videovector_amd/csrc lab).  Unknown name: VV_ERR_ARG. */
int vv_set_option(vv_ctx* ctx, const char* name, double value);
int vv_get_option(vv_ctx* ctx, const char* name, double* value);      /* ... and their current values */
int vv_dedup_stats(vv_ctx* ctx, int64_t* rows, int64_t* unique_rows);
/* Range loss of the f16 ip2 rows (option "h16": rows stored at scale 1, values past 65504 saturated by the forward GEMM's epilogue).  With
 * "h16_guard" >= 1 the segment-wise backward counts, over the distinct rows of the step (each once, however often the batch repeats it):
 *   saturated   elements whose stored f16 value is 65504, the largest finite one.  ip2 is post-ReLU, so >= 0; a true value in
 *               [65488, 65504) rounds to 65504 and is counted too (conservative).
 *   faint_rows  rows whose largest element is > 0 and < 2^-14, the smallest normal f16: every element is subnormal and the normalised
 *               embedding keeps fewer than 11 significant bits.  An all-zero row (index -1 with zero bias, a row dead behind the ReLU) is not faint.
 * The counts ride in the step's report to the host, which reads the report of step s when it issues step s + 4 (a fixed lag: what the
 * reports steer is bit-reproducible, and a host running ahead is never stalled).  flagged_steps / first_flagged_step (steps count from 0,
 * one per vv_forward_backward*) are therefore up to four steps behind, and under "h16_guard" 2 the four steps from the flagged one on have
 * still trained on f16 rows before the fallback holds: nothing is redone.  With f16 and with bf16 operands alike (the rows are f16 in both).
 * "h16_guard" 0, or a step on fp32 rows: both counts 0.  Library default 1; the Solver of the Caffe facade runs its engine with 2.
 * A forward-only pass (vv_forward) counts nothing and is no step: after one, saturated / faint_rows and the flagged fields still describe
 * the last TRAINING step; only rows_f16 (like "last_h16") describes the pass, until the next vv_forward_backward*. */
typedef struct { int64_t saturated, faint_rows;     /* of the LAST completed step (synchronises, like vv_dedup_stats) */
                 int64_t flagged_steps;             /* steps with either count non-zero since vv_create, as read from the ring */
                 int64_t first_flagged_step;        /* its step number, -1: none */
                 int32_t fallback;                  /* 1: guard 2 has switched this engine to fp32 rows */
                 int32_t rows_f16; } vv_h16_report; /* 1: the last forward pass stored f16 rows */
int vv_h16_stats(vv_ctx* ctx, vv_h16_report* out);
/* f16 operands: the 16-bit gradient operand of the weight-gradient product (InnerProductLayer::Backward,
 * inner_product_layer.cpp:80-97) carries one power-of-two scale per step.  A gradient value outside f16's range is never
 * applied clipped: the kernels that round gradients record their maxima, and a step whose values did not fit produces
 * them again at a smaller scale before the product runs (exact: powers of two).  `repeats` = steps so far that needed
 * that (as reported by the device, four steps late); `scale` = the scale the next step starts with. */
int vv_grad_scale_stats(vv_ctx* ctx, int64_t* repeats, float* scale);

/* ---- feature table: stands for the rows the data layer copies out of the VideoShots DB
 * (VideoSampledShotsDataLayer::AddSamplesToTop, src/caffe/layers/video_sampled_shots_data_layer.cpp:
 * 439-452, and BasePrefetchingDataLayer::Forward_gpu's H2D copy, base_data_layer.cu:7-21).  The
 * table stays resident in HBM; a batch is then just row indices.  rows: host fp32 [n_rows][F]. */
int vv_table_set(vv_ctx* ctx, const float* rows, int64_t n_rows, int32_t F);
/* Fill the table with the synthetic features of videovector_amd/synth.py (integer hashing only,
 * bit-identical to the host generator). */
int vv_table_synth(vv_ctx* ctx, uint64_t seed, int64_t n_rows, int32_t F);
/* Read rows back as fp32 (host [n][F]); rows == NULL means 0..n-1. */
int vv_table_get(vv_ctx* ctx, const int32_t* rows, int64_t n, float* out);

/* ---- fc7 parameters and SGD history.  InnerProductLayer blobs_[0] (1,1,D,F) row-major D x F and
 * blobs_[1] (1,1,1,D) (src/caffe/layers/inner_product_layer.cpp:29,36); SGDSolver::history_
 * (include/caffe/solver.hpp:79,91).  NULL history = zeros.  All host fp32. */
int vv_params_set(vv_ctx* ctx, int32_t D, const float* W, const float* b, const float* hW,
                  const float* hb);
int vv_params_get(vv_ctx* ctx, float* W, float* b, float* hW, float* hb);

/* ---- RMSProp and Adam: the parameters vv_step_cfg has no field for, the update count and the second history.  BVLC Caffe's
 * SolverParameter.momentum2 (field 39, default 0.999: Adam's beta2) and rms_decay (field 38, default 0.99); the reference tree's solver
 * (solver.cpp:485-781) knows neither.  Sticky on the context until set again; each range ([0, 1)) is checked by the calls that take a
 * vv_step_cfg of the solver that uses the value.  vv_update_hint's "exactly these solver parameters" includes them. */
int vv_solver_ext_set(vv_ctx* ctx, float momentum2, float rms_decay);
int vv_solver_ext_get(vv_ctx* ctx, float* momentum2, float* rms_decay);
/* The number of Adam updates applied so far: the next one is update t = count + 1 of AdamSolver::ComputeUpdateValue's
 * correction sqrt(1 - beta2^t) / (1 - beta1^t) (BVLC adam_solver.cpp: t = iter + 1).  Counts Adam updates only; vv_params_set puts it
 * back to 0; a restored run sets it to the snapshot's iteration. */
int vv_solver_iter_set(vv_ctx* ctx, int64_t count);
int vv_solver_iter_get(vv_ctx* ctx, int64_t* count);
/* Adam's second history (v; vv_params_set / _get's history holds m), shapes of W and b: BVLC AdamSolver keeps it in the second half of
 * SGDSolver::history_ (adam_solver.cpp: val_v = history_[i + update_history_offset]).  NULL = zeros; before the first Adam update it reads
 * as zeros.  vv_params_set clears it.  Host fp32; with the sharded update vv_history2_get gathers like vv_params_get (a collective). */
int vv_history2_set(vv_ctx* ctx, const float* vW, const float* vb);
int vv_history2_get(vv_ctx* ctx, float* vW, float* vb);

/* ---- the step's carried state, for a run that resumes bit for bit.  The reference's SGDSolver::SnapshotSolverState / RestoreSolverState
 * (src/caffe/solver.cpp:578-596, with Solver::Snapshot, :320-341) carry the iteration and the history; its step carries nothing else
 * from one iteration to the next.  This one does (a counter-based dropout mask, 16-bit operands with lagging power-of-two scales, report
 * rings read at a fixed lag), and these calls carry it: an opaque, versioned blob of what a training step reads that earlier steps left
 * and that vv_params_get, vv_history2_get, vv_solver_iter_get and vv_ema_get do not return --
 *   the dropout counter; the steps' sequence number; the W -> 16-bit scales (Scales: they follow max |W| one update late, where
 *   vv_params_set computes them from the values it is given), the per-block maxima the next scale update folds, and the 16-bit copy of W
 *   rounded at those scales; the gradient scale's adjustment and the report ring it is steered by; the f16 rows' guard (which reports are
 *   due, the fallback); the gradient guard's device record; the distinct-row hints that size the next forward GEMM's tiles.
 * Not carried: statistics counted since vv_create that no step reads (vv_clip_stats, vv_accum_stats, vv_eval_stats, vv_ema_stats's count).
 * Order on the resuming side: vv_params_set, vv_history2_set, vv_solver_iter_set (vv_ema_set / vv_ema_put), THEN vv_run_state_put --
 * vv_params_set resets part of this state.  Options (vv_set_option) and the table are the caller's to set up as they were.
 * vv_run_state_get synchronises.  Both return VV_ERR_STATE without parameters; while a backward pass's gradient waits for its
 * vv_apply_update (get), or any gradient is held (put: the context comes fresh from vv_params_set); while a step announced by
 * vv_update_hint is under way; while gradients are banked; while the overlapped or sharded schedule is selected or an update of theirs is
 * in flight; while the average is in use (vv_ema_use(1)).  vv_run_state_put: a blob of another version, D, F or operand type, a truncated
 * or over-long one: VV_ERR_ARG, nothing past `bytes` is read and the context is untouched. */
int vv_run_state_size(vv_ctx* ctx, int64_t* bytes);
int vv_run_state_get(vv_ctx* ctx, void* buf, int64_t cap, int64_t* written);
int vv_run_state_put(vv_ctx* ctx, const void* buf, int64_t bytes);

/* ---- gradient clipping by the global L2 norm: BVLC Caffe's SolverParameter.clip_gradients and SGDSolver::ClipGradients (sgd_solver.cpp);
 * the reference tree has no such function, so the semantics are BVLC's.  clip < 0 (the default, -1) disables it and a step is in every
 * respect what it was; clip >= 0 makes it active; NaN is VV_ERR_ARG.  Sticky on the context until set again.  In an active
 * vv_apply_update, before the regulariser and before any rule: sumsq = the sum of g^2 over the whole flat gradient buffer [dW (D F) | db (D)]
 * -- the values vv_grads_get would return at that moment: ip_regularization's factor included, summed over the ranks of a communicator --
 * accumulated in double in a fixed order (the same buffer gives the same bits on every run and every rank); norm = sqrt(sumsq); if
 * norm > clip (strictly; norm == clip and norm == 0 scale nothing, there is no division by zero) every element is multiplied in place
 * by scale = clip / norm (one fp32 multiply), else nothing is written.  vv_grads_get after the update returns the clipped gradient, as
 * BVLC's diff would.  Two kernels on the step's stream (k_grad_sumsq, k_grad_scale), no host synchronisation.
 * An active update brings the gradient into the buffer as a reader of the gradient would, and runs the plain k_sgd: "last_update_form" 1
 * or 2.  The fused forms 3 - 5 are not used, and vv_update_hint / vv_step do not announce the epilogue update for such a step ("where the
 * fusion does not apply the hint changes nothing"); vv_update_hint's "exactly these solver parameters" includes the threshold: a
 * vv_apply_update under another one than its hint announced is VV_ERR_ARG.  All five solver rules work.
 * Data parallel: on the sync schedule only -- the all-reduce finishes, then every rank runs the same two kernels on identical buffers.
 * VV_ERR_STATE: vv_clip_gradients_set(>= 0) while schedule 1 or 2 is selected, and vv_comm_schedule(1 or 2) / vv_comm_overlap(1) while
 * clipping is active. */
int vv_clip_gradients_set(vv_ctx* ctx, float clip);
int vv_clip_gradients_get(vv_ctx* ctx, float* clip);
/* What SGDSolver::ClipGradients would have logged (BVLC: "Gradient clipping: scaling down gradients (L2 norm X > Y) by scale factor Z"). */
typedef struct { float norm, scale;                 /* of the LAST completed clipping update (synchronises, like vv_dedup_stats): norm and scale each
                                                       formed in double and rounded once; scale is 1 where the step was not clipped.  0, 1 before the first */
                 int32_t clipped;                   /* 1: that update scaled its gradient */
                 int32_t reserved_;
                 int64_t updates;                   /* updates that computed a norm (clipping active) since vv_create */
                 int64_t clipped_updates; } vv_clip_report;     /* ... of which scaled their gradient */
int vv_clip_stats(vv_ctx* ctx, vv_clip_report* out);

/* ---- gradient accumulation: BVLC Caffe's SolverParameter.iter_size, Solver::Step (solver.cpp) and SGDSolver::Normalize (sgd_solver.cpp);
 * the reference tree has no iter_size, so the semantics are BVLC's.  BVLC's Step clears the diffs (Net::ClearParamDiffs), runs iter_size x
 * ForwardBackward with the layers adding into the diffs, divides the loss by iter_size and calls ApplyUpdate: ClipGradients on the SUM,
 * Normalize (diff *= Dtype(1) / iter_size), Regularize, the rule.  Here the sum is kept in a BANK: a second flat fp32 buffer
 * [dW (D F) | db (D)], allocated zero-filled by the first vv_grads_bank (the one allocation a step may make, never on the step path
 * afterwards).
 * vv_grads_bank: the layers' "add into the diff" (BVLC Solver::Step's accumulating Net::ForwardBackward).  Adds the gradient of the last
 * vv_forward_backward* -- the values vv_grads_get would return at that moment: ip_regularization's factor included, this rank's own
 * gradient, read from a bound buffer (vv_grads_bind) where one is bound -- into the bank.  The first bank of a cycle STORES (the bank is
 * not read: -0 stays -0), every later one computes bank = bank + g, one fp32 add per element, in banking order.  It also folds the last
 * forward pass's loss and violations into two fp32 sums on the device (the first bank stores, later ones add).  One kernel (k_grad_bank)
 * on the step's stream, no atomics, no host synchronisation; no parameter changes.
 * vv_grads_bank_reset: Net::ClearParamDiffs -- discards the bank and the two sums; vv_params_set does the same.
 * vv_apply_update with m >= 1 gradients banked (BVLC SGDSolver::ApplyUpdate), in this order: the bank is written into the flat gradient
 * buffer; with a communicator its all-reduce runs (ONE exchange per cycle); where clipping is active k_grad_sumsq / k_grad_scale run on
 * it (the norm is the SUM's); every element is multiplied by inv = 1.0f / (float)m, one fp32 multiply (SGDSolver::Normalize; without a
 * communicator and without clipping the write and the multiply are one pass); the regulariser and the rule run in the plain k_sgd:
 * "last_update_form" 1 or 2.  Afterwards vv_grads_get returns the normalised (and clipped) buffer, the bank is empty and a new cycle
 * starts; Adam's t has advanced by one.  With nothing banked vv_apply_update is in every respect what it was.
 * VV_ERR_STATE: vv_grads_bank before any backward pass, twice for one backward pass, after a step announced by vv_update_hint (its
 * gradient is not kept), after vv_allreduce_grads (the bank is exchanged once per cycle), or while schedule 1 or 2 is selected;
 * vv_comm_schedule(1 or 2) / vv_comm_overlap(1) while the bank is non-empty; vv_apply_update or vv_step while the bank is non-empty
 * and the last backward pass's gradient has not been banked.  vv_update_hint announces nothing while the bank is non-empty.  A second
 * vv_forward_backward* without banking simply replaces the gradient. */
int vv_grads_bank(vv_ctx* ctx);
int vv_grads_bank_reset(vv_ctx* ctx);
/* What BVLC's Solver::Step would display for an accumulated iteration (loss /= iter_size). */
typedef struct { int32_t banked;                    /* gradients in the bank now */
                 int32_t last_count;                /* the m of the LAST completed accumulated update (synchronises, like vv_clip_stats); 0 before the first */
                 float last_mean_loss;              /* that cycle's sums x inv = 1.0f / (float)m, one fp32 multiply each */
                 float last_mean_violations;
                 int64_t updates; } vv_accum_report;    /* accumulated updates since vv_create */
int vv_accum_stats(vv_ctx* ctx, vv_accum_report* out);

/* ---- magnitude statistics: the reference's SolverParameter.debug_info (caffe.proto field 23).  Net::ForwardDebugInfo, BackwardDebugInfo
 * and UpdateDebugInfo (net.cpp:580-636) print asum / count -- the mean absolute value -- of top blobs, bottom and parameter diffs and
 * parameters; Blob::asum_data / asum_diff (blob.cpp:138-165) are one caffe_gpu_asum each.  Here one kernel (k_abs_stats) measures up to
 * eight device buffers per launch on the step's stream and leaves one record per buffer; nothing is downloaded but the records.
 *   asum       the sum of |x| over the FINITE elements, accumulated in double in a fixed order (no atomics: the same buffer gives the
 *              same bits on every run)
 *   amax       the largest finite |x|
 *   nonfinite  the number of NaN and +-Inf elements; they count neither in asum nor in amax (the reference's asum would be NaN or Inf)
 *   count      the number of elements
 * The reference's printed value is (float)(asum / count). */
typedef struct { double asum; float amax; int32_t reserved_; int64_t count, nonfinite; } vv_abs_stat;
/* Blob::asum_data / asum_diff (blob.cpp:138-165; the lines of net.cpp:580-636 are built on them) without the download: the statistics of
 * n fp32 elements of DEVICE memory of this context (vv_dev_alloc), read as they are on the context's stream.  Synchronises.  n >= 1,
 * else VV_ERR_ARG. */
int vv_op_asum(vv_ctx* ctx, const float* x_dev, int64_t n, vv_abs_stat* out);
/* The tensors of the fused training step that vv_debug_stats_queue can measure. */
enum { VV_STAT_W, VV_STAT_B,                              /* the fp32 master parameters (net.cpp:616-626, "[Update] ... data") */
       VV_STAT_HIST_W, VV_STAT_HIST_B,                    /* the solver's (first) history */
       VV_STAT_DW, VV_STAT_DB,                            /* the gradient (net.cpp:604-612, "[Backward] ... param blob k diff") */
       VV_STAT_TARGET_SCORE, VV_STAT_NEGATIVE_SCORES,     /* the two score blobs (net.cpp:580-590, "[Forward] ... top blob B data") */
       VV_STAT_UPD_W, VV_STAT_UPD_B,                      /* what the last update subtracted (net.cpp:616-626, "[Update] ... diff") */
       VV_STAT_N };
/* vv_debug_stats_queue (Net::ForwardDebugInfo / BackwardDebugInfo / UpdateDebugInfo, net.cpp:580-636; Blob::asum_*, blob.cpp:138-165):
 * queues one k_abs_stats launch (two where mask names more than eight entries) on the step's stream for the entries named by mask
 * (bit VV_STAT_x), as they are at that point of the stream.  No host synchronisation; the record block is allocated by the first call
 * that measures and never on the step path afterwards.  The kernel only reads what it measures: with nothing queued a training step is
 * in every respect what it was, and parameters, histories, the 16-bit copy, loss and gradients of a run that queues statistics are bit
 * for bit those of one that does not.
 *   DW / DB     bring the gradient into the flat buffer as a reader of the gradient would (the lazy reduction of vv_grads_get): the values
 *               vv_grads_get would return at that moment -- after a clipping or accumulated update, the clipped / normalised buffer
 *   scores      the two score buffers of the last forward pass (vv_forward_backward* or vv_forward).  target_score is held once per item
 *               (count = B; the blob repeats each value num_negative_samples times, which changes neither the mean nor the maximum),
 *               negative_scores has B x Nn values
 *   UPD_W / _B  see vv_debug_mark_update
 * mask == 0 or a bit from VV_STAT_N on: VV_ERR_ARG.  VV_ERR_STATE: gradient entries before any backward pass; gradient entries for a step
 * announced by vv_update_hint (vv_step), between its backward pass and its update and after it -- that gradient is not kept; gradient entries
 * while the buffer is laid out for the overlapped or sharded schedule; parameter, history and UPD entries between a hinted backward pass
 * and its vv_apply_update (the parameters are half-way); score entries before any forward pass; UPD_* without a preceding
 * vv_debug_mark_update; W / history / UPD entries while the sharded schedule (2) is selected (the master copy is complete on its owner only). */
int vv_debug_stats_queue(vv_ctx* ctx, uint32_t mask);
/* Of the debug lines (net.cpp:580-636, over Blob::asum_*, blob.cpp:138-165) the "[Update] ... diff" one (Net::UpdateDebugInfo,
 * net.cpp:616-626, over Blob::asum_diff, blob.cpp:152-165) reads the diff blob,
 * which the solver has overwritten with the value Net::Update subtracts.  The update kernels here keep no such buffer, so the library
 * measures the subtraction itself: vv_debug_mark_update copies W and b into a shadow buffer, device to device on the step's stream (the
 * shadow is allocated by the first call and never on the step path afterwards); VV_STAT_UPD_W / VV_STAT_UPD_B, queued after the
 * following vv_apply_update, are the statistics of shadow - current, elementwise in fp32 -- one definition for all five solver rules.
 * It differs from the reference's update value by the rounding of ONE fp32 subtraction per element: the reference measures u where
 * W_new = fl(W - u), this measures fl(W - W_new).  A mark stays valid until vv_params_set.  VV_ERR_STATE: no parameters; between a hinted
 * backward pass and its vv_apply_update; while the sharded schedule (2) is selected. */
int vv_debug_mark_update(vv_ctx* ctx);
/* What the lines of net.cpp:580-636 print (over blob.cpp:138-165): the record of every entry as its LAST queued launch left it.
 * Synchronises the step's stream.  Entries never queued read all-zero. */
int vv_debug_stats_get(vv_ctx* ctx, vv_abs_stat out[VV_STAT_N]);

/* ---- an exponential moving average of the parameters, for evaluation (Polyak averaging).  Neither the reference tree nor BVLC Caffe has
 * a counterpart: the semantics are this project's own.  decay < 0 (the default, -1) turns it off and every call is what it was;
 * 0 <= decay < 1 turns it on; NaN or decay >= 1 is VV_ERR_ARG.  Sticky on the context until set again.  The activation makes the one
 * allocation -- eW [D][F] and eb [D] in fp32, with room for their 16-bit copy -- and starts the average from the current W and b with a
 * device copy; nothing is allocated on the step path afterwards.  vv_params_set while active starts it again from the new values; another
 * decay while active keeps the average; turning it off releases it.
 * While active, every completed vv_apply_update (an accumulated one and the finishing call of a step announced by vv_update_hint too: once
 * per update) is followed by ONE launch of k_ema on the step's stream, behind the update:
 *     e' = decay * e + om * w        om = 1.0f - decay, formed once on the host in fp32
 * for every element of W and of b -- two fp32 products and one fp32 sum, each rounded as written (no contraction into an fma).  No host
 * synchronisation, no atomics.  The update kernels are not touched: k_ema reads W and b after them, and parameters, histories, the 16-bit
 * copy, loss and gradients of a run with the average are bit for bit those of a run without it.
 * vv_ema_get: the average as host fp32 (either pointer may be NULL); synchronises.  VV_ERR_STATE while the average is off.
 * vv_ema_use(1): from here on the forward-only readers -- vv_forward, vv_embed, vv_embed_mean, vv_gallery_from_table -- read the averaged
 * parameters: their 16-bit copy and its scale are produced on demand on the context's stream, exactly as vv_params_set would produce them
 * for these fp32 values (max |e| -> the power-of-two scale -> round to nearest even), and are cached until the next k_ema.  So their
 * results are bit for bit those of a second context given vv_params_set(vv_ema_get()).  While in use every call that trains or replaces
 * the parameters is VV_ERR_STATE: vv_forward_backward*, vv_step, vv_apply_update, vv_params_set (and vv_ema_set(< 0)).  VV_ERR_STATE for
 * vv_ema_use(1) while the average is off, or between a backward pass announced by vv_update_hint and its vv_apply_update.
 * vv_ema_use(0) restores the training view; it moves nothing a training step owns (the guarantee vv_forward states), so the next
 * training step is bit for bit that of an undisturbed run.  The per-layer operators (vv_op_*) always read the training parameters.
 * Data parallel: on the sync schedule only -- every rank averages identical parameters.  VV_ERR_STATE: vv_ema_set(>= 0) while schedule 1
 * or 2 is selected, and vv_comm_schedule(1 or 2) / vv_comm_overlap(1) while the average is active. */
int vv_ema_set(vv_ctx* ctx, float decay);
int vv_ema_get_decay(vv_ctx* ctx, float* decay);
int vv_ema_get(vv_ctx* ctx, float* W, float* b);
/* The inverse of vv_ema_get, for a run that resumes: replaces the average by host fp32 values (either pointer may be NULL: that part
 * stays); synchronises.  VV_ERR_STATE while the average is off. */
int vv_ema_put(vv_ctx* ctx, const float* W, const float* b);
int vv_ema_use(vv_ctx* ctx, int on);
typedef struct { int64_t updates;                  /* k_ema launches since the activation (0 while off) */
                 float decay;                      /* as vv_ema_get_decay */
                 int32_t in_use; } vv_ema_report;  /* 1: vv_ema_use(1) is in effect */
int vv_ema_stats(vv_ctx* ctx, vv_ema_report* out);

/* ---- one training iteration */
typedef struct {
  /* shapes: VideoSampledShotsDataParameter batch_size / context_size / num_negative_samples
   * (caffe.proto:562-620); F and D come from the table and the parameters. */
  int32_t B, C, Nn;
  /* MAX_MARGIN_LOSS (src/caffe/layers/max_margin_loss_layer.cpp:39-40, caffe.proto:858-868) and
   * the loss weight of its first top (include/caffe/layer.hpp:416-422). */
  float margin;
  int32_t norm;
  float loss_weight;
  /* ELTWISE SUM coefficients of context_average (eltwise_layer.cpp:22-32); host [C-1], NULL =
   * 1/(C-1) each (the shipped prototxt's 0.25 x 4). */
  const float* ctx_coeff;
  /* DROPOUT on ip2 (dropout_layer.cpp:13-22): ratio 0 = layer absent.  mask: host uint8
   * [(C+Nn)*B][D] in the reference's row order (row = ch*B + b), 1 = keep; NULL = a counter-based
   * mask from dropout_seed and the iteration counter. */
  float dropout_ratio;
  const uint8_t* dropout_mask;
  uint64_t dropout_seed;
  /* Loss normaliser for data-parallel shards: the GLOBAL B*Nn; 0 = this batch's B*Nn
   * (max_margin_loss_layer.cpp:67 uses the local count; there is no multi-GPU in the reference). */
  int64_t global_count;
  /* SGDSolver::ComputeUpdateValue (src/caffe/solver.cpp:485-531): rate from the lr policy,
   * momentum, weight_decay, per-blob blobs_lr / weight_decay multipliers {W, b}, regulariser. */
  float lr, momentum, weight_decay;
  float lr_mult[2], decay_mult[2];
  int32_t reg;
  /* SolverParameter.solver_type (caffe.proto: SGD = 0, NESTEROV = 1, ADAGRAD = 2; GetSolver, solver.hpp:128-143):
   * NesterovSolver / AdaGradSolver::ComputeUpdateValue (solver.cpp:599-655, 714-781).  delta = AdaGrad's
   * stability constant (SolverParameter.delta, default 1e-8); AdaGrad requires momentum == 0 (solver.hpp:121).
   * RMSPROP = 3 and ADAM = 5 follow BVLC Caffe's RMSPropSolver / AdamSolver::ComputeUpdateValue (sgd_solvers: rmsprop_solver.cpp,
   * adam_solver.cpp; not in the reference tree): RMSProp needs momentum == 0, Adam reads momentum as beta1; delta is their stability
   * constant too, and what this struct has no field for arrives through vv_solver_ext_set. */
  int32_t solver_type;
  float delta;
  /* InnerProductParameter.regularization (inner_product_layer.cpp:80-90): the weight gradient is scaled by
   * 1 + regularization / 2 when regularization > 0.  0 = the shipped files' default. */
  float ip_regularization;
  /* MAX_MARGIN_LOSS's optional third bottom (max_margin_loss_layer.cpp:60-62, 82-97, 152-161, 173-186): a
   * non-negative weight per loss term, here one per batch item (the reference replicates a per-item blob over the
   * Nn terms with a SUM layer): L2 loss term w*max(0,m-d)^2, L1 term w*max(0,m-d).  Either the weights themselves
   * (use_direct_weight) or the values looked up from id_to_weight_file by the caller.  Host [B]; NULL = unweighted. */
  const float* item_weight;
} vv_step_cfg;

/* Defaults of the shipped project files (mednet_embedding_train.prototxt:195-198,655-671,
 * mednet_embedding_train_solver.prototxt:12-14): margin 2, L2, loss_weight 1, no dropout,
 * momentum .9, weight_decay 5e-4, lr_mult {1,2}, decay_mult {1,0}, L2 regulariser. */
void vv_step_cfg_default(vv_step_cfg* cfg);

/* Net::ForwardBackward (include/caffe/net.hpp:78-83) over the videovec TRAIN graph
 * (projects/videovec_embedding/mednet_embedding_train.prototxt:1-671):
 * gather -> fc7 -> ReLU(-> dropout) -> context mean -> L2 normalise -> dot-product scores ->
 * max-margin loss, and its backward down to the fc7 parameter gradients.
 * idx: int32 [B][C+Nn] table rows exactly as the data layer lays out its top blob
 * (video_sampled_shots_data_layer.cpp:214-220: channel 0 target, 1..C-1 context, C.. negatives),
 * -1 = all-zero row.  idx_on_device: 0 = host array; 1 = device pointer whose contents were produced on the context's
 * stream (vv_set_stream): every kernel of the step, the index grouping on the library's second stream included, is
 * ordered after the work already queued there; 2 = device pointer whose contents are complete when the call is made
 * (no ordering is added: static, pre-synchronised batches). */
int vv_forward_backward(vv_ctx* ctx, const vv_step_cfg* cfg, const int32_t* idx, int idx_on_device);
/* The same with the reference's quirk Q1 honoured: a same-video negative (max_same_video_negs > 0)
 * is copied WITHOUT its last feature (video_sampled_shots_data_layer.cpp:492), so that element of
 * the slot keeps what the previous batch left there.  last_src: int32 [B][C+Nn] = the table row
 * whose LAST feature each slot holds (-1 = zero), as vv_sampler_next reports it; both host arrays. */
int vv_forward_backward_q1(vv_ctx* ctx, const vv_step_cfg* cfg, const int32_t* idx,
                           const int32_t* last_src);
/* SGDSolver::ComputeUpdateValue + Net::Update (solver.cpp:485-531, net.cpp:803-839,
 * blob.cpp:112-136) on the gradients of the last vv_forward_backward.
 * (Without a communicator the last stage of the backward pass -- the sum of the weight gradient's split-K partials -- is
 * deferred: called right after vv_forward_backward, vv_apply_update reduces and updates in one launch; vv_loss_get,
 * vv_grads_get, vv_grads_device and vv_grads_bind run the reduction first if it is still due, and once vv_grads_device has
 * handed the buffer out every vv_forward_backward ends with it.  Results are bit for bit
 * those of the eager order; nothing observable through this interface changes.) */
int vv_apply_update(vv_ctx* ctx, const vv_step_cfg* cfg);
/* Both of the above: one iteration of Solver::Solve's loop body (solver.cpp:194,219-220). */
int vv_step(vv_ctx* ctx, const vv_step_cfg* cfg, const int32_t* idx, int idx_on_device);
/* Solver::Step as ONE unit (solver.cpp:177-221: ForwardBackward, ComputeUpdateValue, Update back to back): announces that the NEXT
 * vv_forward_backward* call will be followed by vv_apply_update with exactly these solver parameters (lr, momentum, weight_decay, lr_mult,
 * decay_mult, reg, solver_type, delta, and vv_solver_ext_set's and vv_clip_gradients_set's values) and that nothing reads the gradient in between.  The library may then apply the update where the
 * gradient is produced (option "wgrad_update", on by default): when the weight-gradient GEMM runs with one split of K (large D x F, small batches -- the shipped
 * mednet_embedding_train.prototxt: 4096 x 4096, batch 128) its epilogue applies the solver's rule to the tile it holds, and the 4 D F bytes
 * of dW are neither written nor read back; vv_apply_update then only finishes the step (bias, loss, scale bookkeeping).  Parameters, history
 * and losses are bit for bit those of the un-hinted calls.  Between such a vv_forward_backward* and its vv_apply_update only vv_loss_get
 * is allowed (vv_grads_*, vv_params_get, vv_op_inner_product_bwd, another forward pass: VV_ERR_STATE -- the gradient of such a step is not
 * kept, the parameters are half-way); after that vv_apply_update, until the next backward pass, vv_grads_* and a second vv_apply_update
 * are refused the same way (the gradient was never stored).  Where the fusion does not apply (several splits of K, a communicator, a bound gradient buffer, Adam's two histories, active gradient clipping) the hint changes nothing.
 * vv_step announces itself.  One hint covers one step. */
int vv_update_hint(vv_ctx* ctx, const vv_step_cfg* cfg);

/* Loss (already multiplied by loss_weight) and train_violations of the last forward; synchronises.
 * (the two tops of MAX_MARGIN_LOSS, max_margin_loss_layer.cpp:111-126.) */
int vv_loss_get(vv_ctx* ctx, float* loss, float* violations);

/* ---- the forward-only pass: Net::Forward / Net::ForwardPrefilled (include/caffe/net.hpp, src/caffe/net.cpp) under
 * Caffe::set_phase(Caffe::TEST), one of the test_iter passes of Solver::Test (solver.cpp:251-317) over a net built like the TRAIN graph:
 * gather -> fc7 -> ReLU (-> dropout) -> context mean -> L2 normalise -> scores -> max-margin loss and train_violations, and NO backward
 * pass: the held-out loss with the current weights.  idx and idx_on_device as vv_forward_backward.
 * Arithmetic: the training pass's own -- the same grouping, the same forward GEMM launch, the same score form, in forward-only
 * instantiations of the score kernels -- so for equal weights, idx and cfg the loss and violations are bit for bit those of
 * vv_forward_backward + vv_loss_get, in every score form, with "dedup" and "h16" on or off, with an explicit mask.  cfg->dropout_ratio is
 * honoured as given (a TEST-phase caller passes 0); a counter-based mask reads the iteration counter and does not advance it.  The loss is
 * divided by this batch's own B * Nn, as the training pass's is; cfg->global_count and the solver fields are checked and otherwise unused.
 * Local to the rank: no collective.  Sets "last_score_form", "last_fwd_tile_rows", "last_h16" and vv_dedup_stats, as a forward pass does.
 * Training state: the pass touches nothing a training step owns.  After fb(A); vv_forward(B); vv_apply_update the parameters, histories,
 * the 16-bit copy, vv_loss_get, vv_grads_get and every later step are bit for bit those of fb(A); vv_apply_update: the gradient stays where
 * it is (lazily reduced or not), the step's pending loss partials are not overwritten (the pass has partial buffers of its own; vv_loss_get
 * keeps returning the TRAINING pass's loss), the gradient-scale and f16-row report rings, Adam's t, the clipping and accumulation records
 * are not moved.  With an overlapped or sharded update in flight the pass first orders itself behind it.
 * Afterwards vv_blobs_get returns ip2 and the two score blobs of THIS pass; its ip1_diff, and vv_dedup_groups_get, are VV_ERR_STATE until
 * the next backward pass (after a training pass both are what they were).
 * VV_ERR_STATE: between a vv_forward_backward* announced by vv_update_hint and its vv_apply_update; with a batch shape (B, C, Nn) other
 * than the one the training step's buffers were sized for while that step's state is alive (the batch buffers are shared: evaluate with
 * the training shape; before the first training pass, or after vv_params_set, any shape is taken).
 * The result is read through the record below, not through vv_loss_get. */
int vv_forward(vv_ctx* ctx, const vv_step_cfg* cfg, const int32_t* idx, int idx_on_device);
/* Accumulation over passes (Solver::Test's test_score vector, solver.cpp:262-296, divided by test_iter at :304): a device record kept by
 * one thread of the pass's loss reduction -- no host synchronisation per pass.  last_*: the fp32 values vv_loss_get would show for the
 * last pass.  loss_sum / viol_sum: their sums in double, added in pass order (an fp32 value is exact in double); mean_* =
 * (float)(sum / passes); terms: B * Nn per pass.  vv_eval_reset zeroes the record (queued behind the passes already issued);
 * vv_params_set does not.  vv_eval_stats synchronises; before any pass it gives zeros. */
typedef struct { int64_t passes; int64_t terms; double loss_sum, viol_sum; float last_loss, last_violations;
                 float mean_loss, mean_violations; } vv_eval_report;
int vv_eval_reset(vv_ctx* ctx);
int vv_eval_stats(vv_ctx* ctx, vv_eval_report* out);

/* ---- gradients.  The flat fp32 device buffer [dW (D*F) | db (D)] that a data-parallel host
 * all-reduces (RCCL) between vv_forward_backward and vv_apply_update; there is no counterpart in
 * the reference (single GPU). */
int vv_grads_device(vv_ctx* ctx, void** dev_ptr, int64_t* n_floats);
/* Make the context write its gradients into caller-owned device memory of D*F + D floats (e.g. a
 * tensor of the collective library); NULL returns to the context's own buffer.  Takes effect for the
 * kernels launched afterwards and does not synchronise, so a host can alternate two buffers: one being
 * all-reduced while the next iteration's gradients are written to the other. */
int vv_grads_bind(vv_ctx* ctx, void* dev_ptr);
/* ---- data parallel: one process per GPU, the flat gradient buffer summed over the ranks between the backward pass
 * and the update.  No counterpart in the reference (single device: Caffe::SetDevice, common.cpp:127-145).
 *   vv_comm_init      after vv_params_set.  transport VV_COMM_RCCL: RCCL (loaded at this call; the copy a host framework
 *                     already loaded is reused); rank 0 writes the communicator id to the file id_path, the others wait
 *                     for it.  VV_COMM_SHM: a host-staged all-reduce through POSIX shared memory named after id_path, for
 *                     tests of the multi-rank path on a box with one device.  VV_COMM_PEER: the one-shot DIRECT exchange of one
 *                     node (<= 16 ranks): every rank's gradient and parameter buffers are mapped into every other rank (hipIpc, the
 *                     handles passed through a shared-memory object named after id_path), a reduce-scatter is one kernel that reads
 *                     this rank's shard of all N buffers over xGMI and adds them in rank order, an all-gather one kernel that pulls
 *                     the foreign shards; the ranks meet at flag words in host-coherent memory, the host is not in the loop.
 *                     Bit for bit the sums of VV_COMM_SHM; also works between processes that share one device.  Pair it with cfg.global_count = the
 *                     global B * Nn, and give every rank its items of the same global batch (vv_batch_ring_next).
 *   vv_allreduce_grads  sums [dW | db] over the ranks on the context's communication stream and makes the compute stream
 *                     wait for it (the host does not block with RCCL).  vv_apply_update calls it when the caller has not.
 *   vv_comm_overlap   on: exact synchronous SGD with the exchange hidden behind the NEXT step's forward pass.  The gradient
 *                     buffer is laid out chunk-major (a few column blocks of dW, each one contiguous message; vv_grads_get
 *                     still returns the blob's row-major D x F); vv_apply_update queues, per chunk, all-reduce -> SGD on the
 *                     chunk's columns -> publish on the communication stream and returns; the next vv_forward_backward starts
 *                     its forward GEMM at once, and the kernel waits for each chunk of W where its K loop reaches it
 *                     (InnerProductLayer::Forward reads every column of W: inner_product_layer.cpp:60-69).  Same sums,
 *                     same update as without overlap; every other entry point that touches the parameters first orders
 *                     itself behind the update in flight.  vv_allreduce_grads is a no-op in this mode. */
enum { VV_COMM_RCCL = 0, VV_COMM_SHM = 1, VV_COMM_PEER = 2 };
int vv_comm_init(vv_ctx* ctx, int32_t world, int32_t rank, const char* id_path, int32_t transport);
int vv_comm_overlap(vv_ctx* ctx, int on);
/* The three exchange schedules by number: 0 = sync, 1 = overlap (as vv_comm_overlap), 2 = SHARDED -- reduce-scatter of the gradients
 * (fp32), the solver's rule (SGDSolver::ComputeUpdateValue, solver.cpp:485-531, + Net::Update, net.cpp:803-839) on this rank's
 * D / world rows of W, the history and the bias, all-gather of the 16-bit copy of W + the bias that the next forward pass reads: 3/4 of
 * the all-reduce's bytes on the wire and 1/world of the update's memory traffic; the same parameters as the other schedules, bit for
 * bit in what the forward pass reads.  The fp32 master W and the history are then complete on their owner only: vv_params_get (and
 * vv_comm_destroy, and leaving the schedule) gather them and are COLLECTIVE calls -- every rank makes them, as every rank of
 * `caffe train` does at a snapshot.  Needs D divisible by world (else the step falls back to sync). */
int vv_comm_schedule(vv_ctx* ctx, int schedule);
int vv_allreduce_grads(vv_ctx* ctx);
int vv_comm_destroy(vv_ctx* ctx);
/* InnerProductLayer blobs_[0]/[1] cpu_diff() after Backward (inner_product_layer.cpp:76-98). */
int vv_grads_get(vv_ctx* ctx, float* dW, float* db);

/* ---- inspection of named blobs of the last forward (Net::blob_by_name, net.cpp:846-857);
 * every output optional (NULL).  Host fp32, in the reference's layouts:
 *   ip2          [(C+Nn)*B][D]  row = ch*B + b   (after ReLU / dropout)
 *   target_score [B][Nn], negative_scores [B][Nn]
 *   ip2_diff     [(C+Nn)*B][D]  the diff of ip1_nonorm */
int vv_blobs_get(vv_ctx* ctx, float* ip2, float* target_score, float* negative_scores,
                 float* ip1_diff);

/* ---- inspection of the row grouping of the last de-duplicated forward/backward pass (vv_set_dedup; no counterpart in the
 * reference, which copies and multiplies every repeat: video_sampled_shots_data_layer.cpp:836-875).  Read-only, for tests:
 * nothing a step executes depends on it.  Every output optional (NULL); synchronises.  With R = B*(C+Nn) instances
 * r = b*(C+Nn) + ch, Rp = R rounded up to 256, U distinct rows (vv_dedup_stats) and n_rows the table's all-zero row:
 *   rows      int32 [Rp]     table row of every instance (idx outside [0, n_rows) and r >= R: n_rows)
 *   uniq_rows int32 [Rp]     table row of every slot, slots in order of first appearance; n_rows from U on
 *   map       int32 [R]      slot of every instance
 *   ord       int32 [R]      arrival number of the instance inside its slot (a permutation of 0 .. cnt-1 per slot, order unspecified)
 *   cnt       int32 [Rp]     instances per slot; 0 from U on
 *   seg_start int32 [U + 1]  exclusive prefix sum of cnt; seg_start[U] = R
 *   pos       int32 [R]      seg_start[map[r]] + ord[r]: the instance's row in the grouped gradient buffer
 *   dyu       fp32 [Rp][D]   the per-slot 16-bit gradient sums the weight-gradient GEMM read, divided by *scale
 *   scale     the power of two those 16-bit values carry (1 for bf16): what vv_blobs_get divides ip1_diff by
 * Every vv_forward_backward* entry point runs the backward pass too, so dyu and scale always belong to the same step as the grouping
 * arrays; the debug launches of vv_blobs_get(ip1_diff) leave them untouched.  VV_ERR_STATE before the first forward/backward pass and
 * after a dense one. */
int vv_dedup_groups_get(vv_ctx* ctx, int32_t* rows, int32_t* uniq_rows, int32_t* map, int32_t* ord, int32_t* cnt,
                        int32_t* seg_start, int32_t* pos, float* dyu, float* scale);

/* ---- inference: fc7 (+ReLU) (+L2 normalise) of arbitrary table rows -- the extract_features path
 * (tools/extract_features.cpp:99-198 over videovec_extraction.prototxt:179-205) and the TEST
 * branch's embedding (mednet_embedding_train.prototxt:344-352).  rows host int32 [n] (NULL = 0..n-1),
 * out host fp32 [n][D]. */
int vv_embed(vv_ctx* ctx, const int32_t* rows, int64_t n, int relu, int l2norm, float* out);

/* The TEST branch's input: each sample is the coefficient-weighted sum of k table rows
 * (SLICE/CONCAT/SLICE + ELTWISE SUM `average_for_test`, mednet_embedding_train.prototxt:75-177), then
 * fc7 -> ReLU -> optional NORMALIZATION (`test_norm`, :344-352).  rows: host int32 [n][k];
 * coeff: host [k] or NULL for 1/k; out: host fp32 [n][D]. */
int vv_embed_mean(vv_ctx* ctx, const int32_t* rows, int64_t n, int32_t k, const float* coeff, int relu,
                  int l2norm, float* out);

/* RetrievalStatsLayer::Forward_cpu, per-shot retrieval (src/caffe/layers/retrieval_stats_layer.cpp:
 * 104-141, 143-355): distance = -2 X X^T (computed on the GPU), self excluded, ascending sort,
 * mean AP / hit@1 / hit@5 over samples whose class is >= 0.  feat: host fp32 [n][dim]; video_ids [n];
 * the id_to_class_file as two parallel arrays (ids absent from it read as class 0, as the
 * reference's map operator[] does).  Equal distances are ordered by ascending index (std::sort
 * leaves them unspecified; this order reproduces test_retrieval_stats_layer.cpp:82-84).
 * video_level_retrieval and stats_output_file are not built HERE: vv_gallery_pool_by_id and vv_gallery_class_stats below carry
 * them, for any n and without the n x n download. */
int vv_retrieval_stats(vv_ctx* ctx, const float* feat, int32_t n, int32_t dim, const int32_t* video_ids,
                       const int32_t* map_ids, const int32_t* map_cls, int32_t n_map,
                       int exclude_same_video_shots, float* mean_ap, float* hit_at_1, float* hit_at_5);

/* ---- gallery retrieval: RetrievalRankStatsFixedRefLayer (src/caffe/layers/retrieval_rank_stats_fixed_ref_layer.cpp, declared
 * include/caffe/loss_layers.hpp:64-125).  Queries are ranked against a fixed reference set ("gallery") that stays on the device.
 * Distance: d[i][g] = -2 dot(q_i, r_g) in fp32 with fp32 operands (:142-144).  Order: ascending (d, g) -- equal distances by
 * ascending gallery index (the reference's std::sort, :158-162, leaves ties unspecified; the same rule as vv_retrieval_stats).
 * The n_q x n_ref distance matrix (distance_matrix_, :30) never exists on the host and never whole on the device: queries are
 * processed in blocks whose device scratch is at most 1 GiB ("scratch_bytes" of vv_gallery_get), and no row is ever sorted.
 *
 * vv_gallery_create: bottom[2] / bottom[3] of the layer (:131-132).  feat: host fp32 [n_ref][dim]; ref_ids: host [n_ref], or NULL
 * for a gallery used only for vv_gallery_topk.  The id -> item lists the rank statistics need are built here, once.
 * vv_gallery_from_table: the same gallery from table rows, embedded with the arguments of vv_embed_mean (k = 1 and coeff = NULL:
 * vv_embed); the fp32 embeddings stay on the device.  rows: host int32 [n][k]. */
typedef struct vv_gallery vv_gallery;
int vv_gallery_create(vv_ctx* ctx, const float* feat, int64_t n_ref, int32_t dim, const int32_t* ref_ids, vv_gallery** out);
int vv_gallery_from_table(vv_ctx* ctx, const int32_t* rows, int64_t n, int32_t k, const float* coeff, int relu, int l2norm,
                          const int32_t* ref_ids, vv_gallery** out);
int vv_gallery_destroy(vv_ctx* ctx, vv_gallery* gallery);
/* The k nearest reference items of every query (the head of sort_ids, :158-162, without the sort).  q: host fp32 [n_q][dim];
 * 1 <= k <= 32 and k <= n_ref; idx / dist: host [n_q][k], ascending (d, g). */
int vv_gallery_topk(vv_ctx* ctx, vv_gallery* gallery, const float* q, int32_t n_q, int32_t k, int32_t* idx, float* dist);
/* Forward_cpu (:116-233) with ComputeApStats (:62-118): q = bottom[0], q_ids = bottom[1].  A query's positives are the reference
 * items carrying its id; their full-order ranks are COUNTED (1 + the number of items before the positive), not read off a sorted row.
 * As in the reference: best_rank starts at 10000 and stays there when no positive ranks earlier (:70, :77-79); recall@1 is a count,
 * recall@5 / @10 are divided by min(positives, 5) / min(positives, 10) (:81-108); a query without positives contributes AP 0 and
 * counts in every mean (:95, :226-230); the median is over all queries, the mean of the two middle ranks when n_q is even (:218-224).
 * Optional per-query outputs (NULL to skip): best_rank [n_q], ap [n_q], top5_idx / top5_dist [n_q][5] (both or neither; the five
 * nearest items and their distances, what stats_output_file lists, :180-196; index -1 where the gallery has fewer than five). */
typedef struct { float median_rank, recall_1, recall_5, recall_10, mean_ap; } vv_rank_stats;
int vv_gallery_rank_stats(vv_ctx* ctx, vv_gallery* gallery, const float* q, int32_t n_q, const int32_t* q_ids,
                          vv_rank_stats* out, int32_t* best_rank, float* ap, int32_t* top5_idx, float* top5_dist);
/* Properties of a gallery by name, in the manner of vv_get_option (the reference keeps the counterparts as layer members,
 * loss_layers.hpp:117-124): "n_ref", "dim", "scratch_bytes" (device scratch currently held for query blocks),
 * "scratch_limit_bytes", "query_block" (queries per block), "positive_chunk" (positives of one query ranked per pass; a query
 * with more takes several passes), "last_passes", "last_sim_ms" (device time of the similarity kernels of the last call),
 * "last_device_ms" (device time of the whole last call, uploads of the query blocks included), "n_ids" (distinct ids; 0 without
 * ids), "feat_device" / "row_floats" (the device address of the gallery's fp32 rows, for vv_dev_download, and the floats between
 * two rows: dim rounded up to a multiple of 32, the rest zero), "last_nearest_form" (what the last vv_gallery_nearest* call ran: 1 the
 * streaming form, 2 the selection form; 0 before the first).  Unknown name: VV_ERR_ARG. */
int vv_gallery_get(const vv_gallery* gallery, const char* name, double* value);

/* ---- nearest-neighbour lists of up to 2048 items.  The reference's nearest counterparts are the head of sort_ids
 * (retrieval_rank_stats_fixed_ref_layer.cpp:158-162) and top_5_ids (retrieval_stats_layer.cpp:310-316); k > 5 and the self form
 * HAVE NO REFERENCE COUNTERPART.  Distance, key and order are vv_gallery_topk's: -2 dot in fp32, ascending (d, g); the
 * distances returned are the floats the similarity kernel stored for the query block, nothing is evaluated twice.
 * Two forms, chosen per call: k < "nearest_select_min_k" (vv_set_option; default 33) runs vv_gallery_topk's streaming form with the
 * eligibility below as one more predicate; any other k selects the k smallest keys of every row without sorting it (digit
 * histograms of the distance word, a threshold, a collection pass, one sort of the k candidates).  Among equal distances at the
 * threshold the items of lowest gallery index are taken, whatever order the device ran in.  "last_nearest_form" of vv_gallery_get
 * tells which form ran; "last_sim_ms" / "last_device_ms" describe these calls too.  Device scratch stays within
 * "scratch_limit_bytes" (a block takes fewer rows where the selection form's per-row buffers need the room), nothing of size
 * n_q x n_ref exists on the host, and two calls return bit-identical results.
 *
 * vv_gallery_nearest: 1 <= k <= 2048 (= "positive_chunk").  q: host fp32 [n_q][dim].  q_ids: NULL, or host [n_q]: then only gallery
 * items whose id differs from q_ids[i] are eligible for query i (needs a gallery created with ids).  idx / dist: host [n_q][k],
 * ascending (d, g); where a query has fewer than k eligible items the remaining slots read idx -1, dist 0. */
int vv_gallery_nearest(vv_ctx* ctx, vv_gallery* gallery, const float* q, int32_t n_q, const int32_t* q_ids, int32_t k,
                       int32_t* idx, float* dist);
/* Every item of the gallery as a query against the gallery; the query rows are read from the gallery's device features
 * (as vv_gallery_class_stats does).  Eligible for item i: every j != i; with exclude_same_id every j of another id (needs a
 * gallery created with ids).  idx / dist: host [n_ref][k]. */
int vv_gallery_nearest_self(vv_ctx* ctx, vv_gallery* gallery, int32_t k, int exclude_same_id, int32_t* idx, float* dist);

/* ---- k-nearest-neighbour classifier: the class votes of the lists above, counted on the device.  HAS NO REFERENCE COUNTERPART (the
 * reference's nearest lists stop at five items and are only printed).  The lists are not downloaded and the scores stay in device
 * memory, ready for vv_classification_stats(scores_on_device = 1).
 * labels: host int32 [n_ref], the class of every gallery item, each in [0, num_classes); 1 <= num_classes <= 4096; 1 <= k <= 2048.
 * The neighbour list of a query is exactly the one vv_gallery_nearest / vv_gallery_nearest_self returns for the same arguments: the
 * same stored floats, the same eligibility (q_ids; self form j != i; exclude_same_id), ascending (d, g), the lowest gallery index at
 * a tie on the threshold, the same two forms chosen by "nearest_select_min_k".  m <= k: its filled slots.
 * Weight of list position j, with s_j = -0.5f d_j (exact):
 *   VV_KNN_UNIFORM  w_j = 1
 *   VV_KNN_EXP      w_j = expf((s_j - s_0) / T), s_0 the similarity at position 0, T = temperature > 0 in fp32; the difference and the
 *                   quotient are each rounded once in fp32, expf is the device library's default one.  So w_0 = 1 and every w_j is in
 *                   [0, 1], whatever the scale of the embeddings.
 * score[i][c] = V_c / V: V_c the sum of w_j over the positions with labels[idx_j] == c, V the sum over all m positions -- a posterior
 * estimate that sums to 1 up to rounding in every row with m >= 1, comparable across rows (per-class AP needs that).
 *   UNIFORM: V_c and V are integers <= 2048, counted in integer bins; score = (float)V_c / (float)m: one rounding, fully determined.
 *   EXP: fp32 sums in a fixed order, no floating-point atomics.  V_c adds the class's weights in ascending list position, starting
 *     from the first.  V adds the V_c: thread t of 256 adds those of classes t P .. t P + P - 1 (P = ceil(num_classes / 256)) in
 *     ascending class starting from +0, and the 256 partials fold by the tree x[t] += x[t + o], o = 128, 64 .. 1.  A class without a
 *     vote adds +0, so a row whose neighbours share one class scores exactly 1.0 there and +0 elsewhere.  Two calls give identical
 *     bits, and so do the two list forms.
 *   m == 0 (no eligible item): the row is all +0.0f.  Every element of out_dev is written.
 * out_dev: DEVICE fp32 [n_q][num_classes] of this context owned by the caller (vv_dev_alloc), as for vv_gallery_scores; rows are
 * stored 16 bytes at a time where out_dev is on 16 bytes and num_classes % 4 == 0, element by element otherwise, with identical
 * results (read-only option "last_knn_form": 1 / 2 at the last launch, 0 before the first).  n_used: NULL, or host [n_q]: every
 * row's m.  temperature is read under VV_KNN_EXP only.  vv_gallery_knn_scores_self: every gallery item as a query (n_q = n_ref):
 * leave-one-item-out, with exclude_same_id leave-one-id-out.
 * VV_ERR_ARG, with nothing launched or written: a NULL argument (q_ids and n_used may be NULL); a gallery of another context; n_q < 1;
 * k or num_classes out of range; a label outside [0, num_classes); an unknown weighting; under VV_KNN_EXP a temperature that is not
 * finite or <= 0; q_ids / exclude_same_id on a gallery created without ids.
 * "last_knn_vote_ms" of vv_gallery_get: the device time of the vote launches of the last of these calls; "last_nearest_form",
 * "last_sim_ms" and "last_device_ms" describe these calls too.  The calls synchronise. */
#define VV_KNN_UNIFORM 0
#define VV_KNN_EXP 1
int vv_gallery_knn_scores(vv_ctx* ctx, vv_gallery* gallery, const int32_t* labels, int32_t num_classes, const float* q, int32_t n_q,
                          const int32_t* q_ids, int32_t k, int32_t weighting, float temperature, float* out_dev, int32_t* n_used);
int vv_gallery_knn_scores_self(vv_ctx* ctx, vv_gallery* gallery, const int32_t* labels, int32_t num_classes, int32_t k,
                               int exclude_same_id, int32_t weighting, float temperature, float* out_dev, int32_t* n_used);

/* ---- k-means clustering of a gallery's items (Lloyd's iteration), every iteration on the device.  HAS NO REFERENCE COUNTERPART (the
 * reference has no clustering); the arithmetic below is this project's own and is stated exactly, so two calls, any block size and a
 * restatement in another language agree bit for bit (tests/kmeans_ref.py).  Every fp32 operation is rounded as written, none contracted.
 * Key.  d(i, c): the float the similarity kernel stores for item i against centroid row c -- vv_gallery_topk's distance, and
 *   vv_gallery_scores x -2, on a gallery made of the current centroids; nothing is evaluated a second way.
 *   VV_KMEANS_SPHERICAL  key = d.
 *   VV_KMEANS_EUCLIDEAN  key = d + nn_c, one fp32 add; nn_c = the sum of c[col]^2 as a serial chain in ascending column from +0, each
 *                        product and each sum rounded on its own.
 * Assignment: the cluster of the smallest (key, c); at a tie the lowest cluster index, as vv_gallery_topk orders (d, g).  A key that is
 *   NaN is never the smallest; a row of nothing but NaN goes to cluster 0.
 * Iteration t = 0 .. iters - 1: assign against the current centroids, then update.  After the last update one more assignment pass
 *   runs, so assign_out, counts_out and the report describe centroids_out; iters = 0 is "assign to a given codebook".
 * Traces, iters + 1 entries each, one per pass.  moved[t]: the items whose cluster differs from the previous pass (before the first
 *   pass every item is unassigned, so moved[0] = n).  objective[t]: the sum of the selected keys in double -- items 64 j .. 64 j + 63
 *   form slot j (an absent item adds +0.0), folded by x[i] += x[i + o], o = 32, 16 .. 1, and the slots are added in ascending j
 *   starting from +0.0.  No floating-point atomics.
 * Update of cluster c: its items in ascending item index, cut into chunks of 256 consecutive list entries; a chunk's partial is a
 *   serial fp32 chain (the first row is stored, then acc = acc + x); the partials are added in ascending chunk order starting from
 *   the first, giving s.  EUCLIDEAN: centroid = s * inv, inv = 1.0f / (float)count.  SPHERICAL: q = the serial chain of s[col]^2 from
 *   +0, centroid = s / sqrtf(q), both correctly rounded; q zero or not finite: the previous centroid is kept (degenerate).  A cluster
 *   without an item keeps its previous centroid bit for bit (empty).
 * Once moved[t] == 0 every later pass reproduces the same bits.  Inputs are assumed finite, as for the other gallery calls.
 *
 * vv_kmeans_cfg_default: 0 clusters (must be set), 20 iterations, EUCLIDEAN.  Limits: 1 <= num_clusters <= 4096, num_clusters <= n_ref,
 * iters >= 0.  Exactly one of init_centroids (host [C][dim]) and init_rows (host [C] item indices: the initial centroids are gathered
 * from the gallery's DEVICE rows, so a gallery made by vv_gallery_from_table serves) is given.
 * centroids_out: host [C][dim].  assign_out: host [n_ref] or NULL.  counts_out: host [C] or NULL.  objective_trace / moved_trace: host
 * [iters + 1] or NULL.  out: n, num_clusters, iters; empty_last / degenerate_last: the clusters the LAST update kept as empty /
 * degenerate (0 with iters = 0); moved_last / objective_last / nonfinite_rows (items whose selected key is not finite): the final pass.
 * VV_ERR_ARG, found on the host with nothing launched or written: a NULL required pointer; both or neither init given; a gallery of
 * another context; a value out of range or an unknown metric; an init_rows entry outside [0, n_ref) (vv_last_error names its position);
 * a shape whose buffers, the traces' record of iters + 1 passes included, pass the gallery path's scratch limit.
 * The call touches nothing a training step owns: it may be made between vv_forward_backward* and vv_apply_update.  All iterations are
 * queued on the context's stream without a host wait or an allocation between them; the call synchronises once, at its end.
 * Options: "km_block_rows" (rows of one score block, rounded up to 64; 0 = the plan's choice, csrc/vv_kmeans_plan.h); read-only
 * "last_km_blocks", "last_km_chunks", "last_km_assign_form" (1: 16-byte accesses, 2: element-wise -- identical results) and
 * "last_km_sim_ms" / "last_km_assign_ms" / "last_km_group_ms" / "last_km_update_ms", the device time of the last iteration's legs
 * (a pass of more than 1024 blocks: the first 1024 blocks' similarity and assign legs, scaled to all of them).
 * vv_kmeans_init_rows: a host function without a context -- the first num_clusters entries of the one epoch
 * vv_rows_shuffled(seed, n, 1, .) draws, so they are distinct. */
enum { VV_KMEANS_EUCLIDEAN = 0, VV_KMEANS_SPHERICAL = 1 };
typedef struct { int32_t num_clusters, iters, metric, reserved_; } vv_kmeans_cfg;
typedef struct { int64_t n; int32_t num_clusters, iters, empty_last, degenerate_last; int64_t moved_last;
                 double objective_last; int64_t nonfinite_rows; } vv_kmeans_report;
void vv_kmeans_cfg_default(vv_kmeans_cfg* cfg);
int vv_gallery_kmeans(vv_ctx* ctx, vv_gallery* items, const vv_kmeans_cfg* cfg, const float* init_centroids, const int32_t* init_rows,
                      float* centroids_out, int32_t* assign_out, int32_t* counts_out, double* objective_trace, int64_t* moved_trace,
                      vv_kmeans_report* out);
int vv_kmeans_init_rows(uint64_t seed, int32_t n, int32_t num_clusters, int32_t* rows_out);

/* ---- inverted-file (IVF) index on a gallery: a search that meets only the items of the nprobe nearest clusters.
 * HAS NO REFERENCE COUNTERPART (the reference searches exhaustively); the arithmetic below is this project's own and is stated exactly.
 * Distance.  d(i, g): the float the similarity kernel stores for query i against item g -- vv_gallery_topk's distance.  The grouped
 *   kernel runs the exhaustive kernel's tile body, whose summation order over the columns is the same for every output, so the float
 *   does not depend on where an item's row lies: the search is EXACT on its candidate set, and with nprobe == num_clusters idx and
 *   dist equal vv_gallery_topk's bit for bit.
 * Index (vv_ivf_create).  centroids: host [C][dim].  assign: host [n_ref], every entry in [0, C), taken as it is -- any item may be put
 *   in any list; NULL: the assignment vv_gallery_kmeans with iters = 0 returns for these centroids and this metric (that call is made).
 *   Cluster c's list holds its items in ascending item index; an empty list is legal.  The index owns a cluster-contiguous copy of the
 *   items' rows, the lists, the centroids and (EUCLIDEAN) nn_c as k-means defines it: the items gallery may be destroyed afterwards.
 * Search, one block of queries at a time:
 *   probe    key(i, c) = d(i, c) against the centroids (SPHERICAL) or d(i, c) + nn_c, one fp32 add, not contracted (EUCLIDEAN): k-means'
 *            key.  The nprobe smallest (key, c), ascending, the lowest cluster at a tie; -0 and +0 are one key.  A NaN key is below
 *            nothing: if fewer than nprobe keys are numbers, the remaining slots take the lowest clusters not yet chosen, ascending.
 *            nprobe == num_clusters: every cluster, in ascending index.
 *   candidates of query i: the items of its probed lists, m_i of them (n_candidates[i], if asked).
 *   result   the k smallest (d, g) of the candidates, g the item's index in the items gallery: equal distances order by ascending item
 *            index across lists, as vv_gallery_topk orders them.  Slots past m_i read idx -1, dist 0, as in vv_gallery_nearest.
 * Limits: 1 <= C <= 4096, C <= n_ref; metric VV_KMEANS_EUCLIDEAN or VV_KMEANS_SPHERICAL; 1 <= nprobe <= min(C, 64), and nprobe == C is
 * always allowed; 1 <= k <= 32; n_q >= 1; q: host [n_q][dim] with the index's dim.
 * VV_ERR_ARG, found on the host with nothing allocated, launched or written, vv_last_error naming the argument: a NULL required pointer;
 * a gallery or index of another context; C, metric, nprobe, k or n_q out of range; an assign entry outside [0, C) (its position is
 * named); a shape of which one query's candidates do not fit the gallery path's scratch limit.
 * Everything of a search is queued on the context's stream; the call synchronises once, at its end.  It touches nothing a training step
 * owns: it may be made between vv_forward_backward* and vv_apply_update.  No floating-point atomics.
 * Options: "ivf_block_rows" (query rows of one block) and "ivf_grid_wgs" (workgroups of the grouped similarity's fixed grid, 65535 at
 * most); 0 = the plan's choice (csrc/vv_ivf_plan.h).  Neither changes a bit of the result.
 * vv_ivf_get: "n_ref", "dim", "num_clusters", "metric", "largest_list", "empty_lists"; of the last search "last_blocks", "last_tiles"
 * (128 x 128 similarity tiles), "last_candidates" (the sum of m_i), "last_grid_wgs", and the device time "last_probe_ms",
 * "last_group_ms", "last_sim_ms", "last_select_ms" (a search of more than 64 blocks: the first 64 blocks' legs, scaled to all of them)
 * and "last_device_ms" (the whole call).  An unknown name is VV_ERR_ARG.
 * vv_ivf_lists: host copies for tools and tests -- start [C + 1], list [n_ref]: cluster c's items are list[start[c] .. start[c + 1]). */
typedef struct vv_ivf vv_ivf;
int vv_ivf_create(vv_ctx* ctx, vv_gallery* items, const float* centroids, int32_t num_clusters, int32_t metric, const int32_t* assign_or_null,
                  vv_ivf** out);
int vv_ivf_destroy(vv_ctx* ctx, vv_ivf* index);
int vv_ivf_search(vv_ctx* ctx, vv_ivf* index, const float* q, int32_t n_q, int32_t nprobe, int32_t k, int32_t* idx, float* dist,
                  int32_t* n_candidates_or_null);
int vv_ivf_get(const vv_ivf* index, const char* name, double* value);
int vv_ivf_lists(vv_ctx* ctx, vv_ivf* index, int32_t* start, int32_t* list);

/* ---- product-quantised lists (IVF-PQ): the inverted-file index with every item kept as M one-byte codes in place of its fp32 row.
 * HAS NO REFERENCE COUNTERPART (the reference quantises nothing); the arithmetic below is this project's own and is stated exactly.
 * Every fp32 operation is rounded as written and none is contracted.
 * Sub-space m = 0 .. M - 1 is the columns m dsub .. (m + 1) dsub - 1, dsub = dim / M.
 * Training (vv_pq_train).  codebooks_out[m], host [ksub][dsub], is exactly the centroids_out of vv_gallery_kmeans (EUCLIDEAN, ksub
 *   clusters, iters, init_rows = vv_kmeans_init_rows(seed + m, n_ref, ksub)) on a gallery made of those columns of the items; that call's
 *   body runs on a column slice cut on the device, nothing of it is restated.  objective_out[m] (or NULL) is its objective_last.
 * Encoding (vv_pq_encode, and vv_ivfpq_create for itself).  code[g][m] is the assignment that call returns with iters = 0 and
 *   init_centroids = codebooks[m]: k-means' key d + nn_c, the lowest codeword at a tie, a row of nothing but NaN to codeword 0.  Since
 *   that call is made, ksub <= n_ref holds for encoding as for training.  Codes are never taken from the host: every byte that indexes
 *   a table was written by the library's own encoder and is < ksub.
 * Table of query i (kernel k_pq_lut).  lut(i, m, j) = -2.0f * s + 0.0f; s is the serial chain over the sub-space's columns in ascending
 *   order starting from +0.0f, s = s + q[i][col] * codebooks[m][j][col], every product and every sum rounded on its own.  This is NOT
 *   the similarity kernel's float: dsub is small, and numpy restates the chain directly (tests/pq_ref.py).
 * Approximate distance a(i, g): the serial chain acc = lut(i, 0, code[g][0]), then acc = acc + lut(i, m, code[g][m]), m = 1 .. M - 1.
 * Probe, candidates of query i, n_candidates: vv_ivf_search's, word for word -- the centroid keys are still the similarity kernel's
 *   floats on full-dimension rows.
 * Result: the k smallest (a, g) of the candidates, g the item's index in the items gallery; equal a order by ascending g across lists;
 *   slots past m_i read idx -1, dist 0; dist returns a.
 * Not residual: a code encodes the raw row, not the row minus its list's centroid, so one table serves all of a query's lists.  The
 *   index keeps no fp32 item rows and does not re-rank its result against them.
 * Index (vv_ivfpq_create): centroids, num_clusters, metric and assign_or_null as vv_ivf_create takes them; codebooks: host
 *   [M][ksub][dsub].  The index owns the code rows in list-position order, the codebooks, the lists, the centroids and nn_c: the items
 *   gallery may be destroyed afterwards.
 * Limits: 1 <= M <= 64 and dim % M == 0; 2 <= ksub <= 256 and ksub <= n_ref; M * ksub * 4 <= 65536 (one query's whole table sits in LDS);
 *   iters >= 0; C, metric, nprobe, k <= 32 and n_q exactly vv_ivf_search's, nprobe == C always allowed; q: host [n_q][dim].
 * VV_ERR_ARG, found on the host with nothing allocated, launched or written, vv_last_error naming the argument: a NULL required pointer;
 * a gallery or index of another context; a value outside the limits above; an assign entry outside [0, C) (its position is named); a
 * shape whose buffers do not fit the gallery path's scratch limit.
 * Everything of a search is queued on the context's stream, one scratch allocation carved up by csrc/vv_pq_plan.h; the call synchronises
 * once, at its end, and touches nothing a training step owns.  No floating-point atomics.  Option "ivf_block_rows" is honoured; it
 * changes no bit of the result.
 * vv_ivfpq_get: "n_ref", "dim", "num_clusters", "metric", "M", "ksub", "largest_list", "empty_lists", "index_bytes" (every device byte
 * the index owns, scratch excluded); of the last search "last_blocks", "last_candidates", "last_scan_form" (how k_pq_scan loaded a code
 * row -- 1: 16 bytes, M % 16 == 0; 2: 4 bytes, M % 4 == 0; 3: bytes; 0: no search yet; identical results) and the device time
 * "last_probe_ms", "last_lut_ms", "last_scan_ms", "last_select_ms" (more than 64 blocks: the first 64 blocks' legs, scaled) and
 * "last_device_ms" (the whole call).  An unknown name is VV_ERR_ARG.
 * vv_ivfpq_lists: as vv_ivf_lists.  vv_ivfpq_codes: host [n_ref][M], row p the codes of item list[p] -- list-position order.
 * vv_pq_encode: codes_out host [n_ref][M], item order. */
typedef struct vv_ivfpq vv_ivfpq;
int vv_pq_train(vv_ctx* ctx, vv_gallery* items, int32_t M, int32_t ksub, int32_t iters, uint64_t seed, float* codebooks_out,
                double* objective_out_or_null);
int vv_pq_encode(vv_ctx* ctx, vv_gallery* items, const float* codebooks, int32_t M, int32_t ksub, uint8_t* codes_out);
int vv_ivfpq_create(vv_ctx* ctx, vv_gallery* items, const float* centroids, int32_t num_clusters, int32_t metric, const int32_t* assign_or_null,
                    const float* codebooks, int32_t M, int32_t ksub, vv_ivfpq** out);
int vv_ivfpq_destroy(vv_ctx* ctx, vv_ivfpq* index);
int vv_ivfpq_search(vv_ctx* ctx, vv_ivfpq* index, const float* q, int32_t n_q, int32_t nprobe, int32_t k, int32_t* idx, float* dist,
                    int32_t* n_candidates_or_null);
int vv_ivfpq_get(const vv_ivfpq* index, const char* name, double* value);
int vv_ivfpq_lists(vv_ctx* ctx, vv_ivfpq* index, int32_t* start, int32_t* list);
int vv_ivfpq_codes(vv_ctx* ctx, vv_ivfpq* index, uint8_t* codes);

/* ---- class-level leave-one-out statistics on a gallery: RetrievalStatsLayer (src/caffe/layers/retrieval_stats_layer.cpp).
 * vv_gallery_pool_by_id: video_level_retrieval (:165-198).  A new gallery with one item per distinct id of `gallery`, its row the
 * sum over the id's items, in ascending item index, of (1 / count) x_i in fp32 (the reference's weight matrix, :193, :197-198),
 * its id that id.  Items are in ASCENDING ID (the reference's order is boost::unordered_map's, unspecified).  Needs a gallery
 * created with ids; computed on the device from the gallery's own rows.  "n_ids" of vv_gallery_get: the number of distinct ids.
 *
 * vv_gallery_class_stats: Forward_cpu (:213-304, :351-353) with ComputeStats (:104-141).  Every item i of the gallery is a query
 * against all the others; its class is the map's entry for its id, 0 for an id the map does not hold (operator[], :110, :117;
 * map_ids / map_cls: the id_to_class_file as two parallel host arrays, n_map >= 1, :48; an id listed twice reads as its later
 * entry).  Distance -2 dot(x_i, x_j) in fp32 (:208-209), order ascending (d, j).  A query of negative class is skipped (:250-252)
 * but stays an item others are ranked against.  Ranked set: every j != i (:113, :231-232), and with exclude_same_id every j of
 * another id (:114-115); a positive is a ranked item of the query's class; val / ret of a positive are COUNTED, no row is sorted:
 * ap = (sum ret / val) / positives, 0 without positives (:125, :131-133); acc1 = positives with val <= 1; acc5 = (positives with
 * val <= 5) / 5 (:135).  out: the means over the scored queries (:351-353) and their number; no scored query: VV_ERR_ARG.
 * Optional per-item outputs (NULL to skip): ap / acc1 / acc5 host [n_ref], NaN for a skipped query; top5_idx host [n_ref][5]: the
 * five nearest items of OTHER ids, whatever exclude_same_id says (what stats_output_file lists, :310-316), -1 where fewer exist
 * (the reference prints the previous query's entries there) and for a skipped query.  The query rows are read from the gallery's
 * device features; device scratch stays within "scratch_limit_bytes"; two calls return bit-identical results.
 * "last_passes", "last_sim_ms", "last_device_ms" of vv_gallery_get describe this call too. */
typedef struct { float mean_ap, hit_at_1, hit_at_5; int32_t n_scored; } vv_class_stats;
int vv_gallery_pool_by_id(vv_ctx* ctx, vv_gallery* gallery, vv_gallery** out);
int vv_gallery_class_stats(vv_ctx* ctx, vv_gallery* gallery, const int32_t* map_ids, const int32_t* map_cls, int32_t n_map,
                           int exclude_same_id, vv_class_stats* out, float* ap, float* acc1, float* acc5, int32_t* top5_idx);

/* ---- event classification: ClassificationStatsLayer (src/caffe/layers/classification_stats_layer.cpp:13-95).
 * vv_gallery_scores: out_dev [n_q][n_ref], DEVICE fp32 of this context owned by the caller (vv_dev_alloc), = the fp32 dot products
 * dot(q_i, r_g) of which vv_gallery_topk's distance is the -2 multiple: the float the similarity kernel stored, times -0.5f (both
 * factors powers of two: exact; nothing is evaluated a second way).  q: host fp32 [n_q][dim], processed in query blocks as the
 * other gallery calls do; synchronises.  HAS NO REFERENCE COUNTERPART.  With a gallery of class prototypes (vv_gallery_create with
 * ref_ids = the class of each item, then vv_gallery_pool_by_id: one prototype per class, ascending class) this is a
 * nearest-class-mean classifier's score matrix, ready for vv_classification_stats(scores_on_device = 1) without a host round trip.
 *
 * vv_classification_stats: Forward_cpu (:36-95).  scores: fp32 [n][num_classes] row-major (bottom[0], :38); labels: host int32 [n],
 * the true class of each row (bottom[1], :39, :52).
 *   predicted class of a row: the LOWEST column attaining the row's maximum (the walk starts at column 0 and replaces on strict >,
 *     :50-61; -0.0f and 0.0f compare equal)
 *   count[c]: rows of label c (:53); accuracy[c] = (float)correct_c / (float)count_c, correct_c the rows of label c predicted c
 *     (:63-66, :71), 0 where count[c] == 0 (:88); out->total_accuracy = (float)(sum of correct_c) / (float)n (:93).  The reference
 *     counts in floats; every count here is an integer below 2^24, so these outputs are exact and fully determined
 *   ap[c] (:72-85), the reference's quirk included: it sorts n dummy entries (0, false) together with the n real (score, label == c)
 *     pairs by std::greater<pair> and walks only the first n.  So a row whose score in column c is below 0 never contributes (at
 *     least n dummies precede it) but still counts in the divisor count[c]; among equal scores positives precede the others and the
 *     dummies; a positive with score exactly 0 or -0 is visited.  For a visited positive p with score s:
 *       G = rows (any label) with score > s,  P = positives of c with score > s,  E = positives of c with score == s and index < p
 *       (item order breaks ties among interchangeable entries),  term(p) = (P + E + 1) / (G + E + 1)
 *     ap[c] = (float)(sum of term(p) / count[c]), terms and sum in double, positives in a fixed order of ascending item index
 *     through a fixed reduction tree, no floating-point atomics: two calls give identical bits.  (The reference sums the same terms
 *     as a serial fp32 chain.)  0 where count[c] == 0 (:89).  G, P and E are COUNTED on the device; nothing of size n x n, or sorted,
 *     ever exists
 *   out->mean_ap: the mean of the double quotients over the classes with count > 0, rounded once (THIS PROJECT'S OWN: the layer
 *     has no such top); classes_present: their number; n: the rows
 * scores_on_device = 0: host scores, uploaded in column blocks so that the call's device scratch stays within the gallery path's
 * 1 GiB ("scratch_limit_bytes") for any n x num_classes; 1: device memory of this context (vv_dev_alloc), read on the context's
 * stream.  accuracy / ap / count: host [num_classes], each may be NULL.  The call synchronises.
 * VV_ERR_ARG: n < 1, num_classes < 1, n > 2^24 (above it the reference's float counters stop counting: 2^24 + 1 is not a float);
 * a label outside [0, num_classes) (an out-of-bounds index in the reference); any NaN score (the reference's sort is undefined on
 * them; the device counts them and vv_last_error gives the count).  +-Inf are ordinary values.
 * vv_set_option "cls_pass_tiles" (16384; 1 .. 65535): 256-positive tiles of one counting launch; "cls_block_cols" (0 = as many as
 * the scratch limit admits): columns of one block at most -- small values are how the tests reach several launches and blocks at
 * small shapes; results do not depend on either.  Read-only "last_cls_passes" (counting launches of the largest block),
 * "last_cls_segments" (workgroups along a column), "last_cls_blocks", "last_cls_row_ms" / "last_cls_count_ms" (device time of the
 * row pass + column pack / of the counting and final passes) describe the last call. */
typedef struct { float total_accuracy, mean_ap; int32_t classes_present, reserved_; int64_t n; } vv_classification_report;
int vv_classification_stats(vv_ctx* ctx, const float* scores, int64_t n, int32_t num_classes, const int32_t* labels,
                            int scores_on_device, float* accuracy, float* ap, int32_t* count, vv_classification_report* out);
int vv_gallery_scores(vv_ctx* ctx, vv_gallery* gallery, const float* q, int32_t n_q, float* out_dev);

/* ---- a softmax linear classifier trained on gallery embeddings: the reference's INNER_PRODUCT layer under SOFTMAX_LOSS
 * (src/caffe/layers/softmax_layer.cpp:25-59, softmax_loss_layer.cpp:34-83, inner_product_layer.cu:12-59) with SGDSolver's
 * momentum rule and L2 decay (src/caffe/solver.cpp:485-531).  Its logits are the score matrix vv_classification_stats reads.
 * vv_linear: W fp32 [num_classes][dim], b [num_classes] (bias != 0), their momentum histories, a step counter and the batch cursor,
 * all on the device; created all zero.  vv_linear_get / vv_linear_put: host copies, each pointer may be NULL (put: left as it is);
 * put sets the step counter and returns the cursor to 0.  With bias == 0, b / hb read as zeros and are ignored by put.
 * One step over `count` rows x_i of the training gallery with labels y_i (host int32 [n_ref], each in [0, num_classes)):
 *   z = X W^T + b (inner_product_layer.cu:12-27); the row maximum is the FIRST maximum (softmax_layer.cpp:38-44)
 *   p = exp(z - max) / sum exp(z - max)  (:46-57)
 *   loss = loss_weight (1 / count) sum_i -log(max(p_i[y_i], FLT_MIN))  (softmax_loss_layer.cpp:44-51), summed in double in a fixed order
 *   dz = (p - onehot) (loss_weight / count)  (:68-81; the quotient is formed once, in fp32);  dW = dz^T X, db = sum_i dz_i
 *     (inner_product_layer.cu:33-49)
 *   h = lr (g + weight_decay W) + momentum h;  W = W - h  (solver.cpp:497-523); no decay on b (the shipped nets' decay_mult 0)
 * vv_linear_fit: cfg->iters steps.  batch == 0: every step takes the whole gallery; else count = min(batch, n_ref - cursor) consecutive
 * items from the cursor (a database read in order; a batch never wraps), the cursor returns to 0 behind the last batch of an epoch and
 * is carried across calls.  lr_schedule[t] (host [iters]) replaces cfg->lr for step t when given.  All steps are queued on the context's
 * stream with no host synchronisation in between; the call synchronises once at its end and fills loss_trace (host [iters], may be
 * NULL) and *out: loss_first / loss_last, accuracy_last (the share of the last batch's rows whose first-maximum column is the label),
 * steps (the object's counter), nonfinite_rows (rows of any step with a logit that is not finite).
 * vv_linear_grad: the gradient of the batch [first, first + count) at the current W, b: dW host [num_classes][dim], db [num_classes], *loss
 * (each may be NULL); nothing is updated, the cursor does not move.
 * vv_linear_scores: out_dev [n_q][num_classes] fp32 DEVICE memory of the caller (vv_dev_alloc) = z, bias included, for the rows of host
 * q [n_q][dim] (src NULL), or for the device rows of gallery src (q NULL; n_q must be its item count).  Exactly one of the two.
 * vv_op_softmax_loss: the softmax kernel on the caller's logits z_dev [rows][pitch] (pitch >= cols floats between rows; labels host
 * [rows]): prob_dev / dz_dev [rows][pitch] device or NULL (dz's columns cols .. pitch - 1 are written zero), *loss and *correct (rows whose
 * first maximum is the label) may be NULL.  Synchronises.
 * vv_op_gemm_tn: out_dev [m][n] = A^T B for A_dev [k][m] (lda floats between rows) and B_dev [k][n] (ldb): the weight-gradient launch and
 * its slab reduction, exact fp32 (an ordered fmaf chain per split, the splits added in order).  Synchronises.
 * Every sum has a fixed order and no floating-point atomic exists: the same inputs give the same bits on every call.
 * VV_ERR_ARG: num_classes outside 1 .. 4096; dim < 1 or different from the gallery's; a label outside [0, num_classes); iters < 1;
 * batch < 0; first / count outside the gallery; rows, cols, k, m or n below 1 (cols above 4096, pitch < cols, lda < m, ldb < n).
 * None of these calls touches the training step's state: they may be made between vv_forward_backward* and vv_apply_update.
 * vv_set_option "lin_split_rows" (0 = the library's plan): rows of one split of the weight-gradient product; a row block of a batch holds
 * at most 128 splits, so small values are how the tests reach several splits and row blocks at small shapes.  Read-only
 * "last_lin_splits" (splits of the largest row block), "last_lin_blocks" (row blocks of one batch), "last_lin_fwd_ms" /
 * "last_lin_softmax_ms" / "last_lin_wgrad_ms" / "last_lin_update_ms" (device time of the four legs in the last step of the last fit). */
typedef struct vv_linear vv_linear;
int vv_linear_create(vv_ctx* ctx, int32_t dim, int32_t num_classes, int bias, vv_linear** out);
int vv_linear_destroy(vv_ctx* ctx, vv_linear* lin);
int vv_linear_get(vv_ctx* ctx, vv_linear* lin, float* W, float* b, float* hW, float* hb, int64_t* steps);
int vv_linear_put(vv_ctx* ctx, vv_linear* lin, const float* W, const float* b, const float* hW, const float* hb, int64_t steps);
typedef struct { int32_t iters, batch; float lr, momentum, weight_decay, loss_weight; } vv_linear_cfg;
typedef struct { float loss_first, loss_last, accuracy_last; int32_t reserved_; int64_t steps, nonfinite_rows; } vv_linear_report;
void vv_linear_cfg_default(vv_linear_cfg* cfg);     /* iters 100, batch 0, lr 0.1, momentum 0.9, weight_decay 0, loss_weight 1 */
int vv_linear_fit(vv_ctx* ctx, vv_linear* lin, vv_gallery* train, const int32_t* labels, const vv_linear_cfg* cfg,
                  const float* lr_schedule, float* loss_trace, vv_linear_report* out);
int vv_linear_grad(vv_ctx* ctx, vv_linear* lin, vv_gallery* train, const int32_t* labels, int64_t first, int64_t count,
                   float loss_weight, float* dW, float* db, float* loss);
int vv_linear_scores(vv_ctx* ctx, vv_linear* lin, vv_gallery* src_or_null, const float* q, int64_t n_q, float* out_dev);
int vv_op_softmax_loss(vv_ctx* ctx, const float* z_dev, int64_t rows, int32_t cols, int64_t pitch, const int32_t* labels,
                       float loss_weight, float* prob_dev, float* dz_dev, float* loss, int64_t* correct);
int vv_op_gemm_tn(vv_ctx* ctx, const float* A_dev, int64_t lda, const float* B_dev, int64_t ldb, int64_t k, int32_t m, int32_t n,
                  float* out_dev);

/* ---- the same classifier as a linear SVM per class: the reference's INNER_PRODUCT layer under HINGE_LOSS
 * (src/caffe/layers/hinge_loss_layer.cpp:13-77, HingeLossParameter's L1 and L2 norm).  Every column of the logits is a binary problem
 * with target +1 on the label's column and -1 elsewhere.  For a batch of `count` rows, every fp32 operation rounded as written:
 *   z = the logit the softmax loss reads;  t = (c == label) ? -z : z  (hinge_loss_layer.cpp:25)
 *   m = (0 < 1 + t) ? 1 + t : 0  (:29-30; a NaN logit gives m = 0, as std::max(Dtype(0), x) does; +Inf stays +Inf)
 *   L1: loss = loss_weight (sum m) / count (:36);  dz = +-[m > 0] (loss_weight / (float)count), - on the label's column
 *       (:61-69, caffe_cpu_sign and caffe_scal)
 *   L2: loss = loss_weight (sum m m) / count (:39);  dz = +-m ((loss_weight * 2.0f) / (float)count)  (:71, left to right)
 * The sum is taken in double over the exact fp32 terms (m, or m m formed in double) in a fixed order -- a lane's columns ascending,
 * the lanes of a row, the rows of a wave, the waves of a workgroup, the workgroups in index order -- and rounded once; there is no
 * floating-point atomic, so two calls give the same bits.  `correct` and the non-finite count mean what they mean under the softmax loss.
 * vv_linear_loss_set (hinge_loss_layer.cpp:34-43, the layer's norm switch): the loss vv_linear_fit and vv_linear_grad run from now on,
 * sticky on the object like vv_solver_ext_set on a context.  A new object is VV_LIN_LOSS_SOFTMAX.  Switching touches neither
 * parameters, histories, step counter nor cursor.  norm (VV_NORM_L1 / VV_NORM_L2) is read for VV_LIN_LOSS_HINGE only.  vv_linear_scores,
 * _get and _put do not depend on it.  VV_ERR_ARG: another loss value; with HINGE another norm; a classifier of another context.
 * vv_linear_loss_get (hinge_loss_layer.cpp:34, 65: what the switch reads): either pointer may be NULL; norm is the last one set with
 * HINGE (VV_NORM_L2 on a new object).
 * vv_op_hinge_loss (hinge_loss_layer.cpp:13-77): the hinge kernel on the caller's logits z_dev [rows][pitch], as vv_op_softmax_loss:
 * any pitch >= cols, any alignment; dz_dev [rows][pitch] device or NULL (columns cols .. pitch - 1 are written zero), *loss and *correct
 * may be NULL.  Synchronises.  VV_ERR_ARG: vv_op_softmax_loss's checks, and a norm that is neither VV_NORM_L1 nor VV_NORM_L2.
 * With base pointers on 16 bytes and pitch % 4 == 0 (always inside vv_linear_fit / _grad) the kernel reads and writes 16 bytes at a
 * time; otherwise element by element, with identical results.  Read-only "last_hinge_form": 1 / 2 for the two forms at the last launch,
 * 0 before the first; "last_hinge_nonfinite": rows with a logit that is not finite in the last vv_op_hinge_loss.  Under the hinge
 * loss "last_lin_softmax_ms" is the hinge kernel's device time. */
enum { VV_LIN_LOSS_SOFTMAX = 0, VV_LIN_LOSS_HINGE = 1 };
int vv_linear_loss_set(vv_ctx* ctx, vv_linear* lin, int32_t loss, int32_t norm);
int vv_linear_loss_get(vv_ctx* ctx, vv_linear* lin, int32_t* loss, int32_t* norm);
int vv_op_hinge_loss(vv_ctx* ctx, const float* z_dev, int64_t rows, int32_t cols, int64_t pitch, const int32_t* labels,
                     int32_t norm, float loss_weight, float* dz_dev, float* loss, int64_t* correct);

/* ---- the same classifier trained on a LIST of gallery rows: shuffled epochs, held-out folds, oversampling.  What this replaces in
 * the reference is the data order only: DataLayer reads its database through one cursor, in order, and returns to the first record
 * behind the last (src/caffe/layers/data_layer.cpp:53, 69-70, 180-198), which vv_linear_fit reproduces on a gallery; a shuffled
 * order exists there only as a database built with convert_imageset --shuffle (tools/convert_imageset.cpp:34-35, 68-72).  The row
 * lists, their generator, the folds and cross-validation below are this project's own; nothing else of the reference is involved.
 * rows: host int32 [n_rows], gallery items in any order, repeats allowed, n_rows 1 .. 2^30 (it may exceed n_ref).  labels stays host
 * [n_ref], BY GALLERY ITEM: the library forms labels[rows[i]] and uploads it beside the list.
 * vv_linear_fit_rows: vv_linear_fit with the list in place of the gallery's item range.  The list is consumed from position 0: step t
 * takes count = min(batch, n_rows - pos) consecutive entries, pos returns to 0 behind the last entry; batch == 0: the whole list every
 * step.  The object's gallery cursor is neither read nor moved; the step counter advances; the sticky loss applies; row blocks and the
 * scratch limit are vv_linear_fit's with list positions in place of gallery rows.  One synchronisation, at the end.
 * vv_linear_grad_rows: vv_linear_grad of the batch that is the whole list.  vv_linear_scores_rows: out_dev [n_rows][num_classes]
 * (DEVICE memory of the caller) = the logits of item rows[i] in row i.
 * Every result has the bits the contiguous call gives on a gallery built from the listed rows in list order with labels[rows[i]]: the
 * gathered forms of the two products differ from the contiguous ones in the address of a row and in nothing else.  Read-only option
 * "last_lin_gather": the form of the last batch's products -- 0 before the first batch, 1 contiguous, 2 gathered.
 * VV_ERR_ARG, all found on the host before anything is launched or changed (parameters, histories, step counter and cursor stay as
 * they were): rows NULL; n_rows outside 1 .. 2^30; an entry outside [0, n_ref) -- vv_last_error names its position: no such index ever
 * reaches a kernel; a label outside [0, num_classes) on a LISTED item; and every check vv_linear_fit / _grad / _scores makes.  The
 * label of an item that is NOT listed is never read, so a bad label there is accepted: a held-out item may carry a class the
 * training rows' classifier does not know, or no label at all.
 * vv_rows_shuffled / vv_rows_fold: the lists, host functions without a context (videovector_amd/csrc/vv_rows.h states the generator
 * in full: one splitmix64 stream, Fisher-Yates from i = n - 1 down to 1 on the identity, j = the high 64 bits of next() * (i + 1)).
 * vv_rows_shuffled: out [epochs][n], every epoch a fresh permutation of 0 .. n - 1 from the one stream seeded with seed.
 * vv_rows_fold: perm = one shuffled epoch of seed; held = perm[floor(fold n / folds) .. floor((fold + 1) n / folds)), train = the rest,
 * both in perm's order; exactly *n_held and *n_train = n - *n_held entries are written (buffers of n entries always suffice).  Folds
 * are not stratified: one may lack a class, which vv_classification_stats reports as classes_present.
 * VV_ERR_ARG: n < 1; epochs < 1; folds outside 2 .. n; fold outside [0, folds); a NULL pointer. */
int vv_linear_fit_rows(vv_ctx* ctx, vv_linear* lin, vv_gallery* train, const int32_t* labels, const int32_t* rows, int64_t n_rows,
                       const vv_linear_cfg* cfg, const float* lr_schedule, float* loss_trace, vv_linear_report* out);
int vv_linear_grad_rows(vv_ctx* ctx, vv_linear* lin, vv_gallery* train, const int32_t* labels, const int32_t* rows, int64_t n_rows,
                        float loss_weight, float* dW, float* db, float* loss);
int vv_linear_scores_rows(vv_ctx* ctx, vv_linear* lin, vv_gallery* src, const int32_t* rows, int64_t n_rows, float* out_dev);
int vv_rows_shuffled(uint64_t seed, int32_t n, int32_t epochs, int32_t* out);
int vv_rows_fold(uint64_t seed, int32_t n, int32_t folds, int32_t fold, int32_t* train, int64_t* n_train, int32_t* held,
                 int64_t* n_held);

/* ---- per-layer operators.  The reference's operator interface is Layer<Dtype>::{Forward_gpu, Backward_gpu}
 * (include/caffe/layer.hpp:308-337); its sequential executor (Net::ForwardFromTo / BackwardFromTo, net.cpp:501-578) calls
 * them layer by layer.  Training here runs the fused plan above; these entry points are what the C++ facade's layer classes
 * call when a graph is executed layer by layer (a graph the fused-plan matcher does not recognise, gradient checks, a
 * single Layer::Forward).  All buffers are fp32 DEVICE memory of this context (vv_dev_alloc; SyncedMemory's GPU side,
 * src/caffe/syncedmem.cpp:55-109), row-major; everything is queued on the context's stream.
 *   vv_op_copy2d      rows x cols block copy between strided buffers, optionally accumulating: SLICE / CONCAT forward and
 *                     backward (slice_layer.cu:10-64, concat_layer.cu:10-75), SPLIT's diff sum (split_layer.cu:18-33)
 *   vv_op_axpby       y = a x + b y: ELTWISE SUM with coefficients (eltwise_layer.cu:40-45, 99-105), diff accumulation
 *   vv_op_mul         y (+)= a .* b: ELTWISE PROD forward and its stable-product backward (eltwise_layer.cu:36-38, 83-97)
 *   vv_op_relu(_bwd)  relu_layer.cu:10-59, with negative_slope
 *   vv_op_dropout     dropout_layer.cu:14-73: make_mask = 1 draws the mask (counter-based hash of seed and element index)
 *                     and applies it; make_mask = 0 applies an existing mask -- the TRAIN backward, y = dy, with the same mask
 *   vv_op_rowsum(_bwd)     SUM (sum_layer.cu:10-55): row sums replicated num_output times; backward broadcasts
 *   vv_op_normalize(_bwd)  NORMALIZATION (normalization_layer.cu:10-97), eps placement of the reference (quirk Q6)
 *   vv_op_max_margin(_bwd) MAX_MARGIN_LOSS (max_margin_loss_layer.cpp:53-214; CPU-only in the reference): weight NULL or
 *                     one non-negative weight per term; forward synchronises and returns loss / violations to the host
 *   vv_op_gather_rows the data layer's batch copy (base_data_layer.cu:7-21): table rows idx (host int32 [n], -1 = zeros) as fp32
 *   vv_op_inner_product(_bwd)  INNER_PRODUCT with the context's parameters (inner_product_layer.cu:12-59): Y = X W^T + b;
 *                     backward writes dW (scaled by 1 + regularization / 2 when > 0) and db into the flat gradient buffer,
 *                     from which vv_apply_update updates.  No gradient w.r.t. X (the layer sits on the data layer).
 *   vv_op_gram        out [n][n] = alpha x x^T for x [n][dim]: the distance matrix of RETRIEVAL_STATS (retrieval_stats_layer.cpp:208-209,
 *                     alpha = -2), the launch vv_retrieval_stats makes; n < 1 or dim < 1: VV_ERR_ARG */
int vv_dev_alloc(vv_ctx* ctx, size_t bytes, void** out);     /* zero-filled */
int vv_dev_free(vv_ctx* ctx, void* p);
int vv_dev_upload(vv_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int vv_dev_download(vv_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int vv_dev_memset(vv_ctx* ctx, void* dst_dev, int value, size_t bytes);
int vv_op_copy2d(vv_ctx* ctx, const float* src, int64_t src_stride, float* dst, int64_t dst_stride, int64_t rows, int64_t cols,
                 int accumulate);
int vv_op_axpby(vv_ctx* ctx, int64_t n, float a, const float* x, float b, float* y);
int vv_op_mul(vv_ctx* ctx, int64_t n, const float* a, const float* b, float* y, int accumulate);
int vv_op_relu(vv_ctx* ctx, int64_t n, const float* x, float* y, float negative_slope);
int vv_op_relu_bwd(vv_ctx* ctx, int64_t n, const float* x, const float* dy, float* dx, float negative_slope);
int vv_op_dropout(vv_ctx* ctx, int64_t n, const float* x, float* y, uint8_t* mask, float ratio, uint64_t seed, int make_mask);
int vv_op_rowsum(vv_ctx* ctx, int64_t rows, int32_t cols, const float* x, int32_t num_output, float* y);
int vv_op_rowsum_bwd(vv_ctx* ctx, int64_t rows, int32_t cols, int32_t num_output, const float* dy, float* dx);
int vv_op_normalize(vv_ctx* ctx, int64_t rows, int32_t cols, const float* x, float* y);
int vv_op_normalize_bwd(vv_ctx* ctx, int64_t rows, int32_t cols, const float* x, const float* dy, float* dx);
int vv_op_max_margin(vv_ctx* ctx, int32_t count, const float* s_true, const float* s_bogus, const float* weight, float margin,
                     int32_t norm, float* loss, float* violations);
int vv_op_max_margin_bwd(vv_ctx* ctx, int32_t count, const float* s_true, const float* s_bogus, const float* weight, float margin,
                         int32_t norm, float loss_weight, float* d_true, float* d_bogus);
int vv_op_gather_rows(vv_ctx* ctx, const int32_t* idx, int64_t n, float* out);
int vv_op_inner_product(vv_ctx* ctx, const float* X, int64_t R, float* Y);
int vv_op_inner_product_bwd(vv_ctx* ctx, const float* dY, int64_t R, float ip_regularization);
int vv_op_gram(vv_ctx* ctx, const float* x_dev, int32_t n, int32_t dim, float alpha, float* out_dev);

/* ---- triplet sampler (host side, integer only).  Replaces VideoSampledShotsDataLayer's
 * DataLayerSetUp / AddSamplesToTop / InternalThreadEntry / AddToBuffer / RandomShuffleTopids
 * (src/caffe/layers/video_sampled_shots_data_layer.cpp:24-44,64-369,371-507,768-909) with the
 * feature copies replaced by table-row indices.  The draw order of the reference's libc rand()
 * stream (never seeded => glibc seed 1), include/caffe/util/rng.hpp:43-54's random_unique and
 * libstdc++'s std::random_shuffle are reproduced exactly, so indices are bit-identical.
 * One DB record = one video: record v has video_id[v], n_shots[v] frames whose features are table
 * rows row_base[v] .. row_base[v]+n_shots[v]-1, and shot ids shot_ids[shot_off..] (NULL = 0..n-1).
 * context_type: see VV_CONTEXT_* below. */
typedef struct vv_sampler vv_sampler;
typedef struct {
  int32_t batch_size, context_size, num_negative_samples;
  int32_t max_buffer_size, negative_swap_percentage, max_same_video_negs;
  int32_t max_tries_for_negs;      /* gflag --max_tries_for_negs, default 100 (...data_layer.cpp:20) */
  int32_t context_type;            /* VV_CONTEXT_* (VideoSampledShotsDataParameter.ContextType) */
  int32_t initial_cursor;          /* records skipped before anything else (rand_skip, ...data_layer.cpp:156-180): the DB
                                      cursor starts at this record (modulo the record count) */
  int32_t output_shot_distance;    /* PAIRWISE only (...data_layer.cpp:71, 407-418): label = frame distance, not video id */
  float   max_shot_distance;       /* ... clamped to this bound (caffe.proto:674, default 5) */
  int32_t rand_seed;               /* srand() argument of the draw stream.  0 or 1 = the reference's (it never seeds: glibc's seed
                                      1).  Other values (< 2^31 - 1) give each data-parallel rank its own stream (per-rank
                                      samplers); the stream is still glibc's rand() after srand(rand_seed) */
} vv_sampler_param;
/* WINDOW (...data_layer.cpp:425-507): target = the middle of C sorted random frames.  PAST (:510-596): target = the
 * last of C sorted random frames.  PAST_CONTINUOUS (:599-674): C equally spaced frames, random stride and start,
 * target = the last.  PAST_CONTINUOUS_FIXED (:677-757): the same with the largest stride minus one, ending at the
 * video's end.  PAIRWISE (:396-422): two distinct random frames in draw order (target, then the one context frame),
 * context_size forced to 2 (:200-201), records with one shot skipped; with output_shot_distance the label is their
 * distance.  All fill the same (B, C+Nn) layout. */
enum { VV_CONTEXT_WINDOW = 0, VV_CONTEXT_PAST = 1, VV_CONTEXT_PAST_CONTINUOUS = 2, VV_CONTEXT_PAST_CONTINUOUS_FIXED = 3,
       VV_CONTEXT_PAIRWISE = 4 };
void vv_sampler_param_default(vv_sampler_param* p);
int vv_sampler_create(const vv_sampler_param* p, int32_t n_videos, const int32_t* video_id,
                      const int32_t* n_shots, const int64_t* row_base, const int32_t* shot_ids,
                      vv_sampler** out);
/* The same with VideoSampledShotsDataParameter.negative_dataset (...data_layer.cpp:105-151, 253-286, 325-341): the
 * negative buffer starts as EVERY shot of the negative dataset's records taken in order (no rand() draw, the main
 * cursor stays at initial_cursor) and must come out exactly full -- the reference tests the fill level only after a
 * whole record and overruns its buffer otherwise, so anything but an exact fit is VV_ERR_ARG.  neg_row_base index
 * the same feature table as row_base.  neg_videos == 0 is vv_sampler_create. */
int vv_sampler_create_neg(const vv_sampler_param* p, int32_t n_videos, const int32_t* video_id,
                          const int32_t* n_shots, const int64_t* row_base, const int32_t* shot_ids,
                          int32_t neg_videos, const int32_t* neg_video_id, const int32_t* neg_n_shots,
                          const int64_t* neg_row_base, const int32_t* neg_shot_ids, vv_sampler** out);
/* One prefetch batch.  idx / last_src: int32 [batch_size][context_size + num_negative_samples]
 * (last_src: the row whose LAST feature the slot holds -- differs from idx only for same-video
 * negatives, which the reference copies without their last element, ...data_layer.cpp:492; -1 =
 * zero); label: int32 [batch_size] video ids (...:879).  Any output may be NULL. */
int vv_sampler_next(vv_sampler* s, int32_t* idx, int32_t* last_src, int32_t* label);
int vv_sampler_destroy(vv_sampler* s);

/* ---- prefetch.  Replaces BasePrefetchingDataLayer::{CreatePrefetchThread, JoinPrefetchThread}
 * (src/caffe/layers/base_data_layer.cpp:52-95) and InternalThread (src/caffe/internal_thread.cpp:14-37): the
 * reference starts one thread per batch that fills prefetch_data_ while the solver consumes the previous one.
 * Here background threads run `depth` batches ahead of the consumer; afterwards vv_sampler_next pops finished
 * batches in order (the index stream is exactly the one vv_sampler_next would have produced by itself).
 *   threads   1 = whole batches on one thread; 2, 3 or 4 = the item's three chains (stream walk + buffer swap-in /
 *             negative-slot draw / frame draw) as a pipeline of threads, the fourth generating the rand() stream a
 *             block ahead of the walk (same indices; only for samplers without same-video negatives whose
 *             (video_id, shot_id) keys name distinct rows, else 1 is used).
 *   shm_name  NULL = a private ring.  A name = the ring lives in a POSIX shared-memory object of that name, so that
 *             ONE sampler per node serves `consumers` processes (the data-parallel ranks: every rank takes its
 *             items of the same global batch) -- see vv_batch_ring_attach.
 *   consumers number of readers that must each take (a slice of) a batch before its buffer is reused. */
int vv_sampler_prefetch_start(vv_sampler* s, int32_t depth, int32_t threads, const char* shm_name, int32_t consumers);
int vv_sampler_prefetch_stop(vv_sampler* s);
/* Counters for tests and tuning: which = 0 swap-in walks that had to restart (a swap-in evicted a later shot of the same
 * video), 1 = the staged fast path is in use (0/1), 2 = producer threads of the running prefetch, 3 = time-stamp-counter
 * ticks since the pipeline started, 4 / 5 / 6 = ticks of them the walk / negative-slot / frame stage spent waiting,
 * 7 = the 512-bit forms of the walk and the slot draw are in use (0/1: the host has AVX-512 F/BW/DQ/VL/VBMI2 and
 * VV_SAMPLER_AVX512 is not 0; same indices either way), 8 = ticks the walk stage waited for the stream-generating
 * thread (four-thread pipeline), 9 = cores held for the stage threads (4: one each, claimed against other samplers
 * of the host through /dev/shm/vv_sampler_cpu_<n> locks; 0: the threads share the caller's group of CPUs), 10 = whole batches the
 * running pipeline has produced, 11 = batches its consumers have all taken (10 minus 11 = how far the pipeline is ahead; both -1
 * without a pipeline).  -1 = unknown. */
int64_t vv_sampler_stat(vv_sampler* s, int32_t which);

/* A reader's view of a sampler's batch ring.  vv_sampler_ring: the producer process's own handle (owned by the
 * sampler).  vv_batch_ring_attach: map the named ring of another process (waits up to timeout_s for it to appear).
 * vv_batch_ring_next: wait for this consumer's next batch (timeout_s <= 0: forever; VV_ERR_STATE when the producer
 * has gone or the wait timed out), copy items [item_begin, item_begin + item_count) -- idx int32 [item_count][C+Nn],
 * label int32 [item_count], either may be NULL -- and release the batch for this consumer. */
typedef struct vv_batch_ring vv_batch_ring;
int vv_sampler_ring(vv_sampler* s, vv_batch_ring** out);
int vv_batch_ring_attach(const char* shm_name, double timeout_s, vv_batch_ring** out);
int vv_batch_ring_info(vv_batch_ring* r, int32_t* batch_size, int32_t* slots_per_item, int32_t* consumers, int32_t* depth);
int vv_batch_ring_next(vv_batch_ring* r, int32_t consumer, int32_t item_begin, int32_t item_count, int32_t* idx,
                       int32_t* label, double timeout_s);
int vv_batch_ring_detach(vv_batch_ring* r);

/* ---- the sampler's state, for a run that resumes bit for bit.  The reference's snapshot (Solver::Snapshot / SGDSolver::SnapshotSolverState,
 * src/caffe/solver.cpp:320-341, 578-596) saves the iteration, the learned net and the history and NOTHING of the data layer: neither the DB
 * cursor, nor the negative buffer, nor the rand() state that its batch loop (video_sampled_shots_data_layer.cpp:768-909) carries from one
 * batch to the next, so a restored reference run reads the run's first batches again.  These three calls carry that state.
 * The state meant is that of the reference's ONE sequential stream after the last batch DELIVERED to the consumer -- returned by
 * vv_sampler_next, or taken from the ring by its single consumer -- not after the last batch the prefetch pipeline has produced:
 *   the libc stream (its 31 state words, oldest first: the order is the position), the DB cursor and the negative dataset's own, the
 *   negative buffer (rows, keys; the membership set or bitmap is rebuilt from them), the persistent slot permutation (buffer_ids_), and on
 *   the general path the persistent slot contents that quirk Q1's last_src depends on.
 * The blob is opaque: a magic, a version, a fingerprint (every field of vv_sampler_param, the number of videos, the shot counts, the
 * negative dataset's shape; bytes [24, 112)) and the state.  Its size depends on the fingerprint alone (vv_sampler_state_size).
 * vv_sampler_state_get: never changes a batch delivered later, with the pipeline running or not; two calls with no batch delivered in
 *   between return identical bytes.  With the pipeline running nothing is stopped or rewound: a private serial sampler is replayed, in the
 *   calling thread, over the batches delivered since vv_sampler_prefetch_start or the previous call (the cost falls here, not on a batch).
 *   Call it from the consumer's thread, or while the consumer is quiet.  cap < the state's size: VV_ERR_ARG.  VV_ERR_STATE where no single
 *   consumer position exists: a ring with more than one consumer, VV_SAMPLER_MODE=node in the environment, after vv_sampler_prefetch_stop
 *   (it drops batches the pipeline has produced).
 * vv_sampler_state_put: only on a sampler that has neither delivered a batch nor started its pipeline, else VV_ERR_STATE.  A blob of
 *   another fingerprint, a truncated, over-long or damaged one: VV_ERR_ARG; nothing past `bytes` is read and the sampler is untouched.
 * vv_sampler_state_error: this thread's last message of these calls (which fingerprint field differs, and how). */
int vv_sampler_state_size(vv_sampler* s, int64_t* bytes);
int vv_sampler_state_get(vv_sampler* s, void* buf, int64_t cap, int64_t* written);
int vv_sampler_state_put(vv_sampler* s, const void* buf, int64_t bytes);
const char* vv_sampler_state_error(void);
/* BasePrefetchingDataLayer::Forward_gpu (src/caffe/layers/base_data_layer.cu:7-21: join the prefetch thread, copy the
 * batch to the device) + Net::ForwardBackward: take this consumer's next batch out of the ring -- items
 * [item_begin, item_begin + cfg->B) of it -- send the indices to the device through a pinned staging buffer with an
 * asynchronous copy on the context's stream, and queue vv_forward_backward on them.  label_out: host int32 [B] or NULL. */
int vv_forward_backward_ring(vv_ctx* ctx, const vv_step_cfg* cfg, vv_batch_ring* ring, int32_t consumer,
                             int32_t item_begin, int32_t* label_out, double timeout_s);

/* Timing hook for the benchmark: average device time in ms of one named kernel ("fwd_gemm",
 * "score_loss", "wgrad_gemm", "reduce", "sgd") over the launches since the last reset, measured
 * with hipEvents on the context's stream (only while enabled; enabling adds two event records
 * per launch). */
/* on: 0 = off, 1 = every step, N > 1 = the N-th, 2N-th, ... step after the call (a step ends with vv_apply_update).  The events ride on the
 * kernels' own dispatch packets (hipExtLaunchKernelGGL); no extra packets are queued. */
int vv_profile_enable(vv_ctx* ctx, int on);
/* Restrict the timing to a comma-separated list of kernel names (NULL or "" = all).  A timed dispatch cannot be pipelined
 * behind its predecessor (~5 us each): the benchmark's timed leg times the two GEMMs only. */
int vv_profile_select(vv_ctx* ctx, const char* kernels);
int vv_profile_get(vv_ctx* ctx, const char* kernel, double* avg_ms, int64_t* launches);

/* Box calibration for the benchmark: what THIS device delivers at the moment of the call, so that step times measured on different boxes of
 * a pool can be compared (the step's GEMMs run at whatever clock the chip holds under them).  No reference counterpart: `caffe device_query`
 * (tools/caffe.cpp:108-121, Caffe::DeviceQuery, src/caffe/common.cpp:147-180) prints static properties only.  Two fixed probes on buffers of
 * their own (2.2 GB, released before the call returns), queued on the context's stream, ~10 ms of device time:
 *   gemm  the benchmark's forward instantiation (f16 operands, 192-row tiles, 216 workgroups) on CONTIGUOUS rows of a random table,
 *         20 736 x 4096 x 512, operands uniform in [-1, 1): TFLOP/s over 24 back-to-back launches behind 8 warm-up launches, and the shader
 *         clock held inside the kernel (s_memtime over s_memrealtime, median over its workgroups)
 *   copy  a 1 GiB device-to-device streaming copy: bytes read + written per second over 6 copies behind 2 */
typedef struct {
  double gemm_tflops, gemm_ms, gemm_clock_mhz;
  double copy_tbs, copy_ms;
  int32_t gemm_rows, gemm_k, gemm_n, gemm_launches;
  int64_t copy_bytes;
} vv_box_probe_result;
int vv_box_probe(vv_ctx* ctx, vv_box_probe_result* out);

#ifdef __cplusplus
}
#endif
#endif
