// vv_internal.h -- shared declarations of the HIP implementation behind include/videovec.h.
// gfx950 (MI355X, CDNA4) only.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <type_traits>

#include "vv_pass_plan.h"      // score_fwd_supported / score_fwd_dropout_supported: the shapes the segment-wise pair is built for
#include "vv_gallery_plan.h"   // the RT_* sizes the gallery scratch is made of, its limits and its sizing arithmetic
#include "vv_kmeans_plan.h"    // the KM_* sizes of vv_gallery_kmeans and its block plan
#include "vv_ivf_plan.h"       // the IVF_* sizes of vv_ivf_search and its block plan
#include "vv_pq_plan.h"        // the PQ_* limits of product quantisation and vv_ivfpq_search's block plan

struct vv_gallery;

namespace vv {

// Floats between two split-K slabs of the weight gradient.  Exactly D_p x F_p (8 MiB at 512 x 4096) puts the eight streams that k_reduce /
// k_reduce_sgd read side by side a power of two apart, and a reader of the slabs alone gains 11 % from 4 KiB of skew (3.93 -> 4.38 TB/s,
// tools/lab/slab_pitch_lab.hip) -- but in the step k_reduce_sgd's 0.9 us are given back by the weight-gradient GEMM's stores (+0.7 us),
// alternating builds on one box (profiles/r05_slab_pitch.txt): the pad stays 0; -DVV_SLAB_PAD=<floats> builds the other form.
#ifndef VV_SLAB_PAD
#define VV_SLAB_PAD 0
#endif
__host__ __device__ inline int64_t slab_pitch(int Dp, int Fp) { return (int64_t)Dp * Fp + VV_SLAB_PAD; }


// ---------------------------------------------------------------------------------------------
// GEMM tiling shared by the forward (gather-GEMM) and weight-gradient (gather-GEMM^T) kernels.
// One workgroup = 512 threads = 8 waves (2 along M x 4 along N), one 256x256 output tile,
// K advanced 64 at a time through a double-buffered LDS image filled by LDS-DMA
// (global_load_lds_dwordx4).  Each wave owns a 128x64 sub-tile = 8x4 MFMA 16x16x32 accumulators.
// ---------------------------------------------------------------------------------------------
constexpr int BM = 256, BN = 256, BK = 64;
constexpr int GEMM_THREADS = 512;
constexpr int LDS_TILE_BYTES = 256 * 64 * 2;          // one operand tile: 32 KiB
constexpr int GEMM_LDS_BYTES = 4 * LDS_TILE_BYTES;    // {A,B} x 2 buffers = 128 KiB

// Row padding rules of the half-precision operand copies kept in HBM.
constexpr int F_ALIGN = 256;   // table / W row length (K of fwd, N of wgrad)
constexpr int D_ALIGN = 256;   // W rows (N of fwd), dY row length (M of wgrad)
constexpr int R_ALIGN = 256;   // batch rows (M of fwd, K of wgrad)
constexpr int SGD_BLOCKS = 1024;

inline __host__ __device__ int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// Device-resident scale block: power-of-two factors that keep f16 operands in range.
//   table_h = x * sx          (fixed at table load)
//   W_h     = W * sw_cur      (refreshed by the SGD kernel each step)
//   dY_h    = dY * sg         (sg chosen per step from the loss count)
struct Scales {
  float sx;            // table scale
  float sw_cur;        // scale the current W_h copy carries
  float sw_next;       // scale the next W -> W_h conversion will use
  unsigned wmax_bits;  // running max |W| (float bits) collected by the SGD kernel
};

// f16 gradient-scale guard.  The 16-bit gradient operand of the weight-gradient GEMM carries ONE power-of-two scale per
// step (the host's sg).  A value past f16's range must never reach the GEMM clipped, so every kernel that rounds
// gradients to 16 bits ("producer": k_score_loss / k_score_loss_reg, k_segsum, k_seg_bwd) records its per-block max |g|
// (before rounding) and raises flag[round] when one passes GG_LIMIT; the host then launches the same producers once
// more per guard round as conditional REPEATS: a repeat whose previous round raised no flag returns at once (the normal
// case: one near-empty launch), otherwise it folds the recorded maxima, takes the excess powers of two off the scale
// (max placed at 2^12) and produces its output again.  k_reduce undoes sg * mul.  Exact: powers of two only.
struct GradGuard {
  int32_t flag[4];           // flag[r] == seq: round r of step seq produced a value past GG_LIMIT
  int32_t shift[4];          // shift[r], r = 1, 2: powers of two taken off the host's scale from round r on (cumulative);
                             // shift[3]: the step's final shift
  float mul;                 // 2^-shift of the step's last round
  int32_t repeat_seq;        // the last step in which a conditional repeat really ran
  int32_t pad[2];
};
constexpr float GG_LIMIT = 32768.f;
// The step's report entry in the host-visible ring (vv_ctx::gmax_host: GMAX_ENTRIES of them, written by reduce_loss, read by the host at a
// fixed lag): word 0 the sequence number | bits(max |dY|) << 32 (stored last, release), word 1 the guard's shifts and flags, words 2 and 3
// the f16 ip2 rows' saturated elements and faint rows (option "h16_guard").  Internal.
constexpr int GMAX_ENTRY_WORDS = 4, GMAX_ENTRIES = 16;
struct GuardArgs {
  GradGuard* gg = nullptr;   // null: no guard (bf16 operands: fp32's exponent range)
  float* slots = nullptr;    // [3 rounds][2 producers][nslot] per-block max |g| in the units of that round's scale
  int nslot = 0;
  int producer = 0;          // which producer of the round this launch is (0, 1)
  int n_of[2] = {0, 0};      // blocks of producer 0 / 1 (0: that producer does not exist)
  int round = 0;             // 0: the step's normal pass; r >= 1: the r-th conditional repeat
  int last = 0;              // this launch closes the round (writes shift[round]) ...
  int final_round = 0;       // ... and the round is the step's last (publishes mul)
  int32_t seq = 0;
  // PROACTIVE form (the segment-wise backward: k_score_fwd / k_score_stream + k_seg_bwd): no repeat launch.  The score kernel
  // knows every instance's factored gradient (alpha, beta, the vector it multiplies) and bounds its largest element:
  // |alpha| max|Ah_d| + |beta| max|x_d| <= |alpha| + |beta| |x| for a target / negative instance, |alpha| 4 sA gsum /
  // (sA^1.5 + eps) for a context instance; it leaves the batch's maximum in *bound (tagged with the step's sequence number, so
  // that nothing has to reset it).  A distinct row's sum is at most (its instance count) x that, the grouping kernels leave the
  // largest instance count in *cnt_max: k_seg_bwd takes 2^-shift off the scale BEFORE it rounds anything whenever
  // cnt_max x bound could pass 2^15.  Rigorous (a bound, not an estimate), and loose by design: a shift that was not
  // needed costs nothing while the values stay normal f16 numbers.
  int proactive = 0;
  const unsigned long long* bound = nullptr;   // GG_BOUND_SLOTS words, one 128-B line each (an item adds to slot blockIdx % 64: a
  const int32_t* cnt_max = nullptr;            //   thousand atomics on ONE word cost the score kernel 4 us of serialisation)
};
constexpr int GG_BOUND_SLOTS = 64, GG_BOUND_STRIDE = 16;     // (stride in 8-byte words)
#ifdef __HIPCC__
// the batch's largest per-instance element bound: max over the slots that carry this step's sequence number (every lane alike)
__device__ __forceinline__ float gg_bound_fold(const unsigned long long* bound, int32_t seq) {
  const unsigned long long w = bound[(threadIdx.x & (GG_BOUND_SLOTS - 1)) * GG_BOUND_STRIDE];
  float m = (unsigned)(w >> 32) == (unsigned)seq ? __uint_as_float((unsigned)w) : 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  return m;
}
#endif

struct FwdArgs {
  const uint16_t* table;   // [n_rows + 1][Fp], last row all zero
  const int32_t* rows;     // [Rp] table row per batch row (already mapped, padding -> zero row)
  const uint16_t* Wh;      // [Dp][Fp]
  const float* bias;       // [D] or null
  const Scales* scales;
  float* H;                // [R][D] fp32 output (ip2)
  int R, D, Fp;
  int32_t zero_row;        // table row of zeros (for rows past R inside the last tile)
  int relu;
  // dropout
  float drop_ratio;        // 0 = off
  const uint8_t* mask;     // explicit mask [(C+Nn)*B][D] in reference row order, or null
  uint64_t drop_seed;
  int B, CN;               // to map an internal row (b*CN+ch) to the reference row (ch*B+b)
  const int32_t* n_dev = nullptr;   // dedup mode: device count of valid rows (overrides R; the grid covers R)
  int R_hint = 0;              // dedup mode: expected row count, sizes the tiles (0 = R)
  int32_t* seq_host = nullptr; // host-mapped word that receives `seq` (the step's index batch has been consumed), or null
  int32_t seq = 0;
  int abl = 0;                 // timing studies only (VV_ABLATE): selects an ablated instantiation of the phase-staggered kernel
  // Data-parallel overlap (solver.hip: vv_apply_update): the parameter update of the PREVIOUS step may still be arriving --
  // F-chunk by F-chunk, each chunk all-reduced and applied on the communication stream -- while this kernel runs.
  // gate[c * W_GATE_STRIDE] holds the sequence number of the last update whose chunk c (K-tiles [gate_kt[c], gate_kt[c+1])
  // of W) is complete; a workgroup waits for it to reach gate_seq before it issues its first load of a W tile of chunk c.
  // null = no gating.
  const int32_t* gate = nullptr;
  int32_t gate_seq = 0;
  int gate_n = 0;              // chunks (1 .. W_CHUNKS_MAX)
  int gate_kt[5] = {0, 0, 0, 0, 0};   // first K-tile of each chunk (even; gate_kt[0] = 0, gate_kt[gate_n] = all K-tiles)
  int32_t* gate_err = nullptr; // host-mapped: set when a wait gave up (bounded: a lost update must not hang the device)
  // H as 16-bit floats (round 6, option "h16"): the forward GEMM stores ip2 as f16 -- [R][D] halves in the same buffer, scale 1, values past
  // f16's range saturated at +-65504 -- for the kernels that then read it as such (k_score_fwd / k_score_stream / k_seg_bwd: ScoreArgs::h16).
  // Only the segment-wise path sets it (pass.hip); everything else keeps fp32 rows.
  int h16 = 0;
};
constexpr int W_CHUNKS_MAX = 4; // F-chunks of the overlapped update at most (chunk-major gradient buffer, pass.hip: vv_chunk_plan)
constexpr int W_GATE_STRIDE = 32;   // ints between two chunk flags: a 128-B line each (the waiting workgroups poll them)

// Segment-wise backward (de-duplicated batches): the score kernel keeps the gradient of an instance in factored form
// -- dY[r] = [x_u > 0] (alpha_r V[vec_r] - beta_r x_u), where V holds the item's normalised context mean Ah_b (row 2b:
// target / negative instances, alpha = c n^2/den, beta = c t/den) and the gradient of its context mean dA_b (row 2b+1:
// context instances, alpha = c_j, beta = 0) -- and writes one 16-byte record per instance at its grouped position.
// k_seg_bwd then produces, per distinct row u, dYu[u] = [x_u > 0] (sum_r alpha_r V[vec_r] - (sum_r beta_r) x_u) from
// the records of its instances: the per-instance 16-bit gradient rows ((C+Nn) B D values written and read back) are
// never materialised.
// The dropout mask of the path as a function (drop2 sits behind fc7 + ReLU, mednet_embedding_train.prototxt:220-230): element (reference
// row r = ch B + b, column n).  mode 1: counter hash -- quad n / 4 of row r owns counters row_ctr(r) + 2 (n / 4) + {0, 1}, each 32-bit hash
// gives two 16-bit uniforms, keep <=> uniform >= thr; mode 2: the caller's explicit mask[r D + n].  The forward GEMM's epilogue (dense
// execution) and the score / segment kernels (de-duplicated execution: the projection is shared, the mask is per instance) evaluate the SAME
// function, so the two executions drop the same elements.
struct DropSpec {
  int mode = 0;                    // 0 none, 1 counter hash, 2 explicit mask
  uint32_t thr = 0, s32 = 0;       // mode 1: threshold on the 16-bit uniform, the step's stream
  float scale = 1.f;               // 1 / (1 - ratio)
  const uint8_t* mask = nullptr;   // mode 2
  int B = 0, CN = 0, D = 0;
};
__device__ __forceinline__ uint32_t drop_mix32(uint32_t x) {     // (two multiply-xorshift rounds: C. Wellons' "lowbias32" constants)
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t drop_row_ctr(int64_t ref_row, int D, uint32_t s32) {
  const uint64_t r2 = (uint64_t)ref_row * (uint64_t)(2 * ((D + 3) >> 2));
  return (uint32_t)r2 + (uint32_t)(r2 >> 32) * 0x9E3779B9u + s32;
}
// keep bits of columns n .. n + 3 (n a multiple of 4) of reference row ref_row; bit j = column n + j
__device__ __forceinline__ uint32_t drop_keep4(const DropSpec& d, int64_t ref_row, uint32_t row_ctr, int n) {
  if (d.mode == 2) {
    const uint32_t m = *(const uint32_t*)(d.mask + (uint64_t)ref_row * d.D + n);       // (D a multiple of 4 on these paths)
    return ((m & 0xffu) != 0) | (((m >> 8) & 0xffu) != 0) << 1 | (((m >> 16) & 0xffu) != 0) << 2 | ((m >> 24) != 0) << 3;
  }
  const uint32_t c0 = row_ctr + (uint32_t)(n >> 1);
  const uint32_t h0 = drop_mix32(c0), h1 = drop_mix32(c0 + 1u);
  return ((h0 & 0xffffu) >= d.thr) | ((h0 >> 16) >= d.thr) << 1 | ((h1 & 0xffffu) >= d.thr) << 2 | ((h1 >> 16) >= d.thr) << 3;
}

struct SegRec { float alpha, beta; int32_t vec; int32_t pad; };   // pad: the instance index b (C+Nn) + ch (sets the summation order)
constexpr int SEGB_BLOCKS = 1024;     // persistent grid of k_seg_bwd = rows of its bias partials

struct ScoreArgs {
  const float* H;          // [R][D] item-major rows (b*CN + ch)
  uint16_t* dYh;           // [Rp][Dp] scaled half gradient of ip1_nonorm
  float* dbp;              // [B][D] per-item column sums of dY (fp32, unscaled)
  float* loss_part;        // [B]
  float* viol_part;        // [B]
  float* s_true;           // [B] (replicated Nn times by the reference's SUM layer)
  float* s_bogus;          // [B][Nn]
  const float* coeff;      // [C-1] device
  int B, C, Nn, D, Dp;
  float margin; int norm;
  float grad_scale;        // loss_weight / global_count
  float drop_scale;        // 1/(1-ratio) or 1
  float sg;                // half-precision gradient scale
  // row-dedup mode (both NULL otherwise): H holds one row per UNIQUE table row, instance r reads
  // H[map[r]] and writes its gradient row to dYh[seg_start[map[r]] + ord[r]] (instances of one unique row contiguous)
  const float* item_w = nullptr;     // [B] loss-term weight of each item (MAX_MARGIN_LOSS 3rd bottom) or null
  const int32_t* map = nullptr;      // [R]
  const int32_t* seg_start = nullptr;  // [U + 1]   pos[r] = seg_start[map[r]] + ord[r]
  const int32_t* ord = nullptr;      // [R]
  GuardArgs guard;                   // f16 gradient-scale guard (kernels that write dYh)
  int items_rr = 0;                  // (lab, KernelOpts::score_rr) workgroup -> item round-robin instead of by XCD ranges
  int32_t* gate_host = nullptr;      // host-mapped word that receives gate_seq when the kernel starts ("the forward GEMM
  int32_t gate_seq = 0;              //   of this step has finished": releases the host to queue a later step's grouping)
  // segment-wise backward (launch_score_fwd): outputs instead of dYh / dbp
  float* V = nullptr;                // [2B][D]
  SegRec* rec = nullptr;             // [R]
  unsigned long long* bound_out = nullptr;   // GuardArgs::bound: (seq << 32) | bits of the largest per-instance element bound
  int32_t bound_seq = 0;
  int fwd_only = 0;                  // vv_forward: the launchers pick the forward-only instantiations (template parameter FWD) -- scores, loss and violation
                                     // partials only; dYh / dbp / V / rec / bound_out / guard are not read.  (Sits in what was padding in front of
                                     // `drop`: every other field, and the kernels' hidden arguments behind the struct, keep their offsets)
  DropSpec drop;                    // de-duplicated execution with dropout (k_score_fwd): H holds the SHARED pre-dropout rows, every
                                     // instance applies its own mask as it reads its row
  int h16 = 0;                       // H holds f16 rows (FwdArgs::h16): launch_score_fwd's kernels only
  int v16 = 0;                       // V leaves as f16 (k_score_stream's V16 form; needs h16): SegBwdArgs::v16
  int prefetch = 0;                  // k_score_fwd, f16 rows: first-round workgroups touch the second round's rows into the XCD's L2 (KernelOpts::score_pf)
  int lab_hack = 0;                  // (lab builds, VV_LAB_SCORE_HACK: timing studies of k_score_fwd's row loads -- WRONG results) 1: rows 1 KiB apart (half the footprint, the same requests), 2: only the first half of every row is loaded (half the bytes and requests)
  uint32_t* lab_ts = nullptr;        // (lab builds, VV_LAB_SCORE_TS=1: 16 words per item -- shader-clock stamps of k_score_fwd's phases, 100 MHz
                                     //  real time of its start and end, the compute unit it ran on; the product never sets or reads it)
};

// The forward-only evaluation pass (vv_forward; Net::Forward under phase TEST called test_iter times by Solver::Test): what vv_eval_stats
// reports, kept by k_eval_loss's first thread -- nothing synchronises per pass.  The sums are double: an fp32 value is exact in it, and
// they are added in pass order.
struct EvalRec {
  int64_t passes, terms;              // passes since vv_eval_reset, and their loss terms (B Nn each)
  double loss_sum, viol_sum;          // of last_loss / last_viol over those passes
  float last_loss, last_viol;         // the fp32 values vv_loss_get would show for the last pass
};

// Row de-duplication of one batch (kernels_dedup.hip).  The sampler draws the negatives of every item
// from one shared buffer (video_sampled_shots_data_layer.cpp:836-875), so a batch repeats table rows;
// the projection is computed once per unique row and the gradient rows of its instances are summed
// before the weight-gradient GEMM.
struct DedupArgs {
  int lds_bytes = 0;             // dynamic LDS the kernels ask for and never touch (placement, kernels_dedup.hip)
  const int32_t* idx;            // [R] batch indices as sampled (-1 = empty slot)
  int32_t* rows;                 // [Rp] instance -> table row, written by k_dd_claim (what k_map_rows writes)
  unsigned long long* key;       // [table rows + scratch] epoch-tagged leader election
  unsigned long long* agg;       // [2][agg_stride] epoch-tagged block aggregates of the two scans
  int agg_stride;
  int32_t* slot_of;              // [R] slot of the leader instances
  int32_t* uniq_rows;            // [Rp] slot -> table row (zero_row past U)
  int32_t* map;                  // [R] instance -> slot
  int32_t* ord;                  // [R] arrival order of the instance inside its segment
  int32_t* cnt;                  // [Rp] instances per slot
  int32_t* seg_start;            // [Rp + 1]
  int32_t* pos;                  // [R] instance -> row of the grouped gradient buffer
  int32_t* info;                 // device {U, ...}
  int32_t* tickets;              // device [2]: arrival counters of the two single-pass scans
  int32_t* u_host;               // host-mapped copy of U (read one or more steps late by the launcher)
  int R, Rp; int32_t zero_row; int32_t row_limit; uint32_t epoch;
};

struct SegBwdArgs {
  const float* H;                // [U][D] projection of the distinct rows (x_u)
  const float* V;                // [2B][D]
  const SegRec* rec;             // [R] grouped by slot: records of slot u are rec[seg_start[u] .. seg_start[u+1])
  const int32_t* seg_start;      // [U + 1]
  const int32_t* info;           // {U}
  uint16_t* dYu;                 // [Rp][Dp] (zero rows up to the next multiple of BK)
  float* dbp;                    // [SEGB_BLOCKS][D] column sums of the unrounded rows, unscaled
  int Rp, D, Dp;
  float inv_sg;
  GuardArgs guard;
  DropSpec drop;                 // as ScoreArgs::drop: dx_u = [x_u > 0] (sum_i m_i alpha_i V_i - x_u scale sum_i m_i beta_i), m_i the instance's mask
  int h16 = 0;                   // H holds f16 rows (FwdArgs::h16)
  int v16 = 0;                   // V holds f16 rows (ScoreArgs::v16: the one-sweep score kernel wrote them so)
  uint32_t* h16_cnt = nullptr;   // non-null (option "h16_guard" >= 1; f16 rows, guard round 0): [SEGB_BLOCKS][2] per-workgroup counts of the rows'
                                 //   {saturated elements, faint rows} (k_seg_bwd_cnt, kernels_score.hip); every workgroup writes its pair
};

struct SegsumArgs {
  const uint16_t* dYh;           // [R][Dp] instance gradient rows grouped by slot
  const int32_t* seg_start;      // [U + 1]
  const int32_t* info;           // {U}
  uint16_t* dYu;                 // [Rp][Dp] per-slot sums (zero rows up to the next multiple of BK)
  int Rp, Dp;
  GuardArgs guard;
};

// The solver's parameters as the three update kernels read them -- k_sgd, k_reduce_sgd and the weight-gradient GEMM's UPD epilogue, which
// must give bit-identical parameters -- and the rule itself (solver.hip: vv_solver_rule fills it from a vv_step_cfg and the context's
// vv_solver_ext_set values).
struct SolverRule {
  float rate, momentum, weight_decay;
  float lr_mult_w, lr_mult_b, decay_mult_w, decay_mult_b;
  int reg;                 // 1 L1, 2 L2
  int solver_type;         // 0 SGD, 1 Nesterov, 2 AdaGrad, 3 RMSProp, 5 Adam
  float delta;             // stability constant of AdaGrad, RMSProp and Adam
  // RMSProp and Adam (BVLC Caffe's RMSPropSolver / AdamSolver; the reference tree has neither).  Every 1 - x is formed ONCE, on the host, in
  // fp32: decay2 = rms_decay (RMSProp) or beta2 (Adam; beta1 is `momentum`), om1 = 1 - beta1, om2 = 1 - decay2;
  // corr = sqrt(1 - beta2^t) / (1 - beta1^t) of THIS update (computed in double, rounded once): a queued step carries its own
  float decay2 = 0.f, om1 = 0.f, om2 = 0.f, corr = 1.f;
#ifdef __HIPCC__
  // the regulariser (solver.cpp:502-531): g' = g + dc r
  __device__ __forceinline__ float regularise(float w, float g, float dc) const {
    if (dc != 0.f) g += dc * (reg == 2 ? w : (float)((w > 0.f) - (w < 0.f)));
    return g;
  }
  // one parameter element: regulariser, then SGD (solver.cpp:502-531), Nesterov (:599-655), AdaGrad (:714-781) or RMSProp (BVLC
  // RMSPropSolver::ComputeUpdateValue: h' = rms_decay h + (1 - rms_decay) g'^2, u = lr (g' / (sqrt(h') + delta))); h: its history.
  // lr / dc: the local rate and decay (rate and weight_decay times the blob's multipliers).
  // RMSProp shares the regulariser's statement with the three older rules -- g' formed exactly as today, contraction left to the
  // compiler -- and rounds its OWN products and sums in the order written (contraction off inside its branch).  A form of `step` that
  // took RMSProp out in front of the regulariser, to un-fuse that too, cost the weight-gradient epilogue 84-100 bytes of scratch per
  // lane: rejected.
  // RMS = false: the three older rules alone, instruction for instruction what they always were -- k_sgd and k_reduce_sgd give RMSProp
  // instantiations of its own (with the runtime branch in every instantiation k_reduce_sgd over f16 slabs ran 18.7 -> 19.2 us for SGD
  // at cfg 2 and the step missed the condition of DESIGN.md 3.5); the weight-gradient GEMM's epilogue keeps the branch (RMS = true).
  template <bool RMS = true>
  __device__ __forceinline__ float step(float w, float g, float& h, float lr, float dc) const {
    g = regularise(w, g, dc);
    float u;
    if (solver_type == 1) { const float h0 = h; h = lr * g + momentum * h0; u = (1.f + momentum) * h - momentum * h0; }
    else if (solver_type == 2) { h += g * g; u = lr * (g / (sqrtf(h) + delta)); }
    else if (RMS && solver_type == 3) {
#pragma clang fp contract(off)
      h = decay2 * h + om2 * (g * g); u = lr * (g / (sqrtf(h) + delta));
      return w - u;
    }
    else { h = lr * g + momentum * h; u = h; }
    return w - u;
  }
  // Adam lives in instantiations of its own, so it rounds EVERYTHING in the order written, the regulariser's product and sum included
  // (contraction off): left to the compiler, the scalar bias loops of k_sgd and k_reduce_sgd fused differently and the last bit of m and
  // v of a few bias elements depended on the form.  (So Adam's g' may differ in the last bit from the g' the other rules form.)
  // Adam (BVLC AdamSolver::ComputeUpdateValue), two histories: m' = beta1 m + (1 - beta1) g', v' = beta2 v + (1 - beta2) g'^2,
  // u = (lr corr_t) (m' / (sqrt(v') + delta)).  Only the two-history instantiations of k_sgd and k_reduce_sgd call it.
  __device__ __forceinline__ float step2(float w, float g, float& m, float& v, float lr, float dc) const {
#pragma clang fp contract(off)
    if (dc != 0.f) g = g + dc * (reg == 2 ? w : (float)((w > 0.f) - (w < 0.f)));
    m = momentum * m + om1 * g;
    v = decay2 * v + om2 * (g * g);
    return w - (lr * corr) * (m / (sqrtf(v) + delta));
  }
#endif
};

// The solver's update applied in the weight-gradient GEMM's epilogue (one split of K: the tile in the accumulators IS the gradient;
// pass.hip: vv_update_hint).  What k_reduce_sgd does per 16 bytes of W -- unscale, the solver's rule (solver.cpp:502-531 / 599-655 / 714-781),
// blob.cpp:112-136, the new 16-bit copy, max |w| for the next scale -- done on the 256 x 256 tile while it is in registers: the 4 D F
// bytes of dW are neither written nor read back.  Bias, loss and the guard's report stay with k_reduce_sgd's special workgroups.
struct WgradUpd {
  float* W; float* hW; uint16_t* Wh;
  Scales* scales;
  float* wmax_blocks;                    // one slot per workgroup of the GEMM (this update's per-block max |w|)
  const float* wmax_prev; int wmax_prev_n; int recompute_scale; int prec;      // as FusedUpdArgs
  int D, F;                              // the matrix (tiles are padded to Dp x Fp)
  SolverRule rule;                       // (the bias multipliers unused: the bias is k_reduce_sgd's)
  float sg; const GradGuard* gg; float ip_scale;          // dW = acc * ip_scale / (sg * gg->mul * sx), as ReduceArgs
};

struct WgradArgs {
  const uint16_t* dYh;     // [Rp][Dp]
  const uint16_t* table;   // [n_rows+1][Fp]
  const int32_t* rows;     // [Rp]
  float* slabs;            // [S][Dp][Fp] fp32 partial products
  int Rp, Dp, Fp;
  int S;                   // split-K factor
  int ksteps_per_split;    // BK-steps per split
  const int32_t* n_dev = nullptr;    // dedup mode: device count of valid K rows (overrides Rp / ksteps_per_split)
  int32_t zero_row = 0;              // the table's all-zero row (K-tiles padded past a split's end read it)
  int tm_begin = 0, tm_count = 0;    // restrict the launch to M tiles [tm_begin, tm_begin + tm_count) (0 = all): the
                                     // data-parallel overlap all-reduces one row block of dW while the next is computed
  int abl = 0;                       // as FwdArgs::abl
  int fuse_upd = 0;                  // 1: S == 1 and the epilogue applies `upd` instead of storing the tile to the slab
  WgradUpd upd;
  // Split-K partial products as f16 (round 6, option "slab16"; k_wgrad_gemm_ph only): the slab buffer holds [S][Dp][Fp] HALVES, every
  // (split, 256 x 256 tile) carries one power-of-two factor -- the tile's largest magnitude placed in [2^14, 2^15): no overflow whatever the
  // gradient scale, 11 significant bits per partial product -- whose inverse goes to slab_sc[split * tiles + tm * tilesN + tn]
  int slab16 = 0;
  float* slab_sc = nullptr;
  // the LEAN instantiations of k_wgrad_gemm_ph (round 6, option "wgrad_lean"): gathered rows addressed as table + 32-bit byte offset --
  // set by pass.hip (vv_backward_plan.h) when every row of the table (scratch rows included) lies below 4 GiB and its index below 2^24
  int lean = 0;
};

struct ReduceArgs {
  const float* slabs; int S, Dp, Fp;
  int slab16 = 0; const float* slab_sc = nullptr;   // WgradArgs::slab16: f16 partial products and their per-(split, tile) factors
  const float* dbp; int B;
  int db_rows = 0;         // rows of dbp (0 = B, one per item; the segment-wise backward writes SEGB_BLOCKS partials)
  const Scales* scales;
  float sg;
  const GradGuard* gg = nullptr;   // f16: the step's final scale is sg * gg->mul
  const float* sg_dev = nullptr;   // per-layer operator: the scale chosen on the device (overrides sg)
  // the loss workgroup also reports the step's max |dY| (unscaled) and final shift to the host: ring of 16 entries
  const float* gmax_slots = nullptr; int gmax_n0 = 0, gmax_n1 = 0, gmax_stride = 0;
  unsigned long long* gmax_host = nullptr; int32_t seq = 0;
  int guard_last_round = 0;        // the step's final guard round (its flag must not be up)
  const uint32_t* h16_cnt = nullptr; int h16_cnt_n = 0;   // SegBwdArgs::h16_cnt and its pairs: folded into words 2 and 3 of the report entry (null: zeros)
  const unsigned long long* gbound = nullptr; const int32_t* gcnt = nullptr;   // proactive path: GuardArgs::bound / cnt_max (reported too)
  float* grads;            // [D*F + D]
  int D, F;
  float ip_scale;          // 1 + regularization/2 (inner_product_layer.cpp:80-90), normally 1
  // the loss reduction rides in one extra workgroup: loss = loss_scale * sum(loss_part), violations = sum(viol_part)
  const float* loss_part; const float* viol_part; float loss_scale; float* loss_out;
  int d_begin = 0, d_count = 0;      // rows of dW this launch reduces (d_count 0 = all D)
  int f_begin = 0, f_count = 0;      // columns of dW this launch reduces (f_count 0 = all F); multiples of 4
  int n_chunks = 0;                  // > 0: dW is stored CHUNK-MAJOR -- n_chunks column blocks, block c = all D rows of columns
  int chunk_c0[5] = {0, 0, 0, 0, 0}; //   [chunk_c0[c], chunk_c0[c+1]) at float offset D chunk_c0[c], row stride = the block's width
                                     //   (boundaries multiples of 4) -- so that every F-chunk is one contiguous all-reduce buffer
  int shard_rows = 0;                // > 0: the gradient buffer is SHARD-MAJOR (the sharded update, solver.hip): D / shard_rows shards, shard s =
                                     //   rows [s shard_rows, (s + 1) shard_rows) of dW (row-major) followed by their shard_rows entries of db --
                                     //   one reduce-scatter message per rank, and k_sgd sees its shard as a small [dW | db] buffer of its own
  int parts = 3;                     // bit 0: the dW rows, bit 1: db and the loss scalars
  Scales* scale_sc = nullptr;        // non-null: one more workgroup performs the W -> half scale update left pending by the
  const float* scale_wmax = nullptr; //   previous step's k_sgd (its per-block max |w| slots,
  int scale_n = 0;                   //   this many of them)
  int scale_prec = 0;
};

struct SgdArgs {
  float* W; float* b; float* hW; float* hb;
  const float* grads;      // [D*F + D]
  uint16_t* Wh; Scales* scales;
  float* wmax_blocks;      // [SGD_BLOCKS] per-block max |w| of this update
  int D, F, Dp, Fp;
  SolverRule rule;
  // one F-chunk of the update (data-parallel overlap): columns [f_begin, f_begin + f_count) of every row, read from the
  // chunk-major gradient buffer (ReduceArgs::n_chunks; f_count may be 0: nothing but, possibly, the bias);
  // chunked = 0: the whole matrix from the row-major buffer
  int chunked = 0, f_begin = 0, f_count = 0;
  int blk_off = 0, n_blk = 0;   // slots of wmax_blocks this launch writes = its grid (the chunks of an update share SGD_BLOCKS)
  int do_bias = 1;         // this launch also updates b (the last chunk: db is all-reduced with it)
  int set_scale = 1;       // this launch publishes the scale of the new half copy (the first chunk)
  // Publication from inside the kernel (chunked launches of the overlapped update; null = none): what the NEXT forward
  // GEMM reads while this very stream is still working -- the half copy, its scale, the bias -- is stored write-through
  // at agent scope (sc1); every wave drains its stores, the workgroup meets at a barrier and adds itself to pub_count;
  // the workgroup whose add is the last sets *pub_flag = pub_seq (and clears the counter for the next chunk).  The
  // consumer polls the flag and runs an agent-scope acquire (FwdArgs::gate).  No separate launch, no L2 write-back.
  int32_t* pub_flag = nullptr; int32_t* pub_count = nullptr; int32_t pub_seq = 0;
  // data-parallel, direct peer transport: != 0 once an exchange in front of this launch gave up (a rank is missing) -- the gradient is
  // not the sum over the ranks; the launch changes nothing (and publishes nothing: the failure is fatal for the context, comm.hip)
  const uint32_t* skip_if = nullptr;
};

// Reduction and update in one launch (k_reduce_sgd; pass.hip: the lazy reduction).  r: what k_reduce would have been given (its
// scale_* fields unused), g: what k_sgd would have been given.  Every workgroup that updates parameters derives the scale of
// the new half copy for itself from the previous update's per-block maxima (wmax_prev: what k_scale_update folds) when
// recompute_scale is set, else takes Scales::sw_next as it stands; this update's maxima go to g.wmax_blocks (another buffer).
struct FusedUpdArgs {
  ReduceArgs r; SgdArgs g;
  int no_params = 0;         // 1: only the special workgroups (bias, loss, the guard's report): the parameter matrix was updated in the
                             //    weight-gradient GEMM's epilogue (WgradUpd)
  const float* wmax_prev = nullptr; int wmax_prev_n = 0; int recompute_scale = 0; int prec = 0;
  int store_grads = 0;       // also write dW to the gradient buffer (0: it stays in the slabs, pass.hip materialises it on request)
};
// The two-history forms (Adam): the second history of W and b rides in an argument struct of its own, so that the one-history kernels
// carry no extra pointer.  v of the same shapes and at the same offsets as hW / hb.
struct SgdArgs2 : SgdArgs { float* vW = nullptr; float* vb = nullptr; };
struct FusedUpdArgs2 : FusedUpdArgs { float* vW = nullptr; float* vb = nullptr; };
constexpr int WMAX_SLOTS = 2048;      // slots of one per-block-maxima buffer (k_sgd writes SGD_BLOCKS of them, k_reduce_sgd RED_DW_BLOCKS)

// Gradient clipping by the global L2 norm (BVLC Caffe's SGDSolver::ClipGradients; vv_clip_gradients_set): k_grad_sumsq leaves this
// record, k_grad_scale and vv_clip_stats read it.  sumsq: the sum of g^2 over the flat buffer [dW | db] in double; norm = sqrt(sumsq)
// and scale = clip / norm are formed in double and rounded once each; clipped = norm (the fp32 value, as BVLC compares) > clip, else
// scale is 1 and k_grad_scale writes nothing.  updates / clipped_updates: counted by the kernel itself, so nothing synchronises per step.
struct ClipRec {
  double sumsq; float norm; float scale; int32_t clipped; int32_t pad_;
  int64_t updates, clipped_updates;
};
constexpr int CLIP_BLOCKS = 256;      // k_grad_sumsq's fixed grid = the per-block partial sums its last stage adds in index order
struct ClipArgs {
  float* g; int64_t n;                // the flat gradient buffer
  float clip;
  ClipRec* rec; double* part;         // [CLIP_BLOCKS]
  uint32_t* arrived;                  // arrival counter of k_grad_sumsq's workgroups (0 between launches)
  const uint32_t* skip_if = nullptr;  // as SgdArgs::skip_if: a failed exchange in front, the launch changes nothing
};

// Gradient accumulation (BVLC Caffe's SolverParameter.iter_size: Solver::Step's accumulating ForwardBackward passes and
// SGDSolver::Normalize; vv_grads_bank): the cycle's loss and violation sums and what vv_accum_stats reports, kept by k_grad_bank's
// first thread -- nothing synchronises per pass.
struct AccumRec {
  float loss_sum, viol_sum;           // of the gradients banked in this cycle, fp32, in banking order
  float last_mean_loss, last_mean_viol; int32_t last_count; int32_t pad_;      // of the last completed accumulated update
  int64_t updates;
};
constexpr int BANK_BLOCKS = 1024;     // k_grad_bank's fixed grid: 262 144 threads, one 16-byte item each per pass
// dst[i] = src[i] (Store: the first bank of a cycle, and the bank into the gradient buffer in front of an exchange or of clipping),
// dst[i] = dst[i] + src[i] (Add: every later bank), dst[i] = src[i] * inv (Scale: SGDSolver::Normalize, src == dst allowed)
enum class BankOp : int { Store = 0, Add = 1, Scale = 2 };
struct BankArgs {
  const float* src; float* dst; int64_t n;
  float inv = 1.f;                    // Scale: 1.0f / (float)m
  // the loss: fold = 1 folds loss2 = {loss, violations} of the last forward pass into rec's sums (Store stores, Add adds); fold = 2 closes
  // the cycle (means = sums * inv, last_count = m, updates += 1); 0: the record is not touched
  int fold = 0; int32_t m = 0;
  const float* loss2 = nullptr; AccumRec* rec = nullptr;
  const uint32_t* skip_if = nullptr;  // as SgdArgs::skip_if: a failed exchange in front, the launch changes nothing
};

// The exponential moving average of the parameters (vv_ema_set; this project's own: neither the reference tree nor BVLC Caffe has
// one).  k_ema: e[i] = decay * e[i] + om * w[i] over two streams, the matrix (nW = D F elements) and the bias (nb = D) -- two fp32
// products and one fp32 sum per element, each rounded as written (no contraction).  om = 1.0f - decay, formed by the host.  All four
// bases are on 16-byte boundaries (allocation starts; eb sits behind eW on the next one).
constexpr int EMA_BLOCKS = 1024;      // k_ema's fixed grid: 262 144 threads, one 16-byte item (vec) or one element each per pass
struct EmaArgs {
  const float* W; const float* b;     // the fp32 master parameters, read after the update in front
  float* eW; float* eb;               // the average
  int64_t nW; int32_t nb;
  float decay, om;
  const uint32_t* skip_if = nullptr;  // as SgdArgs::skip_if: a failed exchange in front, the launch changes nothing
};

// Magnitude statistics (the reference's debug_info: Net::ForwardDebugInfo / BackwardDebugInfo / UpdateDebugInfo, net.cpp:580-636, over
// Blob::asum_data / asum_diff, blob.cpp:138-165; vv_op_asum, vv_debug_stats_queue): k_abs_stats measures up to STAT_SEGS buffers in one
// launch and leaves one record per buffer -- the layout of include/videovec.h's vv_abs_stat.  asum: the sum of |x| over the FINITE
// elements in double, in a fixed order; amax: the largest finite |x|; nonfinite: NaN and +-Inf elements, which count in neither.
struct AbsRec { double asum; float amax; int32_t reserved_; int64_t count, nonfinite; };
constexpr int STAT_BLOCKS = 256;      // k_abs_stats' fixed grid = the per-workgroup partials its last stage folds in index order
constexpr int STAT_SEGS = 8;          // buffers per launch
enum : int { STAT_F32 = 0, STAT_F16 = 1, STAT_BF16 = 2 };
// One buffer: n elements of `type` at p.  q (fp32 only): a second buffer of the same length -- the element is p[i] - q[i], one fp32 subtract.
struct AbsSeg { const void* p; const void* q; int64_t n; int type; int slot; };      // slot: the record it fills
struct AbsStatsArgs {
  AbsSeg seg[STAT_SEGS]; int nseg;
  AbsRec* rec;                        // the records (indexed by AbsSeg::slot)
  double* part_sum; float* part_max; unsigned long long* part_nf;      // [STAT_SEGS][STAT_BLOCKS] each: the workgroups' partials
  uint32_t* arrived;                  // arrival counter of the workgroups (0 between launches)
};

// Which kernels a context runs (vv_ctx::ko).  The launchers read the options of the context whose entry point is running on this
// thread (g_ko, set by every ABI entry point next to hipSetDevice); nothing here is process-global, so two contexts of one process
// do not inherit each other's choices.  Product options are set by vv_set_option (their environment variables are read ONCE per
// context, in vv_create); the fields marked (lab) select ablated / experimental kernels whose results may be WRONG: they are
// settable only in a build with -DVV_LAB (make lab -> lib/libvideovec_lab.so, what tools/lab/* use), and the ablated
// instantiations are compiled only there.
struct KernelOpts {
  int fwd_lead = 1;        // "fwd_lead" / VV_FWD_LEAD: the forward GEMM's sibling lead (kernels_gemm_ph.hip)
  int wgrad_tr = 1;        // "wgrad_tr" / VV_WGRAD_TR: transposed LDS reads in the weight-gradient GEMM (0: the round-1 kernel)
  int score_pf = 1;        // "score_pf" / VV_SCORE_PF=0: k_score_fwd's first-round workgroups prefetch the second round's rows into L2 (ScoreArgs::prefetch; 23.4 -> 22.8 us)
  int wgrad_lean = 1;      // "wgrad_lean" / VV_WGRAD_LEAN=0: k_wgrad_gemm_ph's lean instantiations (fewer instructions in the LOAD segments: scalar bases + 32-bit lane offsets, LDS addresses as immediates, a K loop without end-of-stream tests); only for tables below 4 GiB
  int ablate = 0;          // (lab) VV_ABLATE: ablated instantiations of the dense-size GEMMs (results wrong)
  int lab_fwd_abl = 0;     // (lab) VV_LAB_FWD_ABL: ablations of the 192-row forward kernel at the de-duplicated size (results wrong)
  int lab_wg_abl = 0;      // (lab) VV_LAB_WG_ABL
  int ph_mq = 0;           // (lab) VV_PH_MQ: force the forward tile (2, 3, 4 = 128 / 192 / 256 rows)
  int score_reg = 1;       // (lab) VV_SCORE_REG=0: the LDS-resident score kernel
  int score_rr = 0;        // (lab) VV_SCORE_RR=1: the item-major kernels deal their items round-robin over the XCDs again (kernels_score.hip: item_of_block)
  // What the launchers last chose for this context (read-only through vv_get_option: "last_fwd_tile_rows", "last_wgrad_splits",
  // "last_update_form", "last_score_form"): written where the kernel is launched (launch_fwd_ph_q / launch_wgrad_gemm / launch_sgd /
  // launch_reduce_sgd / launch_score_fwd / launch_score_loss), so a test
  // can assert the form it ran without a copy of the pickers' rules.
  mutable int last_fwd_tile_rows = 0;   // rows of the forward GEMM's tile (128, 192, 256); 0: no launch yet
  mutable int last_wgrad_splits = 0;    // S (splits of K) of the weight-gradient GEMM; 0: no launch yet
  mutable int last_update_form = 0;     // what last updated the parameter matrix: 1 k_sgd 16-byte (chunked / sharded launches too), 2 k_sgd scalar,
                                        // 3 k_reduce_sgd, 4 k_reduce_sgd over f16 slabs, 5 the weight-gradient GEMM's epilogue; 0: no update yet
  mutable int last_score_form = 0;      // what last computed scores and loss: 1 k_score_fwd, 2 k_score_stream at D = 512, 3 k_score_stream at D = 1024,
                                        // 4 the per-instance kernels (launch_score_loss); 0: no forward pass yet
};
extern thread_local const KernelOpts* g_ko;
inline const KernelOpts& ko() { static const KernelOpts dflt; return g_ko ? *g_ko : dflt; }

// Kernel timing without extra queue packets: when the ABI layer has armed a pair of events (vv_profile_enable),
// the launch goes through hipExtLaunchKernelGGL, which stamps the events from the dispatch packet's own
// start / completion signal.  (A hipEventRecord pair around every kernel costs ~3 us of queue time per record on
// this runtime -- 50 us per step over the seven timed kernels -- and would distort the very step being measured.)
struct ProfPair { hipEvent_t start = nullptr, stop = nullptr; };
extern thread_local ProfPair g_prof;
#define VV_LAUNCH_EV(kern, grid, block, lds, s, use_start, use_stop, ...)                                   \
  do {                                                                                                     \
    hipEvent_t e0_ = (use_start) ? vv::g_prof.start : nullptr, e1_ = (use_stop) ? vv::g_prof.stop : nullptr; \
    if (e0_ || e1_) {                                                                                      \
      hipExtLaunchKernelGGL(kern, grid, block, lds, s, e0_, e1_, 0, __VA_ARGS__);                           \
      if (use_start) vv::g_prof.start = nullptr;                                                           \
      if (use_stop) vv::g_prof.stop = nullptr;                                                             \
    } else hipLaunchKernelGGL(kern, grid, block, lds, s, __VA_ARGS__);                                      \
  } while (0)
#define VV_LAUNCH(kern, grid, block, lds, s, ...) VV_LAUNCH_EV(kern, grid, block, lds, s, true, true, __VA_ARGS__)
#define VV_LAUNCH_FIRST(kern, grid, block, lds, s, ...) VV_LAUNCH_EV(kern, grid, block, lds, s, true, false, __VA_ARGS__)
#define VV_LAUNCH_LAST(kern, grid, block, lds, s, ...) VV_LAUNCH_EV(kern, grid, block, lds, s, false, true, __VA_ARGS__)
// ... of a kernel with dynamic LDS: the opt-in to more than the default 64 KB, then the launch
#define VV_LAUNCH_LDS(kern, grid, block, lds, s, ...)                                                       \
  do {                                                                                                     \
    (void)hipFuncSetAttribute((const void*)(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)); \
    VV_LAUNCH(kern, grid, block, lds, s, __VA_ARGS__);                                                     \
  } while (0)

// Launch dispatch: run-time flags and the precision become compile-time arguments of a generic lambda, so that a launcher names each
// kernel template once instead of once per combination.  with_flags(f, b1, b2, ...) calls f(std::bool_constant<b1>{}, ...);
// with_prec(prec, f) calls f(TypeTag<F16>{}) or f(TypeTag<BF16>{}).  Every path through the lambda's body is instantiated for EVERY
// combination of its arguments: a combination that has no kernel on purpose is kept out of the lambda by a run-time branch in front of
// it, or inside it by an `if constexpr` that leaves it an empty body (the set of kernels in the library does not grow).
template <typename T> struct TypeTag { using type = T; };
struct F16; struct BF16;
template <typename F> inline void with_flags(F&& f) { f(); }
template <typename F, typename... B> inline void with_flags(F&& f, bool b, B... rest) {
  if (b) with_flags([&](auto... t) { f(std::true_type{}, t...); }, rest...);
  else with_flags([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}
template <typename F> inline void with_prec(int prec, F&& f) { if (prec == 0) f(TypeTag<F16>{}); else f(TypeTag<BF16>{}); }

// kernel launchers (defined in the .hip files); prec: 0 = f16, 1 = bf16
void launch_fwd_gemm(int prec, const FwdArgs& a, hipStream_t s);
bool fwd_gemm_can_gate(const FwdArgs& a);                     // the forward kernel has a gated form for these arguments (FwdArgs::gate)
long fwd_gemm_plan(int R, int R_hint, int D, int* mq_out);   // workgroups of the default forward GEMM that get a tile
void launch_wgrad_gemm(int prec, const WgradArgs& a, hipStream_t s);
bool wgrad_can_fuse_update();
void launch_score_loss(int prec, const ScoreArgs& a, hipStream_t s);
void launch_dedup(const DedupArgs& a, hipStream_t s);
void launch_dedup_groups(const DedupArgs& a, hipStream_t s);
void launch_dedup_pos(const DedupArgs& a, hipStream_t s);   // pos[] for the debug accessors only
void launch_segsum(int prec, const SegsumArgs& a, hipStream_t s);
void launch_score_fwd(const ScoreArgs& a, hipStream_t s);   // forward + factored backward records (dedup mode)
void launch_seg_bwd(int prec, const SegBwdArgs& a, hipStream_t s);
// (h16: src holds f16 rows -- FwdArgs::h16; map == nullptr: row r is its own source)
void launch_gather_rows_dropout(const float* src, const int32_t* map, int R, int D, const DropSpec& dr, float* dst, hipStream_t s, int h16 = 0);
void launch_gather_rows_f32(const float* src, const int32_t* map, int R, int D, float* dst, hipStream_t s, int h16 = 0);
void launch_gather_rows_u16(const uint16_t* src, const int32_t* pos, int R, int Dp, uint16_t* dst, hipStream_t s);
void launch_reduce(const ReduceArgs& a, hipStream_t s);
// (vW / vb: the second history, rule.solver_type == 5 only -- the two-history instantiations)
void launch_sgd(int prec, const SgdArgs& a, hipStream_t s, float* vW = nullptr, float* vb = nullptr);
void launch_grad_sumsq(const ClipArgs& a, hipStream_t s);            // -> ClipArgs::rec (no host synchronisation)
void launch_grad_scale(const ClipArgs& a, hipStream_t s);            // g *= rec->scale where rec->clipped, else every workgroup returns at once
void launch_grad_bank(BankOp op, const BankArgs& a, hipStream_t s);   // k_grad_bank: one owner per element, no atomics
void launch_abs_stats(const AbsStatsArgs& a, hipStream_t s);          // k_abs_stats: reads its buffers, writes its partials and records only
void launch_ema(const EmaArgs& a, bool vec, hipStream_t s);           // k_ema: vec -- 16-byte items (nW % 4 == 0), else one element per thread and pass
void launch_publish(int32_t* flag, int32_t seq, hipStream_t s);
void launch_delay(int us, hipStream_t s);                             // test hook: occupies s for `us` microseconds       // flag <- seq (agent scope), behind everything queued on s
void launch_scale_update(int prec, Scales* sc, const float* wmax_blocks, int n_blocks, hipStream_t s);
int launch_reduce_sgd(const FusedUpdArgs& a, hipStream_t s, float* vW = nullptr, float* vb = nullptr);   // -> the number of per-block maxima it writes
void launch_table_convert(int prec, const float* src, uint16_t* dst, int64_t n_rows, int F, int Fp,
                          float sx, hipStream_t s);
void launch_table_synth(int prec, uint16_t* dst, uint64_t seed, int64_t n_rows, int F, int Fp,
                        float sx, hipStream_t s);
void launch_table_read(int prec, const uint16_t* table, const int32_t* rows, int64_t n, int F,
                       int Fp, float inv_sx, float* out, hipStream_t s);
void launch_w_convert(int prec, const float* W, uint16_t* Wh, int D, int F, int Dp, int Fp,
                      Scales* sc, hipStream_t s);
void launch_map_rows(const int32_t* idx, int32_t* rows, int R, int Rp, int32_t zero_row, int32_t row_limit,
                     hipStream_t s);
void launch_final_loss(const float* loss_part, const float* viol_part, int B, float scale,
                       float* out2, hipStream_t s);
// vv_forward's loss reduction: the fold of k_reduce's loss workgroup (same order, same bits) into rec->last_*, and the record's sums
void launch_eval_loss(const float* loss_part, const float* viol_part, int B, float scale, int64_t terms, EvalRec* rec, hipStream_t s);
void launch_dyh_to_float(int prec, const uint16_t* dYh, int R, int D, int Dp, float inv_sg,
                         float* out, hipStream_t s);
void launch_row_normalize(float* x, int n, int D, hipStream_t s);
void launch_absmax(const float* x, int64_t n, unsigned* out_bits, hipStream_t s);
void launch_mean_rows(int prec, uint16_t* table, const int32_t* rows, int64_t n, int k, const float* coeff,
                      int64_t first_row, int Fp, hipStream_t s);
void launch_gram(const float* x, int n, int dim, float alpha, float* out, hipStream_t s);
void launch_patch_rows(uint16_t* table, const int32_t* desc, int64_t n_patch, int64_t first_row, int F,
                       int Fp, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Gallery retrieval (kernels_retrieval.hip): fp32 similarity of one query block into a scratch buffer, then row kernels.
// ---------------------------------------------------------------------------------------------
constexpr int RT_BM = 128, RT_BN = 128;               // similarity tile (its K, RT_BK, and RT_CHUNK / RT_MAX_K / RT_SEL_*: vv_gallery_plan.h)
struct RankAcc { double ap_sum; int32_t best, acc1, acc5, acc10; };   // ComputeApStats' running values of one query
static_assert(sizeof(RankAcc) == GALLERY_ACC_BYTES, "vv_gallery_plan.h sizes the per-query accumulator");
void launch_sim_f32(const float* Q, const float* G, float* out, int nq, int ng, int Dp, int64_t pitch, hipStream_t s);
// query row i = Q + rowidx[i] * Dp (rowidx: device [nq], checked on the host); otherwise launch_sim_f32, bit for bit
void launch_sim_f32_rows(const float* Q, const int32_t* rowidx, const float* G, float* out, int nq, int ng, int Dp, int64_t pitch, hipStream_t s);
// seg: gallery items per workgroup (a multiple of 1024), S = ceil(ng / seg); part: uint64 [rows][S][k]
void launch_topk(const float* dist, int64_t pitch, int rows, int ng, int k, int seg, int S, uint64_t* part, int32_t* idx,
                 float* dst, hipStream_t s);
// bins: uint32 [rows][2][RT_CHUNK], zero on entry
void launch_rank_pass(const float* dist, int64_t pitch, int rows, int ng, int seg, int S, const int32_t* pos_idx,
                      const int32_t* pstart, const int32_t* pcount, const int32_t* q_ids, const int32_t* ref_ids, int pass,
                      uint32_t* bins, RankAcc* acc, hipStream_t s);
// Class-level statistics (RetrievalStatsLayer): the rows of a block are the gallery items q0 .. q0 + rows - 1.
struct ClassAcc { double ap_sum; int32_t npos, acc1, n5, pad_; };      // ComputeStats' running values of one query
static_assert(sizeof(ClassAcc) == GALLERY_ACC_BYTES, "the two statistics share the per-query accumulator buffer");
// as launch_topk, over the items whose id differs from the row's own
void launch_topk_other_id(const float* dist, int64_t pitch, int rows, int ng, int k, int seg, int S, const int32_t* ids, int q0,
                          uint64_t* part, int32_t* idx, float* dst, hipStream_t s);
// Nearest-neighbour lists (vv_gallery_nearest*).  Eligible for row r: every item; own != NULL: those whose id (ids[]) differs from
// own[r]; self0 >= 0: the rows are gallery items self0 .., item self0 + r is not eligible for row r.
// Streaming form, k <= RT_MAX_K: launch_topk with that predicate.
void launch_topk_eligible(const float* dist, int64_t pitch, int rows, int ng, int k, int seg, int S, const int32_t* ids,
                          const int32_t* own, int self0, uint64_t* part, int32_t* idx, float* dst, hipStream_t s);
// Selection form, k <= RT_CHUNK.  st: uint32 [rows][4] and hist: uint32 [rows][RT_SEL_BINS], both zero on entry;
// segh: uint32 [rows][S][RT_SEL_LAST_BINS]; cand: uint64 [rows][RT_CHUNK]; idx / dst: [rows][k]
void launch_select(const float* dist, int64_t pitch, int rows, int ng, int k, int seg, int S, const int32_t* ids,
                   const int32_t* own, int self0, uint32_t* st, uint32_t* hist, uint32_t* segh, uint64_t* cand, int32_t* idx,
                   float* dst, hipStream_t s);
// k-NN vote (vv_gallery_knn_scores*) over the lists either form above left on the device: idx / dist with `stride` entries between
// two rows; labels: int32 [ng] in [0, C), C <= 4096; out: row r at out + r * C; m_out: int32 [rows], the filled slots of every row.
// exp_weights: VV_KNN_EXP with temperature T, else VV_KNN_UNIFORM (dist and T unread).  Returns the store form: 1 16-byte, 2 element-wise.
int launch_knn_vote(const int32_t* idx, const float* dist, int64_t stride, int rows, int k, int exp_weights, float T,
                    const int32_t* labels, int C, float* out, int32_t* m_out, hipStream_t s);
// cpos: item indices grouped by class; ids / cls: id and class of every item; skeys: uint64 [rows][RT_CHUNK];
// bins: uint32 [rows][3][RT_CHUNK], zero on entry
void launch_class_pass(const float* dist, int64_t pitch, int rows, int ng, int seg, int S, const int32_t* cpos,
                       const int32_t* pstart, const int32_t* pcount, const int32_t* ids, const int32_t* cls, int q0, int exclude,
                       int pass, uint64_t* skeys, uint32_t* bins, ClassAcc* acc, hipStream_t s);
// ustart: int32 [n_ids + 1], the groups of pos_idx; out: [n_ids][Dp]
void launch_pool_by_id(const float* feat, int Dp, const int32_t* pos_idx, const int32_t* ustart, int n_ids, float* out,
                       hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Classification statistics (kernels_classify.hip): ClassificationStatsLayer, one column block of the score matrix at a time.
// ---------------------------------------------------------------------------------------------
constexpr int CLS_TILE = 256;                         // positives of one class per counting workgroup, one per thread
constexpr int CLS_STAGE = 1024;                       // keys of the class's column staged in LDS at a time (4 per thread)
// src: the block's first column of row 0, pitch floats between rows; columns c0 .. c0 + cb - 1; last: the matrix's last block
void launch_cls_rows(const float* src, int64_t pitch, int n, int c0, int cb, int last, const int32_t* labels, float* rmax,
                     int32_t* rarg, uint32_t* correct, unsigned long long* nan_count, hipStream_t s);
// col: [cb][npitch], npitch a multiple of 64
void launch_cls_pack(const float* src, int64_t pitch, int n, int cb, float* col, int64_t npitch, hipStream_t s);
// seg: items per workgroup (a multiple of CLS_STAGE), S = ceil(n / seg); labels: [npitch]; tiles[t] = {first position in pos_idx,
// positives (<= CLS_TILE), class, 0}, the class's keys in column class - c0 of col; cnt: uint32 [n][3] by position in pos_idx, zero on entry
void launch_cls_count(const float* col, int64_t npitch, int n, int seg, int S, int c0, const int32_t* labels, const int32_t* pos_idx,
                      const int4* tiles, int tile0, int ntiles, uint32_t* cnt, hipStream_t s);
// cstart: int32 [C + 1], the groups of pos_idx by class; apd / ap: [C]
void launch_cls_final(const float* col, int64_t npitch, int c0, int cb, const int32_t* pos_idx, const int32_t* cstart,
                      const uint32_t* cnt, double* apd, float* ap, hipStream_t s);
// out [rows][ng] = -0.5f * dist [rows][pitch]
void launch_scores_out(const float* dist, int64_t pitch, int rows, int ng, float* out, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Softmax linear classifier on gallery embeddings (kernels_linear.hip, linear.hip)
// ---------------------------------------------------------------------------------------------
constexpr int LIN_BM = 128, LIN_BN = 128, LIN_BK = 32;   // the weight-gradient product's output tile and K step
constexpr int LIN_TARGET_BLOCKS = 512;                  // workgroups the split plan aims at (a constant, not the device's CU count)
constexpr int LIN_MIN_SPLIT_ROWS = 128;                 // rows of one split at least, in the library's plan (four K steps)
constexpr int LIN_MAX_SPLITS = 128;                     // slabs at most; a batch of more rows than 128 splits runs in row blocks
constexpr int LIN_SM_BLOCKS = 512;                      // k_softmax_xent's fixed grid = the partials its last stage adds in index order
constexpr int LIN_UPD_BLOCKS = 1024;                    // k_lin_update's fixed grid
struct LinRec { double loss_sum; int64_t correct, nonfinite; };   // one batch: sum of the rows' loss terms, rows won by the label, rows with a non-finite logit
struct LinSoftmaxArgs {
  const float* sim; int64_t pitch; int64_t rows; int cols;        // z = mul sim + bias: mul -0.5f on what k_sim_f32 stored, 1 on logits
  float mul;
  const float* bias;                                              // [cols] or NULL
  const int32_t* labels;                                          // device [rows]
  float scale;                                                    // loss_weight / (float)count of the whole batch
  float* dz; float* prob;                                         // [rows][pitch] each, either may be NULL
  float* row_loss; int32_t* row_flags;                            // [rows] (both or neither): the row's term; bit 0 correct, bit 1 non-finite
  int wd;                                                         // lanes per row: 32 (cols <= 32) or 64
  LinRec* rec; int first_block;                                   // first_block: rec is stored, else added to
  double* part_loss; uint32_t* part_cnt; uint32_t* arrived;       // [LIN_SM_BLOCKS], [LIN_SM_BLOCKS][2], the arrival counter (0 between launches)
};
struct LinWgradArgs {
  const float* A; int64_t lda; const float* B; int64_t ldb;       // A [k][m], B [k][n]
  int64_t k; int m, n;
  int64_t split_rows; int S;                                      // split s: rows [s split_rows, (s + 1) split_rows) of k
  float* slabs; int64_t slab_stride;                              // [S][m][n], slab_stride floats apart
  float* dbs;                                                     // [S][m] column sums of A, or NULL
  int accumulate; int vec_a, vec_b;                               // vec_*: base and leading dimension on 16 bytes
  const int32_t* rowidx = nullptr;                                // NULL, or device [k]: row kk of B is B + rowidx[kk] * ldb (checked on the host)
};
struct LinPlan { int64_t split_rows = 0, block_rows = 0; int S = 0, blocks = 0; };    // S: splits of the first (largest) row block
LinPlan lin_plan(int64_t k, int m, int n, int64_t forced_split_rows);
struct LinUpdArgs {
  const float* slabs; int64_t slab_stride; int S; int64_t nW;     // nW = m n elements
  const float* dbs; int64_t db_stride; int nb;                    // nb: bias elements (0: none)
  float *W, *hW, *b, *hb;                                         // rule == 0: W / b are the outputs, hW / hb unused
  float lr, momentum, wd; int rule; int vec;
};
// k_hinge: the one-vs-rest hinge loss (hinge_loss_layer.cpp:13-77) on the same logits, the same record and the same partial buffers
struct LinHingeArgs {
  const float* sim; int64_t pitch; int64_t rows; int cols;        // z = mul sim + bias, as LinSoftmaxArgs
  float mul;
  const float* bias;                                              // [cols] or NULL
  const int32_t* labels;                                          // device [rows]
  int norm;                                                       // 1: L1, 2: L2 (VV_NORM_*)
  float scale;                                                    // L1: loss_weight / (float)count; L2: (loss_weight * 2.0f) / (float)count
  float* dz;                                                      // [rows][pitch] or NULL; columns cols .. pitch - 1 are written zero
  int wd;                                                         // lanes per row: lin_hinge_lanes(cols)
  int vec;                                                        // 1: sim and dz on 16 bytes and pitch % 4 == 0 (float4 accesses); 0: element-wise
  LinRec* rec; int first_block;
  double* part_loss; uint32_t* part_cnt; uint32_t* arrived;       // k_softmax_xent's buffers
};
// lanes per row: the power of two that covers ceil(cols / 4) float4 chunks, 1 .. 64
inline int lin_hinge_lanes(int cols) { int wd = 1; while (wd < 64 && wd * 4 < cols) wd <<= 1; return wd; }
void launch_softmax_xent(const LinSoftmaxArgs& a, hipStream_t s);
void launch_hinge(const LinHingeArgs& a, hipStream_t s);
void launch_lin_scores_out(const float* sim, int64_t pitch, int64_t rows, int cols, const float* bias, float* out, hipStream_t s);
void launch_lin_wgrad(const LinWgradArgs& a, hipStream_t s);
void launch_lin_update(const LinUpdArgs& a, hipStream_t s);
// api.hip: a gallery's device rows ([n_ref][Dp] fp32, columns dim .. Dp - 1 zero) and the context it belongs to
struct GalleryRows { const float* feat; int64_t n_ref; int dim, Dp; const void* ctx; };
GalleryRows gallery_rows(const ::vv_gallery* g);

// ---------------------------------------------------------------------------------------------
// k-means on a gallery (kernels_kmeans.hip, kmeans.hip); the sizes are vv_kmeans_plan.h's
// ---------------------------------------------------------------------------------------------
struct KmRec { double objective; long long moved, nonfinite; int32_t empty, degenerate, chunks, pad_; };   // one pass and the update behind it
static_assert(sizeof(KmRec) == KM_REC_BYTES, "vv_kmeans_plan.h sizes the record");
void launch_km_gather(const float* feat, int Dp, const int32_t* rows, int C, float* cent, hipStream_t s);
// score: rows [row0, row0 + rows) against the C centroids, C floats apart; row0 a multiple of KM_SLOT_ROWS.  -> the form: 1 16-byte, 2 element-wise
int launch_km_assign(const float* score, int C, int64_t row0, int rows, int euclid, const float* nn, int32_t* assign, int32_t* counts,
                     double* slot, KmRec* rec, hipStream_t s);
void launch_km_fold(const double* slot, int64_t slots, KmRec* rec, hipStream_t s);
// hist: int32 [tiles][C]; start, cbase: int32 [C + 1]; chunks: int4 [max_chunks]; nchunks: int32 [1]; list: int32 [n]
void launch_km_group(const int32_t* assign, int64_t n, int C, int64_t tiles, const int32_t* counts, int32_t* hist, int32_t* start,
                     int32_t* cbase, int4* chunks, int64_t max_chunks, int32_t* nchunks, int32_t* list, KmRec* rec, hipStream_t s);
void launch_km_partial(const float* feat, int64_t n, int Dp, const int32_t* list, const int4* chunks, const int32_t* nchunks, int64_t max_chunks,
                       int slices, float* part, hipStream_t s);
// init: cent holds the initial centroids, only nn is written
void launch_km_finish(const float* part, int Dp, int dim, const int32_t* counts, const int32_t* cbase, int64_t max_chunks, int C, int euclid, int init,
                      float* cent, float* nn, KmRec* rec, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Inverted-file search (kernels_ivf.hip, ivf.hip); the sizes are vv_ivf_plan.h's
// ---------------------------------------------------------------------------------------------
static_assert(IVF_TILE == RT_BM && IVF_TILE == RT_BN, "vv_ivf_plan.h counts the similarity kernel's tiles");
struct IvfRec { long long tiles, candidates; };         // one call: the tiles its blocks listed, the sum of its queries' candidate counts
static_assert(sizeof(IvfRec) == IVF_REC_BYTES, "vv_ivf_plan.h sizes the record");
// One block's (query, cluster) pairs: pair i * nprobe + p is query row i's p-th probed cluster.  Every array is the library's own.
struct IvfBlock {
  const float* Q;                  // [rows][Dp] the query block, zero padded
  const float* slab;               // [n_ref][Dp] the index's cluster-contiguous rows
  const int32_t* start;            // [C + 1] cluster c's rows are slab rows start[c] .. start[c + 1] - 1
  const int32_t* list;             // [n_ref] slab row -> item index
  const int32_t* probe;            // [pairs] the pair's cluster
  const int32_t* off;              // [pairs] where the cluster's candidates begin in the query's candidate row
  const int32_t* qstart;           // [C + 1] the pairs grouped by cluster: cluster c's are qlist[qstart[c] .. qstart[c + 1])
  const int32_t* qlist;            // [pairs] pair indices, by cluster, ascending inside one
  const int4* tiles;               // [tile_cap] {cluster, query tile, item tile, 0}
  const int32_t* ntiles;           // [1]
  float* cand;                     // [rows][pitch]
  int64_t pitch;
  int rows, Dp, C, nprobe, tile_cap;
};
// score: [rows][C] what launch_sim_f32 stored for the block against the centroids; nn: [C] (euclid) or unread; counts: [C], zero on
// entry -- the pairs of every cluster; m: [rows] candidate counts.  all: nprobe == C, every cluster in ascending order, nothing selected
void launch_ivf_probe(const float* score, int rows, int C, int nprobe, int all, int euclid, const float* nn, const int32_t* start,
                      int32_t* probe, int32_t* off, int32_t* m, int32_t* counts, IvfRec* rec, hipStream_t s);
void launch_ivf_tiles(const int32_t* start, const int32_t* qstart, int C, int4* tiles, int tile_cap, int32_t* ntiles, IvfRec* rec, hipStream_t s);
void launch_sim_f32_grouped(const IvfBlock& b, int grid_wgs, hipStream_t s);
// idx / dist: [rows][k], slots past m[row] read -1 / 0
void launch_ivf_select(const IvfBlock& b, int k, int32_t* idx, float* dist, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Product-quantised lists (kernels_pq.hip, pq.hip); the sizes are vv_pq_plan.h's
// ---------------------------------------------------------------------------------------------
// out [n][Dps] = columns col0 .. col0 + dsub - 1 of feat [n][Dp], columns dsub .. Dps - 1 zero
void launch_pq_slice(const float* feat, int64_t n, int Dp, int col0, int dsub, int Dps, float* out, hipStream_t s);
// codes [n][M] (item order): byte m of item g = assign[g] cut into 0 .. ksub - 1
void launch_pq_pack(const int32_t* assign, int64_t n, int m, int M, int ksub, uint8_t* codes, hipStream_t s);
// slab [n][Mrow]: row p = the codes of item list[p]
void launch_pq_permute(const uint8_t* codes, const int32_t* list, int64_t n, int M, int Mrow, uint8_t* slab, hipStream_t s);
// lut [rows][table]: entry m * ksub + j of row i = -2.0f * s + 0.0f, s the serial chain of Q[i][m dsub + col] * cb[m][j][col]; Q: [rows][Dp]
void launch_pq_lut(const float* Q, int rows, int Dp, const float* cb, int M, int ksub, int dsub, float* lut, int64_t table, hipStream_t s);
struct PqScan {
  const float* lut; int64_t table;       // [rows][table]
  const uint8_t* slab; int Mrow;         // [n_ref][Mrow] codes in list-position order, every byte < ksub
  const int32_t *start, *probe, *off;    // as IvfBlock's
  float* cand; int64_t pitch;            // [rows][pitch]
  int rows, nprobe, M, ksub;
};
// the form pq_scan_form(M) names; the launch asks for table * 4 bytes of LDS (<= PQ_LDS_BYTES)
void launch_pq_scan(const PqScan& a, int form, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// 16-bit operand types
// ---------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));

struct F16 {
  static constexpr int id = 0;
  static __device__ __forceinline__ f32x4 mfma(i16x8 a, i16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a),
                                                  __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint16_t from_float(float x) {
    x = fminf(fmaxf(x, -65504.f), 65504.f);   // saturate instead of producing inf
    return __builtin_bit_cast(uint16_t, (_Float16)x);
  }
  static __device__ __forceinline__ float to_float(uint16_t v) {
    return (float)__builtin_bit_cast(_Float16, v);
  }
};

struct BF16 {
  static constexpr int id = 1;
  static __device__ __forceinline__ f32x4 mfma(i16x8 a, i16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                   __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint16_t from_float(float x) {
    return __builtin_bit_cast(uint16_t, (__bf16)x);
  }
  static __device__ __forceinline__ float to_float(uint16_t v) {
    return __builtin_bit_cast(float, (uint32_t)v << 16);
  }
};

#ifdef __HIPCC__
// ---- f16 gradient-scale guard, device side (GradGuard above).  Every thread of the block calls these.
// max over the block, valid in every thread; smem: >= 16 floats of LDS not otherwise in use around the call
__device__ __forceinline__ float gg_block_max(float v, float* smem) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = 0.f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) m = fmaxf(m, smem[w]);
  return m;
}
// Start of a producer launch.  false: a repeat whose previous round raised no flag -- nothing to do, the caller returns
// (all threads alike).  sg_mul: the power of two to put on top of the host's scale in this round.
__device__ __forceinline__ bool gg_begin(const GuardArgs& g, float* smem, float& sg_mul) {
  sg_mul = 1.f;
  if (!g.gg || g.round == 0) return true;
  const int prev = g.round > 1 ? g.gg->shift[g.round - 1] : 0;
  int shift = prev;
  const bool active = g.gg->flag[g.round - 1] == g.seq;
  if (active) {
    float m = 0.f;
    const float* sl = g.slots + (size_t)(g.round - 1) * 2 * g.nslot;
    for (int p = 0; p < 2; ++p)
      for (int i = threadIdx.x; i < g.n_of[p]; i += blockDim.x) m = fmaxf(m, sl[(size_t)p * g.nslot + i]);
    m = gg_block_max(m, smem);
    int e = 0;
    (void)frexpf(m, &e);                       // m = f 2^e, f in [0.5, 1): afterwards the largest value lies in [2^11, 2^12)
    shift = prev + (e - 12 > 1 ? e - 12 : 1);
    __syncthreads();                           // smem may be reused by the caller
  }
  if (g.last && blockIdx.x == 0 && threadIdx.x == 0) {
    if (active) g.gg->repeat_seq = g.seq;
    g.gg->shift[g.round] = shift;
    if (g.final_round) { g.gg->mul = ldexpf(1.f, -shift); g.gg->shift[3] = shift; }     // [3]: the step's final shift
  }
  sg_mul = ldexpf(1.f, -shift);
  return active;
}
// End of a producer launch: block_max = this block's max |g| in the round's scaled units, before rounding (thread 0's
// value is used).
__device__ __forceinline__ void gg_end(const GuardArgs& g, float block_max) {
  if (!g.gg || threadIdx.x != 0) return;
  g.slots[((size_t)g.round * 2 + g.producer) * g.nslot + blockIdx.x] = block_max;
  if (block_max > GG_LIMIT) __hip_atomic_store(&g.gg->flag[g.round], g.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the parameter update, device side: what k_sgd, k_reduce_sgd and the weight-gradient GEMM's UPD epilogue share besides
// SolverRule::step.  NW: the waves of the workgroup (4 or 8); red: NW floats of LDS the caller owns; wave: this thread's wave index.
// The scale of a 16-bit copy whose largest magnitude is m: f16 places m in [2^11, 2^12), bf16 needs none
__device__ __forceinline__ float half_scale(float m, int prec) {
  float s = 1.f;
  if (prec == 0 && m > 0.f && isfinite(m)) {
    int e;
    (void)frexpf(m, &e);           // m = f 2^e, f in [0.5, 1)
    s = ldexpf(1.f, 12 - e);
  }
  return s;
}
// every wave's max of v into red[wave], then a barrier
__device__ __forceinline__ void waves_max_to_lds(float v, float* red, int wave) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
}
// the max of red[0 .. NW) (pairwise for four waves, in order for eight: the orders the kernels were tuned with)
template <int NW>
__device__ __forceinline__ float lds_max(const float* red) {
  if constexpr (NW == 4) return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float m = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) m = fmaxf(m, red[w]);
  return m;
}
// The scale of the new half copy, recomputed (FusedUpdArgs::recompute_scale) from the previous update's n per-block maxima and
// vv_params_set's seed in Scales::wmax_bits (the host clears the seed behind the launch).  Every thread gets it; red is free again
// only after a barrier.
template <int NW>
__device__ __forceinline__ float fold_scale(const float* wmax_prev, int n, const Scales* sc, int prec, float* red, int wave) {
  float mm = 0.f;
  for (int k = threadIdx.x; k < n; k += NW * 64) mm = fmaxf(mm, wmax_prev[k]);
  waves_max_to_lds(mm, red, wave);
  mm = lds_max<NW>(red);
  return half_scale(fmaxf(mm, __uint_as_float(sc->wmax_bits)), prec);
}
// The end of an update: this workgroup's max |w| to its slot; workgroup 0 (first) records the scale sw its half copy carries,
// and, when it recomputed that scale, the scale the next update will use
template <int NW>
__device__ __forceinline__ void update_end(float wmax, float* red, int wave, float* slot, bool first, Scales* sc, float sw, int recompute_scale) {
  waves_max_to_lds(wmax, red, wave);
  if (threadIdx.x == 0) {
    *slot = lds_max<NW>(red);
    if (first) { sc->sw_cur = sw; if (recompute_scale) sc->sw_next = sw; }
  }
}
// dW = (the 16-bit operands' product) times this: ip_scale / (sg' sx), sg' the scale the gradients really carry -- chosen on the
// device (sg_dev), else the host's sg times the guard's final multiplier
__device__ __forceinline__ float grad_unscale(float ip_scale, float sg, const GradGuard* gg, const float* sg_dev, const Scales* sc) {
  const float sgf = sg_dev ? *sg_dev : (gg ? sg * gg->mul : sg);
  return ip_scale / (sgf * sc->sx);
}
// four elements of W times sw as four halves of the 16-bit copy
template <typename T>
__device__ __forceinline__ uint2 pack_half4(float x, float y, float z, float w, float sw) {
  return make_uint2(T::from_float(x * sw) | ((uint32_t)T::from_float(y * sw) << 16), T::from_float(z * sw) | ((uint32_t)T::from_float(w * sw) << 16));
}
#endif

// splitmix64 finaliser, identical to videovector_amd/synth.py:mix64
__host__ __device__ inline uint64_t mix64(uint64_t seed, uint64_t x) {
  uint64_t z = seed * 0x9E3779B97F4A7C15ull + x;
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace vv
