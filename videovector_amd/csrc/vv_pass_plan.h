// vv_pass_plan.h -- which execution a pass over one batch takes: de-duplicated or dense, where dropout rides, the segment-wise pair or
// per-instance gradient rows, f16 or fp32 rows of ip2.  The training pass (fb_impl) and the forward-only pass (vv_forward) ask this ONE
// function, so the two cannot choose differently for the same cfg; the blob accessors and the last_* options rely on that.  A pure function
// of the values below: no allocation, no context pointer.  No HIP header: a host compiler builds this alone (tools/pass_plan_check.cc).
#pragma once

namespace vv {

// The segment-wise pair: k_seg_bwd holds a row of D = 512 or 1024 columns; the forward is the register-resident k_score_fwd where an item
// fits (D = 512, up to 56 target / negative rows, 6 context rows), else the streaming kernel
inline bool score_fwd_supported(int D) { return D == 512 || D == 1024; }
// ... with dropout (ScoreArgs::drop), by the value of option "drop_dedup": every kernel of the pair carries the per-instance masks (k_score_fwd,
// k_score_stream and k_seg_bwd, D = 512 and 1024); value 1, the default, keeps dropout steps de-duplicated on the shapes of the register-resident
// kernel only, value 2 on every shape of the pair, value 0 on none.  The DROP forms read fp32 per-item vectors: dropout steps run with v16 off.
inline bool score_fwd_dropout_supported(int drop_dedup, int D, int C, int Nn) {
  if (drop_dedup == 1) return D == 512 && C - 1 <= 6 && 1 + Nn <= 56;
  return drop_dedup == 2 && score_fwd_supported(D);
}

// what the choice depends on, and nothing else
struct PassPlanIn {
  bool dedup = false, seg_bwd = false;      // options "dedup" (vv_set_dedup), "seg_bwd"
  int drop_dedup = 0;                       // option "drop_dedup": 0, 1, 2
  bool h16 = false, h16_fallback = false;   // option "h16", and whether "h16_guard" 2 has switched the context to fp32 rows
  bool v16 = false;                         // option "v16"
  bool ablate = false;                      // timing studies (VV_ABLATE): dense, fp32 rows
  int D = 0, C = 0, Nn = 0;
  bool dropout = false;                     // cfg.dropout_ratio > 0
  bool fwd_only = false;                    // vv_forward
};

struct PassPlan {
  bool drop_on = false;
  bool dd = false;              // the batch rows are de-duplicated (one projection per distinct row)
  bool drop_rides_dd = false;   // dd && drop_on: H holds the shared pre-dropout rows, every instance masks its row as it reads it
  bool seg = false;             // the segment-wise pair (k_score_fwd / k_score_stream + k_seg_bwd)
  bool h16 = false;             // the forward GEMM stores ip2 as f16 rows
  bool v16 = false;             // the per-item vectors leave the score kernel as f16
};

inline PassPlan pass_plan(const PassPlanIn& in) {
  PassPlan p;
  // De-duplicate the batch rows.  Dropout sits BEHIND the projection (fc7 -> ReLU -> drop2, mednet_embedding_train.prototxt:190-230): the
  // projection of equal rows is equal, only the mask differs per instance.  The segment-wise pair carries the masks (k_score_fwd /
  // k_score_stream + k_seg_bwd at D = 512 and 1024: every instance masks its row as it reads it, the backward sums m_i-weighted terms per
  // distinct row), and option "drop_dedup" says on which of its shapes dropout rides the de-duplicated path: 1, the default, the shapes of
  // the register-resident k_score_fwd; 2 every shape of the pair; 0 none.  Elsewhere it stays dense (the mask in the forward GEMM's
  // epilogue).  The two executions evaluate the same mask function (vv_internal.h: DropSpec).
  p.drop_on = in.dropout;
  const bool drop_dd = p.drop_on && in.drop_dedup && in.seg_bwd && score_fwd_dropout_supported(in.drop_dedup, in.D, in.C, in.Nn);
  p.dd = in.dedup && (!p.drop_on || drop_dd) && !in.ablate;
  p.drop_rides_dd = p.dd && p.drop_on;
  // de-duplicated batches of the supported shape: the backward stays factored per instance and is summed per distinct
  // row (k_score_fwd + k_seg_bwd); otherwise per-instance 16-bit gradient rows (+ k_segsum when de-duplicated)
  p.seg = p.dd && in.seg_bwd && score_fwd_supported(in.D);
  // ip2 as f16 (option "h16"): only where the segment-wise pair reads it -- de-duplicated batches of D = 512 / 1024 (k_score_fwd / k_score_stream /
  // k_seg_bwd carry the f16 row loads; the dense and the generic kernels keep fp32 rows), D % 8 == 0, the phase-staggered forward kernel
  p.h16 = in.h16 && !in.h16_fallback && p.seg && !in.ablate;
  // the per-item vectors as f16: the one-sweep kernel's D = 1024 form only (840 k gathers of a 4 KB row per step at configs[4]'s per-GPU shape;
  // at D = 512 the 2 MB matrix lives in L2 and 16-bit vectors measured net zero, profiles/r04_h16_intermediate.txt).  The forward-only
  // instantiations write no per-item vectors.
  p.v16 = p.h16 && in.v16 && in.D == 1024 && !p.drop_on && !in.fwd_only;
  return p;
}

}  // namespace vv
