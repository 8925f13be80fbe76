// vv_backward_plan.h -- what the backward half of a training pass decides on the host: the split of K of the weight-gradient GEMM, the
// F-chunks of the overlapped update, where the gradient goes and in which layout (which of the five update forms solver.hip then finds),
// the lean instantiation, and the rounds of the f16 gradient-scale guard.  pass.hip fills BackwardPlanIn from the context in ONE place
// (plan_backward) and reads the result; nothing else combines these options.  Pure functions of the values below: no allocation, no
// context pointer.  No HIP header: a host compiler builds this alone (tools/backward_plan_check.cc).
#pragma once

namespace vv {

// the kernels' constants the rules read (vv_internal.h), as plain values
struct BackwardTiles { int BM, BN, BK, WMAX_SLOTS, SGD_BLOCKS, SEGB_BLOCKS; };

// Split-K of the weight-gradient GEMM: S splits of kps K-steps each, so that tiles * S is about one wave of workgroups over the 256 CUs;
// never more splits than K-steps, never fewer than one.
struct SplitK { int S, kps; };
inline SplitK split_k_plan(int Dp, int Fp, int Rp, const BackwardTiles& t) {
  const int tiles = (Dp / t.BM) * (Fp / t.BN), total_steps = Rp / t.BK;
  int S = (256 + tiles - 1) / tiles;
  if (S > total_steps) S = total_steps;
  if (S < 1) S = 1;
  return {S, (total_steps + S - 1) / S};
}

// F-chunks of the overlapped update: n column blocks of W whose widths fall off geometrically (ratio 0.6: e.g. 51 / 31 / 18 %
// of F for three).  The exchange is slower than the forward GEMM consumes W, so the GEMM always ends up waiting for the
// LAST chunk and then still has that chunk's K-tiles to run: a small last chunk shortens that tail, a large first chunk
// keeps the number of collectives (each with its launch latency) down.  Boundaries are even K-tiles (the gate sits in
// front of phase 3 of an even K-tile), at least 4 apart; fills kt[0 .. n] for nk K-tiles, returns n (1 when F is too short).
inline int chunk_plan(int nk, int n_chunks, int* kt) {
  int n = n_chunks < nk / 8 ? n_chunks : nk / 8;
  if (n < 1) n = 1;
  for (;;) {
    double den = 0, r = 1;
    for (int i = 0; i < n; ++i) { den += r; r *= 0.6; }
    kt[0] = 0;
    double acc = 0; r = 1;
    bool ok = true;
    for (int i = 1; i < n; ++i) {
      acc += r; r *= 0.6;
      const int k = (int)(nk * acc / den + 0.5) & ~1;
      if (k < kt[i - 1] + 4 || k > nk - 4) ok = false;
      kt[i] = k;
    }
    kt[n] = nk;
    if (ok || n == 1) return n;
    --n;
  }
}

// what the backward half's choices depend on, and nothing else
struct BackwardPlanIn {
  bool comm = false; int world = 0;                      // a communicator exists, and its ranks
  bool comm_sharded = false, comm_overlap = false;       // vv_comm_schedule 2 / 1
  int D = 0, F = 0, Dp = 0, Fp = 0, Rp = 0, B = 0, S = 1;
  bool grads_own = true, grads_exposed = false;          // the gradient buffer is the library's (no vv_grads_bind) / vv_grads_device handed it out
  bool fuse_update = false, wgrad_update = false, slab16 = false, wgrad_lean = false;      // the options of these names
  bool guard_proactive = true, fuse_keep_grads = false;  // (lab)
  bool can_fuse_update = false;                          // wgrad_can_fuse_update(): the phase-staggered weight-gradient kernel runs
  bool hinted = false, hint_adam = false, hint_clip = false;   // vv_update_hint announced this step; its rule is Adam; clipping was on
  bool f16 = false;                                      // VV_PREC_F16
  bool dd = false, seg = false;                          // the pass plan's (vv_pass_plan.h)
  long long table_rows = 0;                              // every row a K-tile can name: the table, its zero row, the scratch rows behind it
};

struct BackwardPlan {
  int shard_rows = 0;       // D / world
  bool sharded = false;     // k_reduce writes the gradient shard-major (GradLayout::Sharded)
  bool chunked = false;     // ... chunk-major (GradLayout::Chunked)
  bool lazy = false;        // the gradient stays in the slabs (GradAt::Slabs) until somebody wants it
  bool fuse_w = false;      // the weight-gradient GEMM applies the announced update in its epilogue (WgradUpd)
  bool slab16 = false;      // f16 split-K partial products
  bool lean = false;        // WgradArgs::lean
  bool proactive = false;   // GuardArgs::proactive: k_seg_bwd settles the scale before it rounds anything
  int n_rounds = 0;         // conditional repeats of the kernels that round gradients to 16 bits
  int n_of[2] = {0, 0};     // slots the guard's two producers report into
};

inline BackwardPlan backward_plan(const BackwardPlanIn& in, const BackwardTiles& t) {
  BackwardPlan p;
  // Sharded update: shard-major rows, every rank updates D / world whole rows of 16-byte groups, and the per-block maxima of all ranks
  // fit one buffer.  A holder of vv_grads_device's pointer, or a bound buffer, reads the documented flat layout: neither schedule then.
  const bool own_layout = in.comm && in.F % 4 == 0 && in.grads_own && !in.grads_exposed;
  p.shard_rows = in.comm ? in.D / in.world : 0;
  p.sharded = own_layout && in.comm_sharded && p.shard_rows * in.world == in.D && p.shard_rows % 4 == 0 &&
              in.world * (t.SGD_BLOCKS / in.world) <= t.WMAX_SLOTS;
  // Data-parallel overlap: the gradient buffer is laid out chunk-major (a few column blocks, each one contiguous all-reduce message)
  p.chunked = !p.sharded && own_layout && in.comm_overlap;
  // Lazy reduction: with no communicator in the way, dW stays in the slabs -- normally until vv_apply_update, which reduces and updates
  // in one launch (k_reduce_sgd sums at most 8 slabs, 16 bytes at a time).  fuse_update 0: reduce at the end of the pass, as ever.
  p.lazy = in.fuse_update && !in.comm && !in.grads_exposed && in.grads_own && in.F % 4 == 0 && in.S <= 8;
  // vv_update_hint + one split of K: the tile in the weight-gradient GEMM's accumulators IS the gradient -- the solver's rule is applied
  // there.  Adam keeps two histories: the epilogue declines it.  Clipping needs the whole gradient's norm first.  In both cases, as for
  // several splits, the hint changes nothing.
  const int tiles = (in.Dp / t.BM) * (in.Fp / t.BN);
  p.fuse_w = in.hinted && in.wgrad_update && p.lazy && in.S == 1 && in.can_fuse_update && !in.fuse_keep_grads && tiles <= t.WMAX_SLOTS &&
             !in.hint_adam && !in.hint_clip;
  // f16 split-K partial products: the phase-staggered kernel with several splits only (one split: the update rides in the epilogue or
  // the slab is the gradient), at most 8 factors per tile, 16-byte groups of f16
  p.slab16 = in.slab16 && !p.fuse_w && in.S > 1 && in.S <= 8 && in.F % 8 == 0 && in.can_fuse_update;
  // the lean instantiations: row ids below 2^24, a row's bytes below 2^24, the whole table (and one K-tile of slack) below 4 GiB
  p.lean = in.wgrad_lean && in.table_rows < (1ll << 24) && (long long)in.Fp * 2 < (1ll << 24) && in.table_rows * in.Fp * 2 + 8192 < (1ll << 32);
  // The guard's rounds (f16 only).  The segment-wise backward needs no repeat: its score kernel bounds every instance's gradient.
  // Otherwise 1 where one kernel rounds (per-instance rows), 2 for rows + their sums (k_segsum, de-duplicated without the pair).
  p.proactive = in.seg && in.guard_proactive;
  p.n_rounds = !in.f16 ? 0 : (p.proactive ? 0 : (in.dd && !in.seg ? 2 : 1));
  p.n_of[0] = in.seg ? 0 : in.B;
  p.n_of[1] = in.seg ? t.SEGB_BLOCKS : (in.dd ? (in.Rp + 3) / 4 : 0);
  return p;
}

}  // namespace vv
