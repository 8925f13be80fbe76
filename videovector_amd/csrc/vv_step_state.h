// vv_step_state.h -- where this step's gradient is, and whether an overlapped parameter update has been joined: the two pieces of
// bookkeeping between vv_forward_backward* and vv_apply_update (pass.hip, api.hip, solver.hip, ops.hip).  Each is ONE value that only the transitions below
// write, and every transition sets the whole of it.  No HIP header: a host compiler builds this alone (tools/step_state_check.cc).
#pragma once
#include <cstring>

namespace vv {

// Where the gradient of the last backward pass is.  Exactly one holds.
enum class GradAt {
  None,           // no forward/backward pass since vv_create, vv_params_set or a change of the batch shape
  Slabs,          // lazy reduction: dW is in the split-K slabs (db / the loss in their partials), the reduction is due -- vv_ctx::red_args.
                  // vv_apply_update reduces and updates in ONE launch (k_reduce_sgd); whoever reads the gradient or the loss first runs
                  // the plain k_reduce (reduce_now)
  SlabsWUpdated,  // ... and the weight-gradient GEMM's epilogue has already updated W (vv_update_hint, one split of K;
                  // vv_ctx::upd_wgrad_blocks): the parameters are half-way, only vv_apply_update and vv_loss_get may come next
  SlabsStale,     // the fused update ran without writing dW to the gradient buffer: it is still in the slabs, untouched since
  Lost,           // vv_apply_update finished a SlabsWUpdated step: its dW was consumed in registers and never stored (vv_grads_*
                  // refuse until the next backward pass; vv_loss_get still answers)
  Buffer          // in the gradient buffer (vv_ctx::grads), laid out as GradBuffer says
};

// How the gradient buffer is laid out: flat [dW | db], chunk-major (ReduceArgs::n_chunks: the overlapped schedule) or shard-major
// (ReduceArgs::shard_rows: the sharded schedule)
enum class GradLayout { Flat, Chunked, Sharded };

// Meaningful in GradAt::Buffer only; every other place holds the default.
struct GradBuffer {
  GradLayout layout = GradLayout::Flat;
  bool summed = true;            // false: the sum over the ranks of a communicator is still due
  bool chunk0_event = false;     // the first F-chunk's reduction was recorded on an event of its own (vv_ctx::ev_chunk0)
};

struct GradState {
  GradAt at = GradAt::None;
  GradBuffer buf;
};

// An overlapped update: joined; in flight on the communication stream, the compute stream has not joined it; or consumed chunk by
// chunk by a gated forward GEMM, the compute stream has still not waited for its END (its plain stores -- W, the history)
enum class UpdSync { Joined, InFlight, Gated };

// ---- the gradient's transitions
// a backward pass left its gradient in the slabs (w_updated: the weight-gradient GEMM applied the update to W as well)
inline void grad_to_slabs(GradState& g, bool w_updated) { g = {w_updated ? GradAt::SlabsWUpdated : GradAt::Slabs, {}}; }
// a backward pass (the fused step's or the per-layer operator's) wrote its gradient into the buffer
inline void grad_to_buffer(GradState& g, GradLayout layout, bool summed, bool chunk0_event) { g = {GradAt::Buffer, {layout, summed, chunk0_event}}; }
// the plain k_reduce ran for a reader: lazily kept gradients only exist without a communicator, so flat and summed
inline void grad_reduced(GradState& g) { if (g.at == GradAt::Slabs || g.at == GradAt::SlabsStale) g = {GradAt::Buffer, {}}; }
// the sum over the ranks is in the buffer (or on its way there, queued in front of every reader)
inline void grad_summed(GradState& g) { if (g.at == GradAt::Buffer) g.buf = {g.buf.layout, true, false}; }
// vv_apply_update queued its update
inline void grad_update_consumed(GradState& g) {
  if (g.at == GradAt::Slabs) g = {GradAt::SlabsStale, {}};
  else if (g.at == GradAt::SlabsWUpdated) g = {GradAt::Lost, {}};
  else grad_summed(g);
}
// vv_params_set, or the batch buffers (the slabs among them) were freed: the gradient goes with what it belonged to
inline void grad_discard(GradState& g) { g = {}; }
// the communicator is gone: nothing is due, and the buffer is read as flat from here on
inline void grad_comm_destroyed(GradState& g) { if (g.at == GradAt::Buffer) g.buf = {}; }

inline bool grad_exists(const GradState& g) { return g.at != GradAt::None; }
inline bool grad_sum_due(const GradState& g) { return g.at == GradAt::Buffer && !g.buf.summed; }

// What the entry point `who` is told (vv_loss_get never asks).  A gradient that was never stored is refused to those that want the gradient
// itself: vv_grads_*, and a second vv_apply_update on the same step.
enum class GradRefusal { No, NeverStored, UpdateFirst };
inline GradRefusal grad_guard(const GradState& g, const char* who) {
  const bool update = !strcmp(who, "vv_apply_update");
  switch (g.at) {
    case GradAt::SlabsWUpdated: return update ? GradRefusal::No : GradRefusal::UpdateFirst;
    case GradAt::Lost: return update || !strncmp(who, "vv_grads", 8) ? GradRefusal::NeverStored : GradRefusal::No;
    default: return GradRefusal::No;
  }
}

// ---- the overlapped update's transitions
inline void upd_queued(UpdSync& u) { u = UpdSync::InFlight; }
inline void upd_gated(UpdSync& u) { if (u == UpdSync::InFlight) u = UpdSync::Gated; }
inline void upd_joined(UpdSync& u) { u = UpdSync::Joined; }

}  // namespace vv
