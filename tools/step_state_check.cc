// step_state_check.cc -- walks every (state, transition) pair of videovector_amd/csrc/vv_step_state.h on the host and checks the WHOLE
// resulting state against the rules written out here, and the guard's answers against the booleans it was derived from.
//   make -C videovector_amd/csrc step_state_check && videovector_amd/csrc/build/step_state_check
#include <cstdio>
#include <vector>

#include "../videovector_amd/csrc/vv_step_state.h"

using namespace vv;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++g_checks;                                            \
    if (!(cond)) {                                         \
      ++g_failed;                                          \
      fprintf(stderr, "FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
    }                                                      \
  } while (0)

static const GradAt kAt[] = {GradAt::None, GradAt::Slabs, GradAt::SlabsWUpdated, GradAt::SlabsStale, GradAt::Lost, GradAt::Buffer};
static const GradLayout kLayout[] = {GradLayout::Flat, GradLayout::Chunked, GradLayout::Sharded};

static bool same(const GradState& a, const GradState& b) {
  return a.at == b.at && a.buf.layout == b.buf.layout && a.buf.summed == b.buf.summed && a.buf.chunk0_event == b.buf.chunk0_event;
}
static GradState mk(GradAt at, GradLayout l = GradLayout::Flat, bool summed = true, bool ev = false) {
  GradState g; g.at = at; g.buf.layout = l; g.buf.summed = summed; g.buf.chunk0_event = ev;       // (the check builds states by hand; the library never does)
  return g;
}
// the invariant: outside the buffer the buffer's record holds its default
static bool well_formed(const GradState& g) { return g.at == GradAt::Buffer || same(g, mk(g.at)); }
static int id(const GradState& g) { return (int)g.at * 100 + (int)g.buf.layout * 10 + (g.buf.summed ? 2 : 0) + (g.buf.chunk0_event ? 1 : 0); }

// every state the transitions can be handed: the five places outside the buffer, and the buffer in each of its 3 x 2 x 2 records
static std::vector<GradState> all_states() {
  std::vector<GradState> v;
  for (GradAt at : kAt) {
    if (at != GradAt::Buffer) { v.push_back(mk(at)); continue; }
    for (GradLayout l : kLayout) for (int s = 0; s < 2; ++s) for (int e = 0; e < 2; ++e) v.push_back(mk(at, l, s != 0, e != 0));
  }
  return v;
}

// The guard as it read before the states existed, on the booleans of each place: grads_lost refused vv_grads_*, upd_in_wgrad refused
// every guarded entry point.
static int old_guard(GradAt at, const char* who) {
  const bool grads_lost = at == GradAt::Lost, upd_in_wgrad = at == GradAt::SlabsWUpdated;
  if (grads_lost && !strncmp(who, "vv_grads", 8)) return 1;
  if (upd_in_wgrad) return 2;
  return 0;
}

int main() {
  const std::vector<GradState> states = all_states();
  CHECK(states.size() == 17, "%zu states", states.size());
  CHECK(same(GradState(), mk(GradAt::None)), "a new context has no gradient");
  for (const GradState& s0 : states) {
    CHECK(well_formed(s0), "state %d", id(s0));
    const bool in_buf = s0.at == GradAt::Buffer;
    GradState g;
    // a backward pass into the slabs: the whole state, whatever came before
    for (int w = 0; w < 2; ++w) {
      g = s0; grad_to_slabs(g, w != 0);
      CHECK(same(g, mk(w ? GradAt::SlabsWUpdated : GradAt::Slabs)), "to_slabs(%d) from %d gave %d", w, id(s0), id(g));
    }
    // a backward pass into the buffer: exactly the record it names (nothing of an earlier layout, sum or event survives)
    for (GradLayout l : kLayout) for (int s = 0; s < 2; ++s) for (int e = 0; e < 2; ++e) {
      g = s0; grad_to_buffer(g, l, s != 0, e != 0);
      CHECK(same(g, mk(GradAt::Buffer, l, s != 0, e != 0)), "to_buffer from %d gave %d", id(s0), id(g));
    }
    // the plain reduction for a reader: what was in the slabs with its reduction due or stale enters the buffer flat, summed, no event;
    // a step whose W is updated stays (only its loss was reduced); everything else had nothing in the slabs
    g = s0; grad_reduced(g);
    if (s0.at == GradAt::Slabs || s0.at == GradAt::SlabsStale) CHECK(same(g, mk(GradAt::Buffer)), "reduced from %d gave %d", id(s0), id(g));
    else CHECK(same(g, s0), "reduced from %d gave %d", id(s0), id(g));
    // summed over the ranks: in the buffer the layout stays, nothing is due, the chunk event is spent
    g = s0; grad_summed(g);
    CHECK(same(g, in_buf ? mk(GradAt::Buffer, s0.buf.layout, true, false) : s0), "summed from %d gave %d", id(s0), id(g));
    // the update consumed the gradient
    g = s0; grad_update_consumed(g);
    GradState want = s0;
    if (s0.at == GradAt::Slabs) want = mk(GradAt::SlabsStale);
    if (s0.at == GradAt::SlabsWUpdated) want = mk(GradAt::Lost);
    if (in_buf) want = mk(GradAt::Buffer, s0.buf.layout, true, false);
    CHECK(same(g, want), "update_consumed from %d gave %d", id(s0), id(g));
    // parameters reset / batch buffers freed
    g = s0; grad_discard(g);
    CHECK(same(g, mk(GradAt::None)), "discard from %d gave %d", id(s0), id(g));
    // communicator destroyed: the place stays, the buffer's record is the default
    g = s0; grad_comm_destroyed(g);
    CHECK(same(g, mk(s0.at)), "comm_destroyed from %d gave %d", id(s0), id(g));
    // no transition leaves a sub-field behind outside the buffer
    for (int t = 0; t < 5; ++t) {
      g = s0;
      if (t == 0) grad_reduced(g); else if (t == 1) grad_summed(g); else if (t == 2) grad_update_consumed(g); else if (t == 3) grad_discard(g); else grad_comm_destroyed(g);
      CHECK(well_formed(g), "transition %d from %d gave %d", t, id(s0), id(g));
    }
    // the predicates
    CHECK(grad_exists(s0) == (s0.at != GradAt::None), "exists at %d", id(s0));
    CHECK(grad_sum_due(s0) == (in_buf && !s0.buf.summed), "sum_due at %d", id(s0));
    // the guard: refuse / allow, and which refusal, as the booleans answered
    static const char* const who[] = {"vv_grads_get", "vv_grads_device", "vv_grads_bind", "vv_forward_backward", "vv_embed", "vv_embed_mean",
                                      "vv_comm_schedule", "vv_comm_init", "vv_allreduce_grads", "vv_params_get", "vv_op_inner_product_bwd"};
    for (const char* w : who) {
      const int old = old_guard(s0.at, w);
      const GradRefusal r = grad_guard(s0, w);
      CHECK((int)r == old && (int)GradRefusal::NeverStored == 1 && (int)GradRefusal::UpdateFirst == 2, "guard(%s) at %d: %d, was %d", w, id(s0), (int)r, old);
    }
    // vv_apply_update itself: due in SlabsWUpdated, refused on a gradient that was never stored (it used to read whatever the buffer held)
    CHECK(grad_guard(s0, "vv_apply_update") == (s0.at == GradAt::Lost ? GradRefusal::NeverStored : GradRefusal::No), "guard(vv_apply_update) at %d", id(s0));
  }
  // the overlapped update: queued -> InFlight from anywhere, gated only moves an update in flight, joined -> Joined from anywhere
  static const UpdSync kSync[] = {UpdSync::Joined, UpdSync::InFlight, UpdSync::Gated};
  for (UpdSync u0 : kSync) {
    UpdSync u = u0; upd_queued(u);
    CHECK(u == UpdSync::InFlight, "queued from %d", (int)u0);
    u = u0; upd_gated(u);
    CHECK(u == (u0 == UpdSync::InFlight ? UpdSync::Gated : u0), "gated from %d", (int)u0);
    u = u0; upd_joined(u);
    CHECK(u == UpdSync::Joined, "joined from %d", (int)u0);
  }
  printf("step_state_check: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
