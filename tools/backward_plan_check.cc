// backward_plan_check.cc -- prints what videovector_amd/csrc/vv_backward_plan.h decides, one line per case in `key=value ... -> key=value ...`
// form; tests/test_backward_plan_host.py compares each line with its own statement of the rules (tests/backward_plan_ref.py).
//   make -C videovector_amd/csrc backward_plan_check && videovector_amd/csrc/build/backward_plan_check
// split_k_plan and chunk_plan: the full product of their value sets.  backward_plan: the full product of ALL its on/off inputs and value
// sets would be 2^17 x 1800 lines, so it is printed in four groups; each keeps the full product of the inputs that appear together in
// the expressions of its outputs and fixes the others (kBase below: f16, de-duplicated, the segment-wise pair, every option at its default,
// no hint, B = 64, Rp = 512, a 2048-row table):
//   dest   sharded, shard_rows, chunked, lazy:  world {0 = none, 1, 2, 3, 8} x comm_sharded x comm_overlap x grads_own x grads_exposed x
//          fuse_update x F x D x S x WMAX_SLOTS {2048, 1023: world * (SGD_BLOCKS / world) lies on both sides of it}
//   fuse   lazy, fuse_w, slab16:  hinted x wgrad_update x can_fuse_update x fuse_keep_grads x hint_adam x hint_clip x slab16 x fuse_update x
//          world {0, 1} x grads_exposed x grads_own x S x F x (D, WMAX_SLOTS) {(256, 2048), (4096, 2048), (4096, 255): 256 tiles on both
//          sides of it}; comm_sharded = comm_overlap = 0
//   lean   lean:  wgrad_lean x table rows on both sides of each limit x Fp {64, 256, 8388352, 8388608}.  Fp = 64 is no table the library
//          builds (rows are padded to 256): with it the row-id limit 2^24 is the one that binds, which at Fp >= 256 the 4-GiB limit hides
//   guard  proactive, n_rounds, n_of:  f16 x dd x seg x guard_proactive x B {64, 65} x Rp {512, 768}
// Every line carries every input and every output, whichever group printed it.
#include <cstdio>
#include <initializer_list>

#include "../videovector_amd/csrc/vv_backward_plan.h"

using namespace vv;

static long cases = 0;

static void show(const char* group, const BackwardPlanIn& in, const BackwardTiles& t) {
  const BackwardPlan p = backward_plan(in, t);
  printf("fn=backward_plan group=%s world=%d comm_sharded=%d comm_overlap=%d D=%d F=%d Dp=%d Fp=%d Rp=%d B=%d S=%d grads_own=%d grads_exposed=%d "
         "fuse_update=%d wgrad_update=%d slab16=%d wgrad_lean=%d guard_proactive=%d fuse_keep_grads=%d can_fuse_update=%d hinted=%d hint_adam=%d "
         "hint_clip=%d f16=%d dd=%d seg=%d table_rows=%lld wmax_slots=%d -> shard_rows=%d sharded=%d chunked=%d lazy=%d fuse_w=%d slab16=%d lean=%d "
         "proactive=%d n_rounds=%d n_of0=%d n_of1=%d\n",
         group, in.comm ? in.world : 0, in.comm_sharded, in.comm_overlap, in.D, in.F, in.Dp, in.Fp, in.Rp, in.B, in.S, in.grads_own, in.grads_exposed,
         in.fuse_update, in.wgrad_update, in.slab16, in.wgrad_lean, in.guard_proactive, in.fuse_keep_grads, in.can_fuse_update, in.hinted, in.hint_adam,
         in.hint_clip, in.f16, in.dd, in.seg, in.table_rows, t.WMAX_SLOTS, p.shard_rows, p.sharded, p.chunked, p.lazy, p.fuse_w, p.slab16, p.lean,
         p.proactive, p.n_rounds, p.n_of[0], p.n_of[1]);
  ++cases;
}

static int pad256(int v) { return (v + 255) / 256 * 256; }

int main() {
  const BackwardTiles kT = {256, 256, 64, 2048, 1024, 1024};       // vv_internal.h: BM, BN, BK, WMAX_SLOTS, SGD_BLOCKS, SEGB_BLOCKS
  static const int kF[] = {252, 254, 256, 260, 4096}, kD[] = {256, 258, 4096}, kS[] = {1, 2, 8, 9}, kWorld[] = {0, 1, 2, 3, 8};
  BackwardPlanIn kBase;
  kBase.D = kBase.F = kBase.Dp = kBase.Fp = 256; kBase.Rp = 512; kBase.B = 64; kBase.S = 8;
  kBase.fuse_update = kBase.wgrad_update = kBase.slab16 = kBase.wgrad_lean = kBase.can_fuse_update = true;
  kBase.f16 = kBase.dd = kBase.seg = true; kBase.table_rows = 2049;
  auto shape = [](BackwardPlanIn& in, int D, int F, int S) { in.D = D; in.F = F; in.Dp = pad256(D); in.Fp = pad256(F); in.S = S; };
  auto comm = [](BackwardPlanIn& in, int world) { in.comm = world > 0; in.world = world; };

  for (int world : kWorld) for (int bits = 0; bits < 32; ++bits) for (int F : kF) for (int D : kD) for (int S : kS) for (int wmax : {2048, 1023}) {
    BackwardPlanIn in = kBase;
    BackwardTiles t = kT; t.WMAX_SLOTS = wmax;
    comm(in, world); shape(in, D, F, S);
    in.comm_sharded = bits & 1; in.comm_overlap = bits & 2; in.grads_own = bits & 4; in.grads_exposed = bits & 8; in.fuse_update = bits & 16;
    show("dest", in, t);
  }
  static const int kTilesD[] = {256, 4096, 4096}, kTilesW[] = {2048, 2048, 255};
  for (int bits = 0; bits < 2048; ++bits) for (int S : kS) for (int F : kF) for (int k = 0; k < 3; ++k) {
    BackwardPlanIn in = kBase;
    BackwardTiles t = kT; t.WMAX_SLOTS = kTilesW[k];
    comm(in, (bits >> 8) & 1); shape(in, kTilesD[k], F, S);
    in.hinted = bits & 1; in.wgrad_update = bits & 2; in.can_fuse_update = bits & 4; in.fuse_keep_grads = bits & 8; in.hint_adam = bits & 16;
    in.hint_clip = bits & 32; in.slab16 = bits & 64; in.fuse_update = bits & 128; in.grads_exposed = bits & 512; in.grads_own = bits & 1024;
    show("fuse", in, t);
  }
  static const long long kRows[] = {255, 256, 257, 8388591, 8388592, 16777215, 16777216};
  for (int lean = 0; lean < 2; ++lean) for (long long rows : kRows) for (int Fp : {64, 256, 8388352, 8388608}) {
    BackwardPlanIn in = kBase;
    in.wgrad_lean = lean; in.table_rows = rows; in.F = in.Fp = Fp;
    show("lean", in, kT);
  }
  for (int bits = 0; bits < 16; ++bits) for (int B : {64, 65}) for (int Rp : {512, 768}) {
    BackwardPlanIn in = kBase;
    in.f16 = bits & 1; in.dd = bits & 2; in.seg = bits & 4; in.guard_proactive = bits & 8; in.B = B; in.Rp = Rp;
    show("guard", in, kT);
  }

  for (int Dp : {256, 512, 4096}) for (int Fp : {256, 512, 4096}) for (int Rp : {256, 512, 768, 8192}) {
    const SplitK k = split_k_plan(Dp, Fp, Rp, kT);
    printf("fn=split_k_plan Dp=%d Fp=%d Rp=%d -> S=%d kps=%d\n", Dp, Fp, Rp, k.S, k.kps);
    ++cases;
  }
  for (int nk : {1, 7, 8, 15, 16, 31, 32, 64, 65}) for (int n_chunks = 1; n_chunks <= 4; ++n_chunks) {
    int kt[5] = {-1, -1, -1, -1, -1};
    const int n = chunk_plan(nk, n_chunks, kt);
    printf("fn=chunk_plan nk=%d n_chunks=%d -> n=%d kt0=%d kt1=%d kt2=%d kt3=%d kt4=%d\n", nk, n_chunks, n, kt[0], kt[1], kt[2], kt[3], kt[4]);
    ++cases;
  }
  fprintf(stderr, "backward_plan_check: %ld cases\n", cases);
  return 0;
}
