// pass_plan_check.cc -- prints the plan of videovector_amd/csrc/vv_pass_plan.h for every combination of the options, dropout, forward-only,
// ablation and the edge shapes, one line per case; tests/test_pass_plan_host.py compares each line with its own statement of the rules.
//   make -C videovector_amd/csrc pass_plan_check && videovector_amd/csrc/build/pass_plan_check
#include <cstdio>

#include "../videovector_amd/csrc/vv_pass_plan.h"

using namespace vv;

int main() {
  static const int kD[] = {256, 512, 1024}, kC[] = {2, 7, 8}, kNn[] = {1, 55, 56};     // C - 1 <= 6 and 1 + Nn <= 56: the register-resident kernel's limits
  long cases = 0;
  for (int bits = 0; bits < 256; ++bits)
    for (int drop_dedup = 0; drop_dedup <= 2; ++drop_dedup)
      for (int D : kD) for (int C : kC) for (int Nn : kNn) {
        PassPlanIn in;
        in.dedup = bits & 1; in.seg_bwd = bits & 2; in.h16 = bits & 4; in.h16_fallback = bits & 8; in.v16 = bits & 16;
        in.ablate = bits & 32; in.dropout = bits & 64; in.fwd_only = bits & 128;
        in.drop_dedup = drop_dedup; in.D = D; in.C = C; in.Nn = Nn;
        const PassPlan p = pass_plan(in);
        printf("dedup=%d seg_bwd=%d drop_dedup=%d h16=%d h16_fallback=%d v16=%d ablate=%d D=%d C=%d Nn=%d dropout=%d fwd_only=%d -> "
               "drop_on=%d dd=%d drop_rides_dd=%d seg=%d h16=%d v16=%d\n",
               in.dedup, in.seg_bwd, in.drop_dedup, in.h16, in.h16_fallback, in.v16, in.ablate, in.D, in.C, in.Nn, in.dropout, in.fwd_only,
               p.drop_on, p.dd, p.drop_rides_dd, p.seg, p.h16, p.v16);
        ++cases;
      }
  fprintf(stderr, "pass_plan_check: %ld cases\n", cases);
  return 0;
}
