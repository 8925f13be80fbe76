// pq_plan_check.cc -- prints the limits and the plan of videovector_amd/csrc/vv_pq_plan.h for every edge of M, ksub, dim, probe count,
// candidate pitch and forced block rows, one line per case; tests/test_pq_host.py compares each line with its own statement of the
// arithmetic.
//   make -C videovector_amd/csrc pq_plan_check && videovector_amd/csrc/build/pq_plan_check
#include <cstdio>

#include "../videovector_amd/csrc/vv_pq_plan.h"

using namespace vv;

int main() {
  // where behaviour can change: M at 0, 1, the three code-row forms (3, 4, 16), 64 and 65; ksub at 1, 2, 255, 256 and 257 -- M = 64 with
  // ksub = 256 is the LDS limit itself; a dim M does not divide; nprobe at and past 64, equal to C and past it; a pitch of nothing and of
  // the whole gallery; a forced block below, at and past n_q; a gallery of which one query's row leaves nothing of the scratch limit
  static const int kM[] = {0, 1, 3, 4, 16, 64, 65}, kKsub[] = {1, 2, 16, 255, 256, 257}, kDim[] = {48, 192, 512, 50};
  static const long long kN[] = {300, 1000000, 1ll << 28};
  static const int kC[] = {1, 8, 65, 4096}, kProbe[] = {1, 8, 64, 65, 4096};
  static const long long kNq[] = {1, 70, 4096, 1ll << 22};
  static const long long kForce[] = {0, 1, 64, 1ll << 20};
  long cases = 0;
  for (int M : kM)
    for (int ksub : kKsub)
      for (int dim : kDim) {
        printf("shape dim=%d M=%d ksub=%d -> error=%d form=%d row=%d table=%lld\n", dim, M, ksub, pq_shape_error(dim, M, ksub),
               M > 0 ? pq_scan_form(M) : 0, M > 0 ? pq_code_row_bytes(M) : 0, (long long)(M > 0 && ksub > 0 ? pq_table_floats(M, ksub) : 0));
        for (long long n : kN)
          for (int C : kC)
            for (int np : kProbe)
              for (long long nq : kNq)
                for (long long f : kForce) {
                  const long long items = cases % 2 ? n : 0;
                  const PqPlan p = pq_plan(n, dim, C, np, nq, items, M, ksub, f);
                  printf("n=%lld dim=%d C=%d nprobe=%d nq=%lld items=%lld M=%d ksub=%d force=%lld -> ok=%d Dp=%d dsub=%d form=%d table=%lld pitch=%lld "
                         "block_rows=%lld blocks=%lld pairs=%lld total=%zu\n", n, dim, C, np, nq, items, M, ksub, f, p.ok, p.Dp, p.dsub, p.form,
                         (long long)p.table, (long long)p.pitch, (long long)p.block_rows, (long long)p.blocks, (long long)p.pairs, p.total_bytes);
                  ++cases;
                }
      }
  fprintf(stderr, "pq_plan_check: %ld cases\n", cases);
  return 0;
}
