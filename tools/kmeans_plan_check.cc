// kmeans_plan_check.cc -- prints the plan of videovector_amd/csrc/vv_kmeans_plan.h for every edge shape, cluster count and forced block, one
// line per case; tests/test_kmeans_host.py compares each line with its own statement of the arithmetic.
//   make -C videovector_amd/csrc kmeans_plan_check && videovector_amd/csrc/build/kmeans_plan_check
#include <cstdio>

#include "../videovector_amd/csrc/vv_kmeans_plan.h"

using namespace vv;

int main() {
  // where behaviour can change: the 64-row slot, the 256-entry chunk, the 1024-item tile; a forced block that is no multiple of 64 or
  // exceeds n; shapes whose fixed buffers leave less than the 64 MiB target (7 000 000 x 8192 in 1024 clusters) or nothing of the
  // scratch limit; a cluster count past the limit
  static const long long kN[] = {1, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 70001, 200000, 1000000, 7000000, 16777216, 1ll << 28, 1ll << 30};
  static const int kDim[] = {1, 32, 33, 512, 8192}, kC[] = {1, 3, 64, 1024, 4096, 4097};
  static const long long kForce[] = {0, 1, 64, 100, 4096, 1ll << 26};
  long cases = 0;
  for (long long n : kN)
    for (int dim : kDim)
      for (int C : kC)
        for (long long f : kForce) {
          const KmeansPlan p = kmeans_plan(n, dim, C, f);
          printf("n=%lld dim=%d C=%d force=%lld -> ok=%d Dp=%d block_rows=%lld blocks=%lld tiles=%lld slots=%lld max_chunks=%lld slices=%d "
                 "score=%zu item=%zu partial=%zu total=%zu\n", n, dim, C, f, p.ok, p.Dp, (long long)p.block_rows, (long long)p.blocks,
                 (long long)p.tiles, (long long)p.slots, (long long)p.max_chunks, p.slices, p.score_bytes, p.item_bytes, p.partial_bytes,
                 p.total_bytes);
          ++cases;
        }
  fprintf(stderr, "kmeans_plan_check: %ld cases\n", cases);
  return 0;
}
