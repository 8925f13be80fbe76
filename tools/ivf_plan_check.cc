// ivf_plan_check.cc -- prints the plan of videovector_amd/csrc/vv_ivf_plan.h for every edge shape, cluster count, probe count, candidate
// pitch and forced option, one line per case, then ivf_pitch_items on a few lists; tests/test_ivf_host.py compares each line with its
// own statement of the arithmetic.
//   make -C videovector_amd/csrc ivf_plan_check && videovector_amd/csrc/build/ivf_plan_check
#include <cstdio>

#include "../videovector_amd/csrc/vv_ivf_plan.h"

using namespace vv;

int main() {
  // where behaviour can change: the 128-row tile, the 1024-pair grouping tile, the 256-entry chunk; nprobe at and past 64, equal to C
  // and past it; a pitch of nothing, of one list, of the whole gallery; a forced block below, at and past n_q; a forced grid past
  // its limit; shapes of which one query's row leaves nothing of the scratch limit
  static const long long kN[] = {1, 127, 128, 129, 700, 8192, 1000000, 1ll << 28};
  static const int kDim[] = {1, 33, 512}, kC[] = {1, 8, 64, 65, 4096, 4097}, kProbe[] = {1, 7, 64, 65, 4096};
  static const long long kNq[] = {1, 129, 4096, 1ll << 22};
  static const int kPitchShare[] = {0, 1, 128, 0x7fffffff};       // pitch_items = min(n, n * share / 128 rounded up); the last: all of n
  static const long long kForce[] = {0, 1, 64, 1ll << 20};
  static const long long kGrid[] = {0, 3, 70000};
  long cases = 0;
  for (long long n : kN)
    for (int dim : kDim)
      for (int C : kC)
        for (int np : kProbe)
          for (long long nq : kNq)
            for (int share : kPitchShare)
              for (long long f : kForce) {
                const long long g = kGrid[cases % 3];
                long long items = share == 0x7fffffff ? n : (n * share + 127) / 128;
                if (items > n) items = n;
                const IvfPlan p = ivf_plan(n, dim, C, np, nq, items, f, g);
                printf("n=%lld dim=%d C=%d nprobe=%d nq=%lld items=%lld force=%lld grid=%lld -> ok=%d Dp=%d pitch=%lld block_rows=%lld blocks=%lld "
                       "pairs=%lld pair_tiles=%lld max_chunks=%lld tile_cap=%lld grid_wgs=%d total=%zu\n", n, dim, C, np, nq, items, f, g, p.ok,
                       p.Dp, (long long)p.pitch, (long long)p.block_rows, (long long)p.blocks, (long long)p.pairs, (long long)p.pair_tiles,
                       (long long)p.max_chunks, (long long)p.tile_cap, p.grid_wgs, p.total_bytes);
                ++cases;
              }
  // the pitch: the nprobe largest list sizes, whatever their order
  static const int32_t kStart[] = {0, 0, 1, 128, 256, 385, 685, 685, 700};     // sizes 0 1 127 128 129 300 0 15
  for (int np : {1, 2, 7, 8}) printf("pitch_items nprobe=%d -> %lld\n", np, (long long)ivf_pitch_items(kStart, 8, np));
  fprintf(stderr, "ivf_plan_check: %ld cases\n", cases);
  return 0;
}
