// gallery_plan_check.cc -- prints the sizes of videovector_amd/csrc/vv_gallery_plan.h for every edge shape, query count and flag pair, one
// line per case; tests/test_gallery_plan_host.py compares each line with its own statement of the arithmetic.
//   make -C videovector_amd/csrc gallery_plan_check && videovector_amd/csrc/build/gallery_plan_check
#include <cstdio>

#include "../videovector_amd/csrc/vv_gallery_plan.h"

using namespace vv;

int main() {
  // where behaviour can change: the 64-float pitch; seg leaving its floor of 16384 (64 * 16384 items); the largest pitch that still
  // allows GALLERY_QB_MAX rows under GALLERY_DIST_MAX and the first that does not; a gallery of which not one row fits
  static const long long kRef[] = {1, 63, 64, 65, 16384, 16385, 1048576, 1048577, 503808, 503809, 1ll << 30};
  static const int kDim[] = {1, 32, 33, 512, 8192}, kQ[] = {1, 511, 512, 513};
  long cases = 0;
  for (long long n_ref : kRef)
    for (int dim : kDim)
      for (int n_q : kQ)
        for (int flags = 0; flags < 4; ++flags) {
          const bool cls = flags & 1, sel = flags & 2;
          const GalleryShape s = gallery_shape(n_ref, dim);
          printf("n_ref=%lld dim=%d n_q=%d cls=%d sel=%d -> Dp=%d pitch=%lld seg=%d S=%d qb_max=%d row_bytes=%zu block_rows=%d\n", n_ref, dim,
                 n_q, cls, sel, s.Dp, (long long)s.pitch, s.seg, s.S, s.qb_max, gallery_row_bytes(s, cls, sel),
                 gallery_block_rows(s, n_q, cls, sel));
          ++cases;
        }
  fprintf(stderr, "gallery_plan_check: %ld cases\n", cases);
  return 0;
}
