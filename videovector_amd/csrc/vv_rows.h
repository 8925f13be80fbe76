// vv_rows.h -- the row lists the linear classifier trains on (vv_linear_fit_rows and its kin, include/videovec.h): shuffled epochs and
// k-fold splits.  Host only: no HIP header, a plain C++ compiler builds it (tools/rows_check.cc checks it alone, under the host
// sanitizers).  linear.hip exports the two functions as vv_rows_shuffled / vv_rows_fold, so that the Python binding and the C++ tool draw
// the same lists.  The reference has no such step: its data order is the database cursor of data_layer.cpp (and convert_imageset
// --shuffle when the database is built); the generator and both rules below are this project's own.
//
// The whole definition, so that a few lines of any language reproduce the lists (all arithmetic on unsigned 64-bit words, wrapping):
//   splitmix64   state = seed;   next():  state += 0x9E3779B97F4A7C15;  z = state;
//                                         z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
//                                         return z ^ (z >> 31)
//   shuffled     ONE stream for the whole call.  Epoch e: out[e][i] = i for i in 0 .. n - 1, then Fisher-Yates,
//                for i = n - 1 down to 1:  j = (next() * (i + 1)) >> 64  (the high 64 bits of the 128-bit product; 0 <= j <= i);
//                swap out[e][i], out[e][j].   n == 1 draws nothing.
//   fold         perm = shuffled(seed, n, 1);  lo = floor(fold n / folds), hi = floor((fold + 1) n / folds);
//                held = perm[lo .. hi), train = perm[0 .. lo) then perm[hi .. n): both in perm's order.  folds <= n, so no fold is empty.
#pragma once
#include <cstdint>

namespace vv {

struct SplitMix64 {
  uint64_t state;
  explicit SplitMix64(uint64_t seed) : state(seed) {}
  uint64_t next() {
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

// what is wrong with the arguments (0: nothing); the exported functions turn it into VV_ERR_ARG and a message
enum RowsError { ROWS_OK = 0, ROWS_BAD_N, ROWS_BAD_EPOCHS, ROWS_BAD_FOLDS, ROWS_BAD_FOLD, ROWS_NULL };

// out [epochs][n]
inline RowsError rows_shuffled(uint64_t seed, int32_t n, int32_t epochs, int32_t* out) {
  if (n < 1) return ROWS_BAD_N;
  if (epochs < 1) return ROWS_BAD_EPOCHS;
  if (!out) return ROWS_NULL;
  SplitMix64 rng(seed);
  for (int32_t e = 0; e < epochs; ++e) {
    int32_t* p = out + (int64_t)e * n;
    for (int32_t i = 0; i < n; ++i) p[i] = i;
    for (int32_t i = n - 1; i >= 1; --i) {
      const uint64_t j = (uint64_t)(((unsigned __int128)rng.next() * (uint64_t)((int64_t)i + 1)) >> 64);
      const int32_t t = p[i]; p[i] = p[j]; p[j] = t;
    }
  }
  return ROWS_OK;
}

// the bounds [lo, hi) of fold `fold` of `folds` within a permutation of n items
inline void rows_fold_bounds(int32_t n, int32_t folds, int32_t fold, int64_t* lo, int64_t* hi) {
  *lo = (int64_t)fold * n / folds;
  *hi = ((int64_t)fold + 1) * n / folds;
}

// train [n - (hi - lo)], held [hi - lo]: exactly that many entries are written to each; perm: scratch of the caller, [n]
inline RowsError rows_fold(uint64_t seed, int32_t n, int32_t folds, int32_t fold, int32_t* perm, int32_t* train, int64_t* n_train,
                           int32_t* held, int64_t* n_held) {
  if (n < 1) return ROWS_BAD_N;
  if (folds < 2 || folds > n) return ROWS_BAD_FOLDS;
  if (fold < 0 || fold >= folds) return ROWS_BAD_FOLD;
  if (!perm || !train || !n_train || !held || !n_held) return ROWS_NULL;
  rows_shuffled(seed, n, 1, perm);
  int64_t lo, hi;
  rows_fold_bounds(n, folds, fold, &lo, &hi);
  int64_t nt = 0, nh = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (i >= lo && i < hi) held[nh++] = perm[i];
    else train[nt++] = perm[i];
  }
  *n_train = nt; *n_held = nh;
  return ROWS_OK;
}

}  // namespace vv
