// Stand-alone check of the row lists of videovector_amd/csrc/vv_rows.h (vv_rows_shuffled / vv_rows_fold), host only:
//   g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -fsanitize=address,undefined -static-libasan -static-libubsan tools/rows_check.cc -o rows_check
// (make -C videovector_amd/csrc rows_check SAN="...": the sanitizers' runtimes linked into the program, so that it runs as it is).  Over small n, epochs, folds and a few seeds:
// every epoch is a permutation of 0 .. n - 1; the folds' held-out parts partition 0 .. n - 1 and each training part is the rest, in
// the permutation's order; the same seed gives the same lists and another seed (n >= 8) another; every buffer is allocated at EXACTLY
// the size the header promises to write, on the heap, so that the address sanitizer sees one entry too many; the argument errors.
// Exit status 0 = all held.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../videovector_amd/csrc/vv_rows.h"

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++g_bad; } } while (0)

static bool is_permutation(const int32_t* p, int32_t n) {
  std::vector<char> seen((size_t)n, 0);
  for (int32_t i = 0; i < n; ++i) {
    if (p[i] < 0 || p[i] >= n || seen[(size_t)p[i]]) return false;
    seen[(size_t)p[i]] = 1;
  }
  return true;
}

int main() {
  const uint64_t seeds[] = {0ull, 1ull, 7ull, 0xFFFFFFFFFFFFFFFFull, 0x123456789ABCDEFull};
  long cases = 0;
  for (uint64_t seed : seeds)
    for (int32_t n = 1; n <= 40; ++n) {
      for (int32_t epochs = 1; epochs <= 3; ++epochs) {
        // exactly epochs * n entries, on the heap: a write past either end is an error under the sanitizer
        std::unique_ptr<int32_t[]> a(new int32_t[(size_t)epochs * n]), b(new int32_t[(size_t)epochs * n]);
        CHECK(vv::rows_shuffled(seed, n, epochs, a.get()) == vv::ROWS_OK, "shuffled n=%d epochs=%d", n, epochs);
        CHECK(vv::rows_shuffled(seed, n, epochs, b.get()) == vv::ROWS_OK, "shuffled again n=%d", n);
        for (int32_t e = 0; e < epochs; ++e) CHECK(is_permutation(a.get() + (size_t)e * n, n), "seed %llu n=%d epoch %d is no permutation", (unsigned long long)seed, n, e);
        bool same = true;
        for (int64_t i = 0; i < (int64_t)epochs * n; ++i) same &= a[(size_t)i] == b[(size_t)i];
        CHECK(same, "seed %llu n=%d: two calls differ", (unsigned long long)seed, n);
        // one stream: the first epoch of a longer call is the shorter call
        if (epochs > 1) {
          std::unique_ptr<int32_t[]> one(new int32_t[(size_t)n]);
          vv::rows_shuffled(seed, n, 1, one.get());
          bool prefix = true, second_differs = false;
          for (int32_t i = 0; i < n; ++i) { prefix &= one[(size_t)i] == a[(size_t)i]; second_differs |= a[(size_t)n + i] != a[(size_t)i]; }
          CHECK(prefix, "n=%d: epoch 0 depends on the number of epochs", n);
          if (n >= 8) CHECK(second_differs, "n=%d: epoch 1 repeats epoch 0", n);
        }
        if (n >= 8) {
          vv::rows_shuffled(seed + 1, n, epochs, b.get());
          bool differs = false;
          for (int64_t i = 0; i < (int64_t)epochs * n; ++i) differs |= a[(size_t)i] != b[(size_t)i];
          CHECK(differs, "seed %llu and the next give the same list at n=%d", (unsigned long long)seed, n);
        }
        ++cases;
      }
      std::unique_ptr<int32_t[]> perm(new int32_t[(size_t)n]), scratch(new int32_t[(size_t)n]);
      vv::rows_shuffled(seed, n, 1, perm.get());
      for (int32_t folds = 2; folds <= n; ++folds) {
        std::vector<int> held_times((size_t)n, 0);
        for (int32_t fold = 0; fold < folds; ++fold) {
          int64_t lo, hi;
          vv::rows_fold_bounds(n, folds, fold, &lo, &hi);
          CHECK(hi > lo, "n=%d folds=%d fold %d is empty", n, folds, fold);
          const int64_t nh = hi - lo, nt = n - nh;
          // new int32_t[0] is a valid, zero-sized heap block: nothing may be written to it
          std::unique_ptr<int32_t[]> train(new int32_t[(size_t)nt]), held(new int32_t[(size_t)nh]);
          int64_t got_t = -1, got_h = -1;
          CHECK(vv::rows_fold(seed, n, folds, fold, scratch.get(), train.get(), &got_t, held.get(), &got_h) == vv::ROWS_OK, "fold n=%d", n);
          CHECK(got_t == nt && got_h == nh, "n=%d folds=%d fold %d: %lld + %lld entries", n, folds, fold, (long long)got_t, (long long)got_h);
          // held = perm[lo .. hi), train = the rest, both in perm's order
          bool order = true;
          for (int64_t i = 0; i < nh; ++i) order &= held[(size_t)i] == perm[(size_t)(lo + i)];
          for (int64_t i = 0; i < nt; ++i) order &= train[(size_t)i] == perm[(size_t)(i < lo ? i : i + nh)];
          CHECK(order, "n=%d folds=%d fold %d: not the permutation's order", n, folds, fold);
          for (int64_t i = 0; i < nh; ++i) held_times[(size_t)held[(size_t)i]] += 1;
          ++cases;
        }
        bool once = true;
        for (int v : held_times) once &= v == 1;
        CHECK(once, "n=%d folds=%d: the held-out parts do not partition the items", n, folds);
      }
    }
  // the argument errors; nothing is written on any of them
  int32_t buf[4] = {-9, -9, -9, -9}, perm[4];
  int64_t a = -9, b = -9;
  CHECK(vv::rows_shuffled(1, 0, 1, buf) == vv::ROWS_BAD_N, "n = 0");
  CHECK(vv::rows_shuffled(1, -3, 1, buf) == vv::ROWS_BAD_N, "n < 0");
  CHECK(vv::rows_shuffled(1, 4, 0, buf) == vv::ROWS_BAD_EPOCHS, "epochs = 0");
  CHECK(vv::rows_shuffled(1, 4, 1, nullptr) == vv::ROWS_NULL, "out NULL");
  CHECK(vv::rows_fold(1, 0, 2, 0, perm, buf, &a, buf, &b) == vv::ROWS_BAD_N, "fold n = 0");
  CHECK(vv::rows_fold(1, 4, 1, 0, perm, buf, &a, buf, &b) == vv::ROWS_BAD_FOLDS, "folds = 1");
  CHECK(vv::rows_fold(1, 4, 5, 0, perm, buf, &a, buf, &b) == vv::ROWS_BAD_FOLDS, "folds > n");
  CHECK(vv::rows_fold(1, 4, 2, 2, perm, buf, &a, buf, &b) == vv::ROWS_BAD_FOLD, "fold = folds");
  CHECK(vv::rows_fold(1, 4, 2, -1, perm, buf, &a, buf, &b) == vv::ROWS_BAD_FOLD, "fold < 0");
  CHECK(vv::rows_fold(1, 4, 2, 0, perm, nullptr, &a, buf, &b) == vv::ROWS_NULL, "train NULL");
  CHECK(buf[0] == -9 && buf[3] == -9 && a == -9 && b == -9, "a refused call wrote something");
  // the largest draw: i + 1 = 2^31 - 1 does not overflow the 128-bit product's bounds (j <= i)
  vv::SplitMix64 rng(3);
  for (int t = 0; t < 1000; ++t) {
    const uint64_t i1 = 0x7FFFFFFFull, j = (uint64_t)(((unsigned __int128)rng.next() * i1) >> 64);
    CHECK(j < i1, "j = %llu", (unsigned long long)j);
  }
  printf("%ld cases, %d failed\n", cases, g_bad);
  return g_bad ? 1 : 0;
}
