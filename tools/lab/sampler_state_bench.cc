// What a snapshot of the sampler's state costs (vv_sampler_state_get), at configuration 2's sampler parameters (2048 synthetic videos of
// 16 .. 64 shots, batch 1024, context 5, 50 negatives, buffer 5000, swap 50 %), with the four-thread pipeline running:
//   rate     batches per second of a consumer that only takes batches, over `batches` batches, repeated `reps` times
//   get      milliseconds of ONE vv_sampler_state_get after `interval` delivered batches (the replay of `interval` batches)
//   rate+get the same consumer with one get per `interval` batches
// Built with -DNO_STATE against a sampler.cc without the state calls it measures the rate alone (the parent commit's, the same way).
//   g++ -O3 -march=x86-64-v3 -std=c++17 -pthread tools/lab/sampler_state_bench.cc videovector_amd/csrc/sampler.cc -lrt -o sampler_state_bench
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../include/videovec.h"

static uint64_t mix(uint64_t seed, uint64_t x) {
  uint64_t z = seed * 0x9E3779B97F4A7C15ull + x; z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
  const int interval = argc > 1 ? atoi(argv[1]) : 2000, reps = argc > 2 ? atoi(argv[2]) : 5, threads = argc > 3 ? atoi(argv[3]) : 4;
  const int V = 2048;
  std::vector<int32_t> vid(V), ns(V); std::vector<int64_t> rb(V);
  int64_t rows = 0;
  for (int v = 0; v < V; ++v) { vid[v] = v; ns[v] = 16 + (int)(mix(1701, v) % 49); rb[v] = rows; rows += ns[v]; }
  vv_sampler_param p; vv_sampler_param_default(&p);
  p.batch_size = 1024; p.context_size = 5; p.num_negative_samples = 50; p.max_buffer_size = 5000; p.negative_swap_percentage = 50;
  std::vector<int32_t> idx((size_t)p.batch_size * 55);
  for (int with_get = 0; with_get < 2; ++with_get) {
#ifdef NO_STATE
    if (with_get) break;
#endif
    for (int r = 0; r < reps; ++r) {
      vv_sampler* s = nullptr;
      if (vv_sampler_create(&p, V, vid.data(), ns.data(), rb.data(), nullptr, &s)) return 2;
      if (vv_sampler_prefetch_start(s, 128, threads, nullptr, 1)) return 2;
      for (int i = 0; i < 200; ++i) vv_sampler_next(s, idx.data(), nullptr, nullptr);        // warm-up
      double get_ms = 0;
      const double t0 = now();
      for (int i = 0; i < interval; ++i) vv_sampler_next(s, idx.data(), nullptr, nullptr);
#ifndef NO_STATE
      if (with_get) {
        int64_t n = 0, w = 0; vv_sampler_state_size(s, &n);
        std::vector<unsigned char> blob((size_t)n);
        const double g0 = now();
        if (vv_sampler_state_get(s, blob.data(), n, &w)) return 3;
        get_ms = (now() - g0) * 1e3;
      }
#endif
      const double dt = now() - t0;
      printf("%s rep %d: %d batches in %.3f s = %.0f batches/s%s", with_get ? "rate+get" : "rate    ", r, interval, dt, interval / dt, with_get ? "" : "\n");
      if (with_get) printf(", the get %.1f ms (a replay of %d batches)\n", get_ms, interval + 200);
      vv_sampler_destroy(s);
    }
  }
  return 0;
}
