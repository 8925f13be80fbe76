// Stand-alone check of the sampler's state blob (vv_sampler_state_*), host only: built together with videovector_amd/csrc/sampler.cc, e.g.
//   g++ -O1 -g -std=c++17 -march=x86-64-v3 -pthread -fsanitize=address,undefined tools/sampler_state_check.cc videovector_amd/csrc/sampler.cc -lrt -o sampler_state_check
// For every sampler family: 2k batches uninterrupted against k batches, get, put into a fresh sampler, k more -- with source and destination
// each serial and pipelined; get must not disturb the source; two gets are byte-equal; put is fed EVERY truncation of a valid blob, an
// over-long one and one with a fingerprint byte flipped, and must refuse each without touching the sampler.  Exit status 0 = all held.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "../include/videovec.h"

static uint64_t mix(uint64_t a, uint64_t b) { uint64_t x = a * 0x9E3779B97F4A7C15ull + b; x ^= x >> 31; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 29; return x; }

struct Data {
  std::vector<int32_t> vid, ns; std::vector<int64_t> rb;
  std::vector<int32_t> nvid, nns; std::vector<int64_t> nrb;      // the negative dataset (rows behind the main one's)
};
struct Batch { std::vector<int32_t> idx, last, label; bool operator==(const Batch& o) const { return idx == o.idx && last == o.last && label == o.label; } };

static vv_sampler* make(const Data& d, const vv_sampler_param& p, bool neg) {
  vv_sampler* s = nullptr;
  const int rc = vv_sampler_create_neg(&p, (int)d.vid.size(), d.vid.data(), d.ns.data(), d.rb.data(), nullptr,
                                       neg ? (int)d.nvid.size() : 0, d.nvid.data(), d.nns.data(), d.nrb.data(), nullptr, &s);
  if (rc) { printf("create failed (%d)\n", rc); exit(2); }
  return s;
}
static Batch next(vv_sampler* s, const vv_sampler_param& p) {
  const int C = p.context_type == VV_CONTEXT_PAIRWISE ? 2 : p.context_size;
  Batch b; const size_t n = (size_t)p.batch_size * (C + p.num_negative_samples);
  b.idx.assign(n, -7); b.last.assign(n, -7); b.label.assign(p.batch_size, -7);
  if (vv_sampler_next(s, b.idx.data(), b.last.data(), b.label.data())) { printf("next failed\n"); exit(2); }
  return b;
}
static const int kDepth = 3;
// the ring is full: the pipeline is provably kDepth batches ahead of the consumer
static void wait_full(vv_sampler* s) {
  for (int i = 0; i < 20000 && vv_sampler_stat(s, 10) - vv_sampler_stat(s, 11) < kDepth; ++i) std::this_thread::sleep_for(std::chrono::microseconds(100));
  if (vv_sampler_stat(s, 10) - vv_sampler_stat(s, 11) < kDepth) { printf("the pipeline did not fill its ring\n"); exit(2); }
}
static std::vector<unsigned char> get(vv_sampler* s) {
  int64_t n = 0, w = 0;
  if (vv_sampler_state_size(s, &n)) { printf("size failed\n"); exit(2); }
  std::vector<unsigned char> b((size_t)n);
  const int rc = vv_sampler_state_get(s, b.data(), n, &w);
  if (rc || w != n) { printf("get failed (%d): %s\n", rc, vv_sampler_state_error()); exit(2); }
  return b;
}

int main() {
  Data d;
  const int V = 40;
  int64_t rows = 0;
  for (int v = 0; v < V; ++v) { d.vid.push_back(1000 + v); d.ns.push_back(v % 9 == 3 ? 1 : 6 + (int)(mix(7, v) % 30)); d.rb.push_back(rows); rows += d.ns.back(); }
  for (int v = 0; v < 5; ++v) { d.nvid.push_back(5000 + v); d.nns.push_back(8); d.nrb.push_back(rows); rows += 8; }     // 40 shots: an exact fit of the buffer below
  struct Family { const char* name; int ctype, max_same, cursor; bool neg; } fams[] = {
    {"window fast path", VV_CONTEXT_WINDOW, 0, 0, false}, {"general path, max_same_video_negs 6", VV_CONTEXT_WINDOW, 6, 0, false},
    {"negative_dataset", VV_CONTEXT_WINDOW, 0, 0, true}, {"rand_skip", VV_CONTEXT_WINDOW, 0, 17, false},
    {"pairwise", VV_CONTEXT_PAIRWISE, 0, 0, false}, {"past", VV_CONTEXT_PAST, 0, 0, false}, {"past, same-video negatives", VV_CONTEXT_PAST, 3, 0, false},
  };
  const int k = 7;
  int failures = 0;
  for (const Family& f : fams) {
    vv_sampler_param p; vv_sampler_param_default(&p);
    p.batch_size = 8; p.context_size = 5; p.num_negative_samples = 10; p.max_buffer_size = 40; p.negative_swap_percentage = 50;
    p.context_type = f.ctype; p.max_same_video_negs = f.max_same; p.initial_cursor = f.cursor;
    std::vector<Batch> want;
    { vv_sampler* s = make(d, p, f.neg); for (int i = 0; i < 2 * k; ++i) want.push_back(next(s, p)); vv_sampler_destroy(s); }
    std::vector<unsigned char> blob_serial;
    for (int src_pipe = 0; src_pipe < 2; ++src_pipe)
      for (int dst_pipe = 0; dst_pipe < 2; ++dst_pipe) {
        int bad = 0;
        vv_sampler* a = make(d, p, f.neg);
        if (src_pipe && vv_sampler_prefetch_start(a, kDepth, 3, nullptr, 1)) { printf("prefetch_start failed\n"); return 2; }
        for (int i = 0; i < k; ++i) if (!(next(a, p) == want[i])) ++bad;
        if (src_pipe) wait_full(a);
        const std::vector<unsigned char> blob = get(a), again = get(a);
        if (blob != again) { printf("  two gets differ\n"); ++bad; }
        if (!src_pipe) blob_serial = blob; else if (blob != blob_serial) { printf("  the pipelined source's state differs from the serial one's\n"); ++bad; }
        for (int i = k; i < 2 * k; ++i) if (!(next(a, p) == want[i])) { printf("  get disturbed batch %d of its source\n", i); ++bad; }
        vv_sampler_destroy(a);
        vv_sampler* b = make(d, p, f.neg);
        if (vv_sampler_state_put(b, blob.data(), (int64_t)blob.size())) { printf("  put failed: %s\n", vv_sampler_state_error()); ++bad; }
        if (dst_pipe && vv_sampler_prefetch_start(b, kDepth, 3, nullptr, 1)) { printf("prefetch_start failed\n"); return 2; }
        for (int i = k; i < 2 * k; ++i) if (!(next(b, p) == want[i])) { printf("  resumed batch %d differs\n", i); ++bad; }
        if (vv_sampler_state_put(b, blob.data(), (int64_t)blob.size()) != VV_ERR_STATE) { printf("  a late put was not refused\n"); ++bad; }
        vv_sampler_destroy(b);
        printf("%-38s source %-9s destination %-9s %s\n", f.name, src_pipe ? "pipelined" : "serial", dst_pipe ? "pipelined" : "serial", bad ? "FAILED" : "ok");
        failures += bad;
      }
    // every truncation, an over-long blob, a flipped fingerprint byte: refused, and the sampler's next batch is the first of the run
    {
      int bad = 0;
      vv_sampler* b = make(d, p, f.neg);
      for (size_t n = 0; n < blob_serial.size(); ++n) {
        std::vector<unsigned char> cut(blob_serial.begin(), blob_serial.begin() + n);      // an exact-size allocation: a read past it is a sanitizer report
        if (cut.empty()) cut.reserve(1);
        if (vv_sampler_state_put(b, cut.data() ? cut.data() : (const unsigned char*)"", (int64_t)n) != VV_ERR_ARG) { printf("  truncation to %zu bytes was not refused\n", n); ++bad; }
      }
      { std::vector<unsigned char> lng = blob_serial; lng.push_back(0);
        if (vv_sampler_state_put(b, lng.data(), (int64_t)lng.size()) != VV_ERR_ARG) { printf("  an over-long blob was not refused\n"); ++bad; } }
      for (size_t o = 24; o < 112; ++o) {
        std::vector<unsigned char> fl = blob_serial; fl[o] ^= 0x10;
        if (vv_sampler_state_put(b, fl.data(), (int64_t)fl.size()) != VV_ERR_ARG) { printf("  fingerprint byte %zu flipped was not refused\n", o); ++bad; }
      }
      { std::vector<unsigned char> fl = blob_serial; fl[0] ^= 1;
        if (vv_sampler_state_put(b, fl.data(), (int64_t)fl.size()) != VV_ERR_ARG) { printf("  a damaged magic was not refused\n"); ++bad; } }
      vv_sampler_param q = p; q.batch_size = 4;
      { vv_sampler* o = make(d, q, f.neg);
        if (vv_sampler_state_put(o, blob_serial.data(), (int64_t)blob_serial.size()) != VV_ERR_ARG) { printf("  a blob of other parameters was not refused\n"); ++bad; }
        vv_sampler_destroy(o); }
      if (!(next(b, p) == want[0])) { printf("  a refused put changed the sampler\n"); ++bad; }
      vv_sampler_destroy(b);
      printf("%-38s refusals (%zu truncations)                 %s\n", f.name, blob_serial.size(), bad ? "FAILED" : "ok");
      failures += bad;
    }
  }
  printf(failures ? "sampler_state_check: %d FAILURES\n" : "sampler_state_check: all ok\n", failures);
  return failures ? 1 : 0;
}
