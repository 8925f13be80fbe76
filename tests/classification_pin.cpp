// classification_pin -- the procedure of ClassificationStatsLayer::Forward_cpu performed with the real libstdc++, as a stand-alone
// program of this project's own text: per class a vector that starts as n dummy entries (0, false), push_back of the n real
// (score, label == class) pairs, std::sort with std::greater<std::pair<float, bool>>, a walk over the first n entries, float
// accumulation throughout.  tests/test_classification_ref_host.py holds the numpy restatement against it; tools/classification_bench.py
// times it as the host side of the comparison (`threads` > 1: the classes are spread over that many threads).
//   classification_pin in.bin out.bin [threads]
// in.bin : int32 n, int32 C, float scores[n][C], int32 labels[n]
// out.bin: int32 count[C], float accuracy[C], float ap[C], float total_accuracy, double seconds (the procedure, without the file I/O)
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <utility>
#include <vector>

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: classification_pin in.bin out.bin [threads]\n"); return 2; }
  const int threads = argc > 3 ? std::max(1, atoi(argv[3])) : 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  int32_t n = 0, C = 0;
  if (fread(&n, 4, 1, f) != 1 || fread(&C, 4, 1, f) != 1 || n < 1 || C < 1) { fprintf(stderr, "bad header\n"); return 1; }
  std::vector<float> data((size_t)n * C);
  std::vector<int32_t> label((size_t)n);
  if (fread(data.data(), 4, data.size(), f) != data.size() || fread(label.data(), 4, label.size(), f) != label.size()) {
    fprintf(stderr, "short file\n");
    return 1;
  }
  fclose(f);

  const auto t0 = std::chrono::steady_clock::now();
  std::vector<float> ap(C, 0.f), right_c(C, 0.f), acc(C, 0.f);
  std::vector<int32_t> count(C, 0);
  float right = 0.f;
  for (int i = 0; i < n; ++i) {
    int best_col = 0;
    float best = data[(size_t)i * C];
    const int lab = label[i];
    count[lab]++;
    for (int j = 0; j < C; ++j)
      if (data[(size_t)i * C + j] > best) { best_col = j; best = data[(size_t)i * C + j]; }
    if (best_col == lab) { ++right_c[lab]; ++right; }
  }
  auto one_class = [&](int c) {
    if (count[c] == 0) { acc[c] = 0.f; ap[c] = 0.f; return; }
    acc[c] = right_c[c] / count[c];
    std::vector<std::pair<float, bool> > v((size_t)n, std::make_pair(0.f, false));
    for (int i = 0; i < n; ++i) v.push_back(std::make_pair(data[(size_t)i * C + c], label[i] == c));
    std::sort(v.begin(), v.end(), std::greater<std::pair<float, bool> >());
    float prec = 0.f, hits = 0.f;
    for (int j = 0; j < n; ++j)
      if (v[j].second) { ++hits; prec += hits / (j + 1); }
    ap[c] = prec / count[c];
  };
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&, t] { for (int c = t; c < C; c += threads) one_class(c); });
  for (auto& th : pool) th.join();
  const float total = right / n;
  const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 1; }
  fwrite(count.data(), 4, C, o);
  fwrite(acc.data(), 4, C, o);
  fwrite(ap.data(), 4, C, o);
  fwrite(&total, 4, 1, o);
  fwrite(&seconds, 8, 1, o);
  fclose(o);
  return 0;
}
