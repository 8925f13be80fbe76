// kmeans -- k-means clustering of extracted features without Python: a feature file in the text_output.txt format extract_features
// writes becomes a device gallery, vv_gallery_kmeans runs every iteration on the device, and the centroids (the same format) and the
// items' clusters (one integer per line) are written out.  The reference has no clustering: the tool is this project's own.
//   kmeans features.txt K [--iters N] [--metric euclidean|spherical] [--seed S | --init centroids.txt] --out_centroids F --out_assign F
// --seed S (default 0): the initial centroids are the items vv_kmeans_init_rows(S, items, K) names; --init: a feature file of K rows.
// Prints one line per pass, `pass t objective = o moved = m`, then `empty = e degenerate = d nonfinite_rows = r`.
#include <cstring>

#include "feature_files.hpp"

using namespace caffe;

static int usage() {
  fprintf(stderr, "usage: kmeans features.txt K [--iters N] [--metric euclidean|spherical] [--seed S | --init centroids.txt] "
                  "--out_centroids F --out_assign F\n");
  return 2;
}

int main(int argc, char** argv) {
  vv_kmeans_cfg cfg;
  vv_kmeans_cfg_default(&cfg);
  const char *init = nullptr, *out_cent = nullptr, *out_assign = nullptr;
  unsigned long long seed = 0;
  bool have_seed = false;
  vector<const char*> pos;
  for (int i = 1; i < argc; ++i) {
    const bool more = i + 1 < argc;
    if (!strcmp(argv[i], "--iters") && more) cfg.iters = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--metric") && more) {
      ++i;
      if (!strcmp(argv[i], "euclidean")) cfg.metric = VV_KMEANS_EUCLIDEAN;
      else if (!strcmp(argv[i], "spherical")) cfg.metric = VV_KMEANS_SPHERICAL;
      else { fprintf(stderr, "kmeans: --metric %s is neither euclidean nor spherical\n", argv[i]); return 2; }
    }
    else if (!strcmp(argv[i], "--seed") && more) { seed = strtoull(argv[++i], nullptr, 10); have_seed = true; }
    else if (!strcmp(argv[i], "--init") && more) init = argv[++i];
    else if (!strcmp(argv[i], "--out_centroids") && more) out_cent = argv[++i];
    else if (!strcmp(argv[i], "--out_assign") && more) out_assign = argv[++i];
    else if (!strncmp(argv[i], "--", 2)) return usage();
    else pos.push_back(argv[i]);
  }
  if (pos.size() != 2 || !out_cent || !out_assign || (init && have_seed)) return usage();
  cfg.num_clusters = atoi(pos[1]);
  Caffe::SetDevice(0);
  Caffe::set_mode(Caffe::GPU);
  Caffe::set_phase(Caffe::TEST);
  vector<float> fv, iv;
  int n = 0, dim = 0;
  ReadFeatures(pos[0], &fv, &n, &dim);
  const int K = cfg.num_clusters;
  CHECK(K >= 1 && K <= n) << "K = " << K << " is outside 1 .. " << n << " (the items of " << pos[0] << ")";
  CHECK_GE(cfg.iters, 0) << "--iters";
  vector<int> rows;
  if (init) {
    int in = 0, idim = 0;
    ReadFeatures(init, &iv, &in, &idim);
    CHECK(in == K && idim == dim) << init << " holds " << in << " rows of " << idim << " values, not " << K << " of " << dim;
  } else {
    rows.resize(K);
    VV_CHECK(vv_kmeans_init_rows(seed, n, K, rows.data()));
  }
  vv_gallery* items = nullptr;
  VV_CHECK(vv_gallery_create(Caffe::ctx(), fv.data(), n, dim, nullptr, &items));
  vector<float> cent((size_t)K * dim);
  vector<int> assign(n);
  vector<double> objective(cfg.iters + 1);
  vector<int64_t> moved(cfg.iters + 1);
  vv_kmeans_report rep;
  VV_CHECK(vv_gallery_kmeans(Caffe::ctx(), items, &cfg, init ? iv.data() : nullptr, init ? nullptr : rows.data(), cent.data(), assign.data(),
                             nullptr, objective.data(), moved.data(), &rep));
  VV_CHECK(vv_gallery_destroy(Caffe::ctx(), items));
  for (int t = 0; t <= cfg.iters; ++t) printf("pass %d objective = %.17g moved = %lld\n", t, objective[t], (long long)moved[t]);
  printf("empty = %d degenerate = %d nonfinite_rows = %lld\n", rep.empty_last, rep.degenerate_last, (long long)rep.nonfinite_rows);
  WriteFeatures(out_cent, cent.data(), K, dim);
  WriteInts(out_assign, assign.data(), n);
  return 0;
}
