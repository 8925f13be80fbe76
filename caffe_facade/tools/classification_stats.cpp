// classification_stats -- per-class accuracy and average precision of a score file without Python: builds one
// CLASSIFICATION_STATS layer directly (as class_stats builds its RETRIEVAL_STATS layer), feeds it a score file in the
// text_output.txt format extract_features writes (one row per item, one column per class) plus one integer label per line,
// runs SetUp / Forward and prints `accuracy_c<k> = `, `ap_c<k> = ` for every class, then `total_accuracy = ` and `mean_ap = `.
//   classification_stats scores.txt labels.txt [--prototxt net.prototxt] [--num_classes K] [--label_channels K]
//   classification_stats features.txt labels.txt --prototypes train_features.txt train_labels.txt
// --prototypes: features.txt holds embeddings, not scores.  The training items become a device gallery whose ids are their
//   classes, vv_gallery_pool_by_id turns it into one mean per class (ascending class), vv_gallery_scores writes the dot products of
//   every test embedding with every class mean into device memory, and the layer reads them there: a nearest-class-mean
//   classifier whose scores never visit the host.  Column k is the k-th class present in train_labels.txt; they must be 0 .. C-1.
//   classification_stats features.txt labels.txt --linear train_features.txt train_labels.txt [--iters N] [--batch B] [--lr x]
//                        [--momentum m] [--weight_decay w] [--loss softmax|hinge] [--hinge_norm L1|L2]
// --linear: as --prototypes, but the classifier is a softmax linear layer trained on the training items (the reference's
//   INNER_PRODUCT under SOFTMAX_LOSS): they become a device gallery, vv_linear_fit runs N steps of SGD with momentum on it
//   (vv_linear_cfg_default's values unless given), vv_linear_scores writes the test items' logits into device memory and the
//   layer reads them there.  Prints `Linear fit: steps = N loss = first -> last` in front of the statistics.
//   --loss hinge trains the same layer under the reference's HINGE_LOSS instead (hinge_loss_layer.cpp:13-77: one linear SVM per
//   class, vv_linear_loss_set), with --hinge_norm L1 or L2 (the default here, as in the Python binding);
//   --loss softmax is the default and prints what the tool printed before the flag existed.  Another value of either: the usage, exit 2.
//   [--shuffle SEED --epochs E]: the steps take their batches from vv_rows_shuffled(SEED, items, E) -- E shuffled epochs of the training
//   items, consumed from the front and wrapping -- through vv_linear_fit_rows, instead of from the items in file order.
//   [--folds K --weight_decay a,b,c [--cv_seed S]]: K-fold cross-validation of the weight decay first.  For every decay and every fold of
//   vv_rows_fold(S, items, K, f): zero parameters, vv_linear_fit_rows on the fold's training rows, vv_linear_scores_rows of its held-out
//   rows into device memory, vv_classification_stats on them there.  Prints one line per decay, `cv weight_decay = w mean_ap = a
//   total_accuracy = t` (float sums in fold order over K), then `cv chosen weight_decay = w` (the best mean_ap, a tie to the smaller
//   decay), then trains on all items with it and prints the usual lines.  The row lists are the library's own (videovec.h), not the
//   reference's: its data order is the database cursor of data_layer.cpp.
//   --dump_rows FILE: the list(s) used, one index per line, each under a `# ...` line that names it.
//   Without these flags the tool prints what it printed before they existed.
//   classification_stats features.txt labels.txt --knn K train_features.txt train_labels.txt [--knn_weighting uniform|exp] [--knn_temperature T]
// --knn: as --prototypes, but the classifier is the k-nearest-neighbour vote: the training items become a device gallery,
//   vv_gallery_knn_scores counts the class votes of every test item's K nearest training items on the device (uniform weights, or
//   exp((s_j - s_0) / T) with T = 0.07 unless given) into device memory and the layer reads them there.  Prints
//   `kNN: k = K weighting = uniform|exp form = F` in front of the statistics, F the neighbour lists' form ("last_nearest_form": 1 streaming,
//   2 selection).  A K outside 1 .. 2048, another weighting, a T that is not a positive finite number: the usage, exit 2.
// --prototxt: the layer's parameter is the first CLASSIFICATION_STATS layer of that net file (its num_classes included) instead of
//   one made here with num_classes = the number of columns.
// --num_classes / --label_channels: override num_classes / give the label blob K channels -- the layer's shape CHECKs then fire.
#include <cstring>
#include <set>
#include <sstream>

#include "feature_files.hpp"

using namespace caffe;

static int CountRows(const char* path) {
  std::ifstream f(path);
  CHECK(f.good()) << "Failed to open " << path;
  string line;
  int n = 0;
  while (std::getline(f, line))
    if (!line.empty() && line[0] != '#') ++n;
  return n;
}

int main(int argc, char** argv) {
  vector<const char*> pos;
  const char *proto = nullptr, *train_feat = nullptr, *train_lab = nullptr;
  int num_classes = -1, label_channels = 1;
  bool linear = false, bad_flag = false, shuffle = false, knn_flag = false;
  int knn = 0;
  int32_t knn_weighting = VV_KNN_UNIFORM;
  float knn_temperature = 0.07f;
  unsigned long long shuffle_seed = 0, cv_seed = 0;
  int epochs = 0, folds = 0;
  vector<float> decays;
  const char* dump_rows = nullptr;
  int32_t lin_loss = VV_LIN_LOSS_SOFTMAX, hinge_norm = VV_NORM_L2;
  vv_linear_cfg lcfg;
  vv_linear_cfg_default(&lcfg);
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--prototypes") && i + 2 < argc) { train_feat = argv[i + 1]; train_lab = argv[i + 2]; i += 2; }
    else if (!strcmp(argv[i], "--linear") && i + 2 < argc) { train_feat = argv[i + 1]; train_lab = argv[i + 2]; linear = true; i += 2; }
    else if (!strcmp(argv[i], "--knn") && i + 3 < argc) {
      char* end = nullptr;
      const long v = strtol(argv[i + 1], &end, 10);
      if (end == argv[i + 1] || *end || v < 1 || v > 2048) bad_flag = true;
      knn = (int)v; train_feat = argv[i + 2]; train_lab = argv[i + 3]; i += 3;
    } else if (!strcmp(argv[i], "--knn_weighting") && i + 1 < argc) {
      ++i; knn_flag = true;
      if (!strcmp(argv[i], "uniform")) knn_weighting = VV_KNN_UNIFORM;
      else if (!strcmp(argv[i], "exp")) knn_weighting = VV_KNN_EXP;
      else bad_flag = true;
    } else if (!strcmp(argv[i], "--knn_temperature") && i + 1 < argc) {
      char* end = nullptr;
      knn_temperature = strtof(argv[++i], &end); knn_flag = true;
      if (end == argv[i] || *end || !(knn_temperature > 0.f) || knn_temperature > 3.4028234e38f) bad_flag = true;
    }
    else if (!strcmp(argv[i], "--iters") && i + 1 < argc) lcfg.iters = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--batch") && i + 1 < argc) lcfg.batch = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--lr") && i + 1 < argc) lcfg.lr = (float)atof(argv[++i]);
    else if (!strcmp(argv[i], "--momentum") && i + 1 < argc) lcfg.momentum = (float)atof(argv[++i]);
    else if (!strcmp(argv[i], "--weight_decay") && i + 1 < argc) {
      lcfg.weight_decay = (float)atof(argv[++i]);                       // (the first of a list: what a single value has always been)
      std::stringstream list(argv[i]);
      string item;
      decays.clear();
      while (std::getline(list, item, ',')) decays.push_back((float)atof(item.c_str()));
    }
    else if (!strcmp(argv[i], "--shuffle") && i + 1 < argc) { shuffle = true; shuffle_seed = strtoull(argv[++i], nullptr, 10); }
    else if (!strcmp(argv[i], "--epochs") && i + 1 < argc) epochs = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--folds") && i + 1 < argc) folds = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--cv_seed") && i + 1 < argc) cv_seed = strtoull(argv[++i], nullptr, 10);
    else if (!strcmp(argv[i], "--dump_rows") && i + 1 < argc) dump_rows = argv[++i];
    else if (!strcmp(argv[i], "--loss") && i + 1 < argc) {
      ++i;
      if (!strcmp(argv[i], "softmax")) lin_loss = VV_LIN_LOSS_SOFTMAX;
      else if (!strcmp(argv[i], "hinge")) lin_loss = VV_LIN_LOSS_HINGE;
      else bad_flag = true;
    } else if (!strcmp(argv[i], "--hinge_norm") && i + 1 < argc) {
      ++i;
      if (!strcmp(argv[i], "L1")) hinge_norm = VV_NORM_L1;
      else if (!strcmp(argv[i], "L2")) hinge_norm = VV_NORM_L2;
      else bad_flag = true;
    } else if (!strcmp(argv[i], "--prototxt") && i + 1 < argc) proto = argv[++i];
    else if (!strcmp(argv[i], "--num_classes") && i + 1 < argc) num_classes = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--label_channels") && i + 1 < argc) label_channels = atoi(argv[++i]);
    else pos.push_back(argv[i]);
  }
  if (shuffle != (epochs != 0) || ((shuffle || folds || dump_rows) && !linear) || (folds && decays.empty())) bad_flag = true;
  if ((knn_flag && !knn) || (knn && linear)) bad_flag = true;
  if (pos.size() != 2 || label_channels < 1 || bad_flag) {
    fprintf(stderr, "usage: classification_stats scores.txt labels.txt [--prototxt net.prototxt] [--num_classes K] [--label_channels K]\n"
                    "       classification_stats features.txt labels.txt --prototypes train_features.txt train_labels.txt\n"
                    "       classification_stats features.txt labels.txt --linear train_features.txt train_labels.txt [--iters N] [--batch B] [--lr x] [--momentum m] [--weight_decay w] [--loss softmax|hinge] [--hinge_norm L1|L2]\n"
                    "                            [--shuffle SEED --epochs E] [--folds K --weight_decay a,b,c [--cv_seed S]] [--dump_rows FILE]\n"
                    "       classification_stats features.txt labels.txt --knn K train_features.txt train_labels.txt [--knn_weighting uniform|exp] [--knn_temperature T]\n");
    return 2;
  }
  Caffe::SetDevice(0);
  Caffe::set_mode(Caffe::GPU);
  Caffe::set_phase(Caffe::TEST);
  vector<float> fv;
  int n = 0, dim = 0;
  ReadFeatures(pos[0], &fv, &n, &dim);
  Blob<float> x, labels, t0, t1, t2;
  int C = dim;
  if (train_feat) {
    vector<float> tv;
    int tn = 0, tdim = 0;
    ReadFeatures(train_feat, &tv, &tn, &tdim);
    CHECK_EQ(tdim, dim) << "training and test embeddings differ in dimension";
    Blob<float> tl;
    ReadIds(train_lab, tn, &tl);
    vector<int32_t> cls((size_t)tn);
    for (int i = 0; i < tn; ++i) cls[i] = static_cast<int>(tl.cpu_data()[i]);
    std::set<int32_t> distinct(cls.begin(), cls.end());
    C = (int)distinct.size();
    CHECK(*distinct.begin() == 0 && *distinct.rbegin() == C - 1) << "the training labels must cover the classes 0 .. " << C - 1;
    vv_gallery *items = nullptr, *means = nullptr;
    VV_CHECK(vv_gallery_create(Caffe::ctx(), tv.data(), tn, dim, cls.data(), &items));
    x.Reshape(n, C, 1, 1);
    if (linear) {
      vv_linear* lin = nullptr;
      vv_linear_report rep;
      VV_CHECK(vv_linear_create(Caffe::ctx(), dim, C, 1, &lin));
      if (lin_loss != VV_LIN_LOSS_SOFTMAX) VV_CHECK(vv_linear_loss_set(Caffe::ctx(), lin, lin_loss, hinge_norm));
      FILE* dump = nullptr;
      if (dump_rows) { dump = fopen(dump_rows, "w"); CHECK(dump) << "Failed to open " << dump_rows; }
      auto dump_list = [&](const char* what, int f, const vector<int32_t>& rows, int64_t count) {
        if (!dump) return;
        if (f >= 0) fprintf(dump, "# fold %d %s\n", f, what); else fprintf(dump, "# %s\n", what);
        for (int64_t i = 0; i < count; ++i) fprintf(dump, "%d\n", rows[(size_t)i]);
      };
      if (folds) {
        // the held-out scores of one fold: device memory, read there by vv_classification_stats
        vector<int32_t> train((size_t)tn), held((size_t)tn), held_lab((size_t)tn);
        vector<float> zero((size_t)C * dim, 0.f);
        void* held_scores = nullptr;
        VV_CHECK(vv_dev_alloc(Caffe::ctx(), (size_t)tn * C * sizeof(float), &held_scores));
        float best_ap = 0.f, best_wd = 0.f;
        for (size_t w = 0; w < decays.size(); ++w) {
          vv_linear_cfg fcfg = lcfg;
          fcfg.weight_decay = decays[w];
          float ap_sum = 0.f, acc_sum = 0.f;
          for (int f = 0; f < folds; ++f) {
            int64_t n_train = 0, n_held = 0;
            VV_CHECK(vv_rows_fold(cv_seed, tn, folds, f, train.data(), &n_train, held.data(), &n_held));
            if (w == 0) { dump_list("train", f, train, n_train); dump_list("held", f, held, n_held); }
            VV_CHECK(vv_linear_put(Caffe::ctx(), lin, zero.data(), zero.data(), zero.data(), zero.data(), 0));
            VV_CHECK(vv_linear_fit_rows(Caffe::ctx(), lin, items, cls.data(), train.data(), n_train, &fcfg, nullptr, nullptr, &rep));
            VV_CHECK(vv_linear_scores_rows(Caffe::ctx(), lin, items, held.data(), n_held, static_cast<float*>(held_scores)));
            for (int64_t i = 0; i < n_held; ++i) held_lab[(size_t)i] = cls[(size_t)held[(size_t)i]];
            vv_classification_report cr;
            VV_CHECK(vv_classification_stats(Caffe::ctx(), static_cast<const float*>(held_scores), n_held, C, held_lab.data(), 1, nullptr, nullptr,
                                             nullptr, &cr));
            ap_sum += cr.mean_ap; acc_sum += cr.total_accuracy;
          }
          const float ap = ap_sum / (float)folds, acc = acc_sum / (float)folds;
          printf("cv weight_decay = %.9g mean_ap = %.9g total_accuracy = %.9g\n", (double)decays[w], (double)ap, (double)acc);
          if (w == 0 || ap > best_ap || (ap == best_ap && decays[w] < best_wd)) { best_ap = ap; best_wd = decays[w]; }
        }
        printf("cv chosen weight_decay = %.9g\n", (double)best_wd);
        VV_CHECK(vv_dev_free(Caffe::ctx(), held_scores));
        VV_CHECK(vv_linear_put(Caffe::ctx(), lin, zero.data(), zero.data(), zero.data(), zero.data(), 0));
        lcfg.weight_decay = best_wd;
      }
      if (shuffle) {
        CHECK(epochs >= 1 && (int64_t)epochs * tn <= (1ll << 30)) << "--epochs " << epochs;
        vector<int32_t> rows((size_t)epochs * tn);
        VV_CHECK(vv_rows_shuffled(shuffle_seed, tn, epochs, rows.data()));
        dump_list("shuffled", -1, rows, (int64_t)rows.size());
        VV_CHECK(vv_linear_fit_rows(Caffe::ctx(), lin, items, cls.data(), rows.data(), (int64_t)rows.size(), &lcfg, nullptr, nullptr, &rep));
      } else {
        VV_CHECK(vv_linear_fit(Caffe::ctx(), lin, items, cls.data(), &lcfg, nullptr, nullptr, &rep));
      }
      if (dump) fclose(dump);
      printf("Linear fit: steps = %lld loss = %.9g -> %.9g\n", (long long)rep.steps, (double)rep.loss_first, (double)rep.loss_last);
      VV_CHECK(vv_linear_scores(Caffe::ctx(), lin, nullptr, fv.data(), n, x.mutable_gpu_data()));
      VV_CHECK(vv_linear_destroy(Caffe::ctx(), lin));
    } else if (knn) {
      VV_CHECK(vv_gallery_knn_scores(Caffe::ctx(), items, cls.data(), C, fv.data(), n, nullptr, knn, knn_weighting, knn_temperature,
                                     x.mutable_gpu_data(), nullptr));
      double form = 0;
      VV_CHECK(vv_gallery_get(items, "last_nearest_form", &form));
      printf("kNN: k = %d weighting = %s form = %d\n", knn, knn_weighting == VV_KNN_EXP ? "exp" : "uniform", (int)form);
    } else {
      VV_CHECK(vv_gallery_pool_by_id(Caffe::ctx(), items, &means));
      VV_CHECK(vv_gallery_scores(Caffe::ctx(), means, fv.data(), n, x.mutable_gpu_data()));
      VV_CHECK(vv_gallery_destroy(Caffe::ctx(), means));
    }
    VV_CHECK(vv_gallery_destroy(Caffe::ctx(), items));
  } else {
    Fill(fv, n, dim, &x);
  }
  const int nl = CountRows(pos[1]);                 // (its own count: a label file of another length is the layer's CHECK to make)
  ReadIds(pos[1], nl, &labels);
  if (label_channels > 1) {
    vector<float> keep(labels.cpu_data(), labels.cpu_data() + nl);
    labels.Reshape(nl, label_channels, 1, 1);
    for (int i = 0; i < nl * label_channels; ++i) labels.mutable_cpu_data()[i] = keep[i / label_channels];
  }

  LayerParameter param("LayerParameter");
  if (proto) {
    pl::Message net("NetParameter");
    pl::ReadProtoFromTextFileOrDie(proto, &net);
    int found = -1;
    for (int i = 0; i < net.size("layers") && found < 0; ++i)
      if (net.get_msg("layers", i).get_enum("type") == "CLASSIFICATION_STATS") found = i;
    CHECK_GE(found, 0) << proto << " has no CLASSIFICATION_STATS layer";
    param = net.get_msg("layers", found);
  } else {
    param.set_str("name", "classification_stats");
    param.set_enum("type", "CLASSIFICATION_STATS");
    param.mutable_msg("classification_stats_param")->set_int("num_classes", C);
  }
  if (num_classes >= 0) param.mutable_msg("classification_stats_param")->set_int("num_classes", num_classes);
  shared_ptr<Layer<float> > layer(GetLayer<float>(param));
  vector<Blob<float>*> bottom{&x, &labels}, top{&t0, &t1, &t2};
  layer->SetUp(bottom, &top);
  layer->Forward(bottom, &top);
  const int K = t0.count();
  for (int k = 0; k < K; ++k) printf("accuracy_c%d = %.9g\n", k, (double)t0.cpu_data()[k]);
  for (int k = 0; k < K; ++k) printf("ap_c%d = %.9g\n", k, (double)t1.cpu_data()[k]);
  printf("total_accuracy = %.9g\n", (double)t2.cpu_data()[0]);
  printf("mean_ap = %.9g\n", (double)static_cast<ClassificationStatsLayer<float>*>(layer.get())->mean_ap());
  return 0;
}
