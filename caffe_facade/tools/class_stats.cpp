// class_stats -- class-level leave-one-out retrieval statistics of extracted features without Python: builds one
// RETRIEVAL_STATS layer directly (as the reference's test_retrieval_stats_layer.cpp builds its own), feeds it a feature file in
// the text_output.txt format extract_features writes plus one integer video id per line, runs SetUp / Forward and prints the
// three tops, one per line, as `name = value`.  id_to_class.txt: the layer's id_to_class_file, `video_id,class` per line.
//   class_stats features.txt video_ids.txt id_to_class.txt [--video_level] [--include_same_video] [--within_batch] [stats_output_file]
// --video_level: video_level_retrieval with max_num_videos = the number of distinct ids in video_ids.txt.
// --within_batch: leave the layer on the call it makes when neither video_level_retrieval nor stats_output_file is set
// (vv_retrieval_stats: Gram matrix and host ranking); without it the layer runs on the device gallery in every case.
#include <cstring>
#include <set>

#include "feature_files.hpp"

using namespace caffe;

int main(int argc, char** argv) {
  bool video_level = false, include_same = false, within_batch = false;
  vector<const char*> pos;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--video_level")) video_level = true;
    else if (!strcmp(argv[i], "--include_same_video")) include_same = true;
    else if (!strcmp(argv[i], "--within_batch")) within_batch = true;
    else pos.push_back(argv[i]);
  }
  if (pos.size() < 3 || pos.size() > 4) {
    fprintf(stderr, "usage: class_stats features.txt video_ids.txt id_to_class.txt [--video_level] [--include_same_video] [--within_batch] [stats_output_file]\n");
    return 2;
  }
  Caffe::SetDevice(0);
  Caffe::set_mode(Caffe::GPU);
  Caffe::set_phase(Caffe::TEST);
  vector<float> fv;
  int n = 0, dim = 0;
  ReadFeatures(pos[0], &fv, &n, &dim);
  Blob<float> x, ids, t0, t1, t2;
  Fill(fv, n, dim, &x);
  ReadIds(pos[1], n, &ids);

  LayerParameter param("LayerParameter");
  param.set_str("name", "class_stats");
  param.set_enum("type", "RETRIEVAL_STATS");
  pl::Message* rp = param.mutable_msg("retrieval_stats_param");
  rp->set_str("id_to_class_file", pos[2]);
  rp->set_int("exclude_same_video_shots", include_same ? 0 : 1);
  if (video_level) {
    std::set<float> distinct(ids.cpu_data(), ids.cpu_data() + n);
    rp->set_int("video_level_retrieval", 1);
    rp->set_int("max_num_videos", (int)distinct.size());
  }
  if (pos.size() > 3) rp->set_str("stats_output_file", pos[3]);
  shared_ptr<Layer<float> > layer(GetLayer<float>(param));
  vector<Blob<float>*> bottom{&x, &ids}, top{&t0, &t1, &t2};
  layer->SetUp(bottom, &top);
  if (!within_batch) static_cast<RetrievalStatsLayer<float>*>(layer.get())->set_gallery_path(true);
  layer->Forward(bottom, &top);
  const char* names[3] = {"test_map", "test_hit_at_1", "test_hit_at_5"};
  for (int i = 0; i < 3; ++i) printf("%s = %.9g\n", names[i], (double)top[i]->cpu_data()[0]);
  return 0;
}
