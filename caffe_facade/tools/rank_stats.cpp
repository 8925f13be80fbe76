// rank_stats -- retrieval statistics of extracted features without Python: builds one RETRIEVAL_RANK_STATS_FIXED_REF layer
// directly (as the reference's layer unit tests build theirs), feeds it a reference and a query feature file in the
// text_output.txt format extract_features writes ("#features", then one line of comma-terminated values per row) plus one
// integer id per line for each, runs SetUp / Forward and prints the five tops, one per line, as `name = value`.
//   rank_stats ref_features.txt ref_ids.txt query_features.txt query_ids.txt [stats_output_file]
#include "feature_files.hpp"

using namespace caffe;

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: rank_stats ref_features.txt ref_ids.txt query_features.txt query_ids.txt [stats_output_file]\n");
    return 2;
  }
  Caffe::SetDevice(0);
  Caffe::set_mode(Caffe::GPU);
  Caffe::set_phase(Caffe::TEST);
  vector<float> rv, qv;
  int nr = 0, nq = 0, dr = 0, dq = 0;
  ReadFeatures(argv[1], &rv, &nr, &dr);
  ReadFeatures(argv[3], &qv, &nq, &dq);
  CHECK_EQ(dr, dq) << "reference and query features differ in dimension";
  Blob<float> q, qi, r, ri, t0, t1, t2, t3, t4;
  Fill(rv, nr, dr, &r); Fill(qv, nq, dq, &q);
  ReadIds(argv[2], nr, &ri); ReadIds(argv[4], nq, &qi);

  LayerParameter param("LayerParameter");
  param.set_str("name", "rank_stats");
  param.set_enum("type", "RETRIEVAL_RANK_STATS_FIXED_REF");
  if (argc > 5) param.mutable_msg("retrieval_rank_stats_fixed_ref_param")->set_str("stats_output_file", argv[5]);
  shared_ptr<Layer<float> > layer(GetLayer<float>(param));
  vector<Blob<float>*> bottom{&q, &qi, &r, &ri}, top{&t0, &t1, &t2, &t3, &t4};
  layer->SetUp(bottom, &top);
  layer->Forward(bottom, &top);
  const char* names[5] = {"median_rank", "recall_at_1", "recall_at_5", "recall_at_10", "mean_ap"};
  for (int i = 0; i < 5; ++i) printf("%s = %.9g\n", names[i], (double)top[i]->cpu_data()[0]);
  return 0;
}
