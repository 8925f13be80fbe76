// solver.cpp -- Solver / SGDSolver (reference: src/caffe/solver.cpp).  The arithmetic of
// ComputeUpdateValue + Net::Update runs as one fused HIP kernel; this file keeps the reference's
// control flow, log lines (parsed by caffe_utils/plot_training_stats.py) and snapshot formats.
#include "caffe/solver.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

namespace caffe {

template <typename Dtype>
Solver<Dtype>::Solver(const SolverParameter& param) : param_("SolverParameter"), iter_(0) { Init(param); }
template <typename Dtype>
Solver<Dtype>::Solver(const string& param_file) : param_("SolverParameter"), iter_(0) {
  SolverParameter param("SolverParameter");
  pl::ReadProtoFromTextFileOrDie(param_file, &param);
  Init(param);
}

// ---- which nets a SolverParameter names -------------------------------------------------------------------------
// The reference accepts the train net from one of four fields and the test nets from three kinds of source
// (solver.cpp:46-157).  Here the fields are tables; what is contract is which field wins, the CHECK messages and the
// "Creating ..." log lines.
namespace {

// level and stages of `src` laid over `dst` (NetState::MergeFrom for the two fields the path uses)
void OverlayState(const NetState& src, NetState* dst) {
  if (src.has("level")) dst->set_int("level", src.get_int("level"));
  for (int i = 0; i < src.size("stage"); ++i) dst->add_str("stage", src.get_str("stage", i));
}

struct NetField { const char* name; bool is_file; const char* what; };
const NetField kTrainFields[] = {     // later entries override earlier ones (solver.cpp:52-71)
  {"train_net_param", false, "Creating training net specified in train_net_param."},
  {"train_net", true, "Creating training net from train_net file: "},
  {"net_param", false, "Creating training net specified in net_param."},
  {"net", true, "Creating training net from net file: "},
};

NetParameter ReadNet(const SolverParameter& sp, const char* field, bool is_file, int index) {
  NetParameter np("NetParameter");
  if (is_file) pl::ReadProtoFromTextFileOrDie(sp.get_str(field, index), &np);
  else np = sp.get_msg(field, index);
  return np;
}

NetParameter TrainNetOf(const SolverParameter& sp) {
  int given = 0;
  for (const NetField& f : kTrainFields) given += sp.has(f.name) ? 1 : 0;
  const string field_names = "net, net_param, train_net, train_net_param";
  CHECK_GE(given, 1) << "SolverParameter must specify a train net using one of these fields: " << field_names;
  CHECK_LE(given, 1) << "SolverParameter must not contain more than one of these fields specifying a train_net: " << field_names;
  NetParameter np("NetParameter");
  for (const NetField& f : kTrainFields) {
    if (!sp.has(f.name)) continue;
    if (f.is_file) LOG(INFO) << f.what << sp.get_str(f.name); else LOG(INFO) << f.what;
    np = ReadNet(sp, f.name, f.is_file, 0);
  }
  // net state, weakest first: phase TRAIN, the net's own state, the solver's train_state (solver.cpp:73-80)
  NetState state("NetState");
  state.set_enum("phase", "TRAIN");
  if (np.has("state")) OverlayState(np.get_msg("state"), &state);
  if (sp.has("train_state")) OverlayState(sp.get_msg("train_state"), &state);
  *np.mutable_msg("state") = state;
  return np;
}

vector<NetParameter> TestNetsOf(const SolverParameter& sp) {
  const bool generic_inline = sp.has("net_param"), generic_file = sp.has("net");
  CHECK_LE(generic_inline + generic_file, 1) << "Both net_param and net_file may not be specified.";
  const int explicit_nets = sp.size("test_net_param") + sp.size("test_net");
  const int iters_given = sp.size("test_iter");
  if (generic_inline || generic_file) CHECK_GE(iters_given, explicit_nets) << "test_iter must be specified for each test network.";
  else CHECK_EQ(iters_given, explicit_nets) << "test_iter must be specified for each test network.";
  const int instances = iters_given;                       // explicit ones first, the generic net fills the rest
  if (sp.size("test_state")) CHECK_EQ(sp.size("test_state"), instances) << "test_state must be unspecified or specified once per test net.";
  if (instances) CHECK_GT(sp.get_int("test_interval"), 0);
  vector<NetParameter> nets;
  for (int i = 0; i < sp.size("test_net_param"); ++i) nets.push_back(ReadNet(sp, "test_net_param", false, i));
  for (int i = 0; i < sp.size("test_net"); ++i) nets.push_back(ReadNet(sp, "test_net", true, i));
  while ((int)nets.size() < instances) nets.push_back(ReadNet(sp, generic_inline ? "net_param" : "net", !generic_inline, 0));
  for (int i = 0; i < instances; ++i) {
    NetState state("NetState");
    state.set_enum("phase", "TEST");
    if (sp.size("test_state")) OverlayState(sp.get_msg("test_state", i), &state);
    *nets[i].mutable_msg("state") = state;
  }
  return nets;
}

}  // namespace

template <typename Dtype>
void Solver<Dtype>::Init(const SolverParameter& param) {
  LOG(INFO) << "Initializing solver from parameters: \n" << param.PrintText();
  param_ = param;
  if (param_.get_int("random_seed") >= 0) Caffe::set_random_seed((unsigned)param_.get_int("random_seed"));   // solver.cpp:37-39
  InitTrainNet();
  InitTestNets();
  // A training job must never go on, unnoticed, on embeddings that f16's range has clipped: the solver runs its engine with "h16_guard" 2
  // (include/videovec.h: once a step's report shows saturated elements or faint rows of ip2, every later step stores fp32 rows) unless
  // VV_H16_GUARD names another value, which the context took when it was created.
  const char* hg = getenv("VV_H16_GUARD");
  if (!hg || !*hg) VV_CHECK(vv_set_option(Caffe::ctx(), "h16_guard", 2));
  // BVLC SolverParameter.clip_gradients (SGDSolver::ClipGradients; vv_clip_gradients_set): the norm needs the whole summed gradient, so a
  // data-parallel job that clips runs the sync exchange schedule
  clip_gradients_ = (float)param_.get_num("clip_gradients");
  if (clip_gradients_ >= 0) {
    if (Caffe::world() > 1) {
      VV_CHECK(vv_comm_schedule(Caffe::ctx(), 0));
      LOG(INFO) << "clip_gradients: " << clip_gradients_ << " -- the gradient exchange runs on the sync schedule (the norm is taken of the summed gradient)";
    }
    VV_CHECK(vv_clip_gradients_set(Caffe::ctx(), clip_gradients_));
  }
  // BVLC SolverParameter.iter_size (Solver::Step, SGDSolver::Normalize; vv_grads_bank): iter_size forward/backward passes per update.  The
  // bank is exchanged whole, once per update: a data-parallel job that accumulates runs the sync exchange schedule
  iter_size_ = (int)param_.get_int("iter_size");
  CHECK_GE(iter_size_, 1) << "iter_size must be at least 1";
  if (iter_size_ > 1) {
    CHECK(!net_->sequential()) << "iter_size: " << iter_size_ << " needs the fused training step (this net runs layer by layer)";
    if (Caffe::world() > 1 && !(clip_gradients_ >= 0)) {     // (as Net::Init chose it; clip_gradients has selected the sync schedule above)
      const char* sch = getenv("VV_COMM_SCHEDULE");
      const char* ov = getenv("VV_COMM_OVERLAP");
      const bool sync = sch ? !strcmp(sch, "sync") : (ov && atoi(ov) == 0);
      CHECK(sync) << "iter_size: " << iter_size_ << " accumulates gradients on the sync exchange schedule only (one exchange per update): set VV_COMM_SCHEDULE=sync";
    }
    LOG(INFO) << "iter_size: " << iter_size_ << " -- " << iter_size_ << " forward/backward passes are banked per update; iterations, the learning-rate policy and snapshots count updates";
  }
  // ema_decay (this project's own; vv_ema_set): the moving average of the parameters, kept on the device behind every update.  Every rank
  // averages the whole, identical matrix: a data-parallel job with the average runs the sync exchange schedule
  ema_decay_ = (float)param_.get_num("ema_decay");
  CHECK(ema_decay_ < 1.f) << "ema_decay must be negative (off) or in [0, 1)";
  if (ema_decay_ >= 0) {
    CHECK(!net_->sequential()) << "ema_decay: " << ema_decay_ << " needs the fused training step (this net runs layer by layer)";
    if (Caffe::world() > 1) {
      VV_CHECK(vv_comm_schedule(Caffe::ctx(), 0));
      LOG(INFO) << "ema_decay: " << ema_decay_ << " -- the gradient exchange runs on the sync schedule (every rank averages the whole parameter matrix)";
    }
    VV_CHECK(vv_ema_set(Caffe::ctx(), ema_decay_));
    LOG(INFO) << "ema_decay: " << ema_decay_ << " -- a moving average of the parameters is kept behind every update and written beside every snapshot (.ema.caffemodel)";
  }
  if (param_.get_bool("test_with_ema")) CHECK(ema_decay_ >= 0) << "test_with_ema needs ema_decay";
  LOG(INFO) << "Solver scaffolding done.";
}

template <typename Dtype>
void Solver<Dtype>::InitTrainNet() { net_.reset(new Net<Dtype>(TrainNetOf(param_))); }

template <typename Dtype>
void Solver<Dtype>::InitTestNets() {
  const vector<NetParameter> specs = TestNetsOf(param_);
  Caffe::set_phase(Caffe::TEST);
  for (size_t i = 0; i < specs.size(); ++i) {
    LOG(INFO) << "Creating test net (#" << i << ")";
    test_nets_.push_back(shared_ptr<Net<Dtype> >(new Net<Dtype>(specs[i])));
  }
  Caffe::set_phase(Caffe::TRAIN);
}

// ---- the training loop -------------------------------------------------------------------------------------------
// Solver::Solve (solver.cpp:159-240).  One iteration = periodic work that looks at iter_ (snapshot, test), then
// ForwardBackward, the display lines, ComputeUpdateValue + Update -- in that order, because the log lines of an
// iteration (loss, outputs, lr) are parsed as a group by caffe_utils/plot_training_stats.py:10-14.
// Data-parallel runs (Caffe::world() > 1): every rank runs this loop; only rank 0 writes snapshots.
namespace {
bool Every(int64_t period, int iter) { return period > 0 && iter % period == 0; }
}

template <typename Dtype>
void Solver<Dtype>::ReportOutputs(const Net<Dtype>& net, const char* prefix, bool with_iter, const vector<Dtype>& values) {
  // one line per scalar of every output blob: "<prefix> #k: name = [iter = I value = ]v[ (* w = w*v loss)]"  (solver.cpp:211-214, 305-315)
  size_t k = 0;
  const vector<Blob<Dtype>*>& outs = net.output_blobs();
  for (size_t j = 0; j < outs.size(); ++j) {
    const int blob = net.output_blob_indices()[j];
    const Dtype w = net.blob_loss_weights()[blob];
    for (int e = 0; e < outs[j]->count(); ++e, ++k) {
      std::ostringstream line;
      line << "    " << prefix << " #" << k << ": " << net.blob_names()[blob] << " = ";
      if (with_iter) line << "iter = " << iter_ << " value = ";
      line << values[k];
      if (w) line << " (* " << w << " = " << w * values[k] << " loss)";
      LOG(INFO) << line.str();
    }
  }
}

template <typename Dtype>
void Solver<Dtype>::Step(bool display) {
  vector<Blob<Dtype>*> no_bottom;
  net_->set_debug_info(display && param_.get_bool("debug_info"));
  net_->set_loss_needed(display);                   // the loss is read back from the device only when it is shown
  PrepareUpdate();                                  // this iteration's rate (a function of iter_) ...
  // ... and: ForwardBackward is followed by Update and nothing reads a diff in between -- unless this solver's snapshots carry the diffs
  // (snapshot_diff, caffe.proto SolverParameter field 16; Net::ToProto, net.cpp:784-800, then reads them back): such a job keeps its
  // gradient, i.e. the update stays its own launch (with the hint the shipped 4096 x 4096 shape applies the rule in the
  // weight-gradient GEMM's epilogue and the gradient never exists outside its registers)
  Dtype loss;
  if (iter_size_ == 1) {
    if (!param_.get_bool("snapshot_diff")) net_->HintUpdate();
    loss = net_->ForwardBackward(no_bottom);
  } else {
    // BVLC Solver::Step: ClearParamDiffs, iter_size x ForwardBackward adding into the diffs, loss /= iter_size.  No hint: every pass's
    // gradient is kept and banked.  The mean as the library forms it (vv_accum_stats): fp32 sum in pass order times 1.0f / iter_size
    VV_CHECK(vv_grads_bank_reset(Caffe::ctx()));
    Dtype sum = 0;
    for (int k = 0; k < iter_size_; ++k) {
      const Dtype l = net_->ForwardBackward(no_bottom);
      sum = k ? sum + l : l;
      VV_CHECK(vv_grads_bank(Caffe::ctx()));
    }
    loss = sum * (1.0f / (float)iter_size_);           // (without display the passes return the last value read: not shown)
  }
  if (!h16_warned_) {                               // (a flag of the context: nothing is read from the device)
    double fb = 0, sat = 0, faint = 0;
    VV_CHECK(vv_get_option(Caffe::ctx(), "h16_fallback", &fb));
    if (fb != 0) {
      VV_CHECK(vv_get_option(Caffe::ctx(), "h16_flagged_saturated", &sat));
      VV_CHECK(vv_get_option(Caffe::ctx(), "h16_flagged_faint_rows", &faint));
      LOG(WARNING) << "Iteration " << iter_ << ", ip2 left f16's range: " << (long long)sat << " saturated elements, " << (long long)faint
                   << " faint rows in the step reported now (four iterations back); fp32 rows from this iteration on";
      h16_warned_ = true;
    }
  }
  if (display) {
    LOG(INFO) << "Iteration " << iter_ << ", loss = " << loss;                          // solver.cpp:196
    vector<Dtype> values;
    for (Blob<Dtype>* b : net_->output_blobs()) values.insert(values.end(), b->cpu_data(), b->cpu_data() + b->count());
    ReportOutputs(*net_, "Train net output", true, values);
  }
  ComputeUpdateValue();
  net_->Update();
  if (display && clip_gradients_ >= 0) {            // (a display iteration has read the loss anyway; no synchronisation on the others)
    vv_clip_report r;
    VV_CHECK(vv_clip_stats(Caffe::ctx(), &r));
    if (r.clipped)                                  // BVLC SGDSolver::ClipGradients' line
      LOG(INFO) << "Gradient clipping: scaling down gradients (L2 norm " << r.norm << " > " << clip_gradients_ << ") by scale factor " << r.scale;
  }
}

template <typename Dtype>
void Solver<Dtype>::Solve(const char* resume_file) {
  Caffe::set_phase(Caffe::TRAIN);
  LOG(INFO) << "Solving " << net_->name();
  PreSolve();
  iter_ = 0;
  if (resume_file) {
    LOG(INFO) << "Restoring previous solver status from " << resume_file;
    Restore(resume_file);
  }
  const int first = iter_, last = (int)param_.get_int("max_iter");
  const int64_t snap = param_.get_int("snapshot"), test = param_.get_int("test_interval"), disp = param_.get_int("display");
  for (; iter_ < last; ++iter_) {
    if (iter_ > first && Every(snap, iter_)) Snapshot();
    if (Every(test, iter_) && (iter_ > 0 || param_.get_bool("test_initialization"))) TestAll();
    Step(Every(disp, iter_));
  }
  // after the last update: final snapshot, one more forward pass for the closing loss line, final test
  net_->set_loss_needed(true);
  if (param_.get_bool("snapshot_after_train")) Snapshot();
  if (Every(disp, iter_)) {
    Dtype loss;
    net_->Forward(vector<Blob<Dtype>*>(), &loss);
    LOG(INFO) << "Iteration " << iter_ << ", loss = " << loss;
  }
  if (Every(test, iter_)) TestAll();
  if (clip_gradients_ >= 0) {
    vv_clip_report r;
    VV_CHECK(vv_clip_stats(Caffe::ctx(), &r));
    LOG(INFO) << "Gradient clipping: " << (long long)r.clipped_updates << " of " << (long long)r.updates << " updates were scaled down (clip_gradients " << clip_gradients_ << ")";
  }
  LOG(INFO) << "Optimization Done.";
}

template <typename Dtype>
void Solver<Dtype>::TestAll() { for (size_t i = 0; i < test_nets_.size(); ++i) Test((int)i); }

// Solver::Test (solver.cpp:251-317): test_iter forward passes of the test net on the current weights; every scalar
// of every output blob is averaged over the passes.
template <typename Dtype>
void Solver<Dtype>::Test(const int test_net_id) {
  LOG(INFO) << "Iteration " << iter_ << ", Testing net (#" << test_net_id << ")";
  Caffe::set_phase(Caffe::TEST);
  Net<Dtype>& net = *test_nets_[test_net_id];
  if (param_.get_bool("test_with_ema")) {           // the test net's own context is given the average in the weights' place
    LOG(INFO) << "    Testing on the moving average of the parameters (ema_decay " << ema_decay_ << ")";
    net.ShareAveragedLayersWith(net_.get());
  } else {
    net.ShareTrainedLayersWith(net_.get());
  }
  const int passes = (int)param_.get_int("test_iter", test_net_id);
  const bool want_loss = param_.get_bool("test_compute_loss");
  vector<Dtype> mean;
  Dtype loss_sum = 0;
  for (int pass = 0; pass < passes; ++pass) {
    Dtype pass_loss = 0;
    const vector<Blob<Dtype>*>& outs = net.Forward(vector<Blob<Dtype>*>(), &pass_loss);
    loss_sum += pass_loss;
    size_t k = 0;
    for (Blob<Dtype>* b : outs)
      for (int e = 0; e < b->count(); ++e, ++k) {
        if (k == mean.size()) mean.push_back(0);
        mean[k] += b->cpu_data()[e];
      }
  }
  for (Dtype& m : mean) m /= passes;
  if (want_loss) LOG(INFO) << "Test loss: " << loss_sum / passes;
  ReportOutputs(net, "Test net output", false, mean);
  Caffe::set_phase(Caffe::TRAIN);
}

// ---- SolverParameter.snapshot_data_state (field 139, default false): <prefix>_iter_<N>.datastate beside the solverstate.
// The reference's snapshot (solver.cpp:320-341, 578-596) carries the iteration, the weights and the history; what the RUN carries from one
// iteration to the next -- the data layer's stream (…data_layer.cpp:768-909) and the step's own hidden state -- is left out, so its
// restored run is another run.  The file holds, in this order: the sampler state of the training net's VIDEO_SAMPLED_SHOTS_DATA layer,
// one per such layer of every TEST net (the held-out branches: their "Test loss" lines continue too), and the training context's run state
// (vv_run_state_*).  The retrieval TEST net's VIDEO_SHOT_WINDOW_TEST_DATA layer restarts with every run, as it always did.
namespace {
const char kDataStateMagic[8] = {'V', 'V', 'D', 'A', 'T', 'S', 'T', '1'};
template <typename Dtype>
void DataLayersOf(const shared_ptr<Net<Dtype> >& net, int net_id, vector<std::pair<string, VideoSampledShotsDataLayer<Dtype>*> >* out) {
  for (size_t i = 0; i < net->layers().size(); ++i)
    if (VideoSampledShotsDataLayer<Dtype>* d = dynamic_cast<VideoSampledShotsDataLayer<Dtype>*>(net->layers()[i].get()))
      out->push_back(std::make_pair((net_id < 0 ? string("train/") : "test" + std::to_string(net_id) + "/") + net->layer_names()[i], d));
}
void PutBlob(FILE* f, const string& s) { const uint64_t n = s.size(); fwrite(&n, 8, 1, f); if (n) fwrite(s.data(), 1, n, f); }
bool GetBlob(FILE* f, string* s) {
  uint64_t n = 0;
  if (fread(&n, 8, 1, f) != 1 || n > ((uint64_t)1 << 34)) return false;
  s->resize((size_t)n);
  return n == 0 || fread(&(*s)[0], 1, (size_t)n, f) == n;
}
string DataStateFileOf(const string& model_or_state_file, const string& ext) {
  if (model_or_state_file.size() > ext.size() && model_or_state_file.compare(model_or_state_file.size() - ext.size(), ext.size(), ext) == 0)
    return model_or_state_file.substr(0, model_or_state_file.size() - ext.size()) + ".datastate";
  return string();
}
}  // namespace

template <typename Dtype>
void Solver<Dtype>::SnapshotDataState(const string& file) {
  CHECK_EQ(Caffe::world(), 1) << "snapshot_data_state: one process only";
  vector<std::pair<string, VideoSampledShotsDataLayer<Dtype>*> > layers;
  DataLayersOf(net_, -1, &layers);
  for (size_t t = 0; t < test_nets_.size(); ++t) DataLayersOf(test_nets_[t], (int)t, &layers);
  int64_t n = 0, w = 0;
  VV_CHECK(vv_run_state_size(Caffe::ctx(), &n));
  string run((size_t)n, '\0');
  VV_CHECK(vv_run_state_get(Caffe::ctx(), &run[0], n, &w));
  FILE* f = fopen(file.c_str(), "wb");
  CHECK(f) << "cannot write " << file;
  fwrite(kDataStateMagic, 1, 8, f);
  const uint32_t count = (uint32_t)layers.size();
  fwrite(&count, 4, 1, f);
  for (size_t i = 0; i < layers.size(); ++i) { PutBlob(f, layers[i].first); PutBlob(f, layers[i].second->SamplerState()); }
  PutBlob(f, run);
  CHECK_EQ(fclose(f), 0) << "cannot write " << file;
  LOG(INFO) << "Snapshotting data state to " << file << " (" << count << " sampler" << (count == 1 ? "" : "s") << ", the step's carried state)";
}

template <typename Dtype>
void Solver<Dtype>::RestoreDataState(const string& file) {
  FILE* f = file.empty() ? nullptr : fopen(file.c_str(), "rb");
  if (!f) {
    LOG(INFO) << "No data state beside the restored solver state" << (file.empty() ? string() : " (" + file + ")") << ": the data layers start over, this run sees the first batches again";
    return;
  }
  vector<std::pair<string, VideoSampledShotsDataLayer<Dtype>*> > layers;
  DataLayersOf(net_, -1, &layers);
  for (size_t t = 0; t < test_nets_.size(); ++t) DataLayersOf(test_nets_[t], (int)t, &layers);
  char magic[8]; uint32_t count = 0;
  CHECK(fread(magic, 1, 8, f) == 8 && !memcmp(magic, kDataStateMagic, 8) && fread(&count, 4, 1, f) == 1) << file << " is not a data state file";
  if (count != layers.size())
    LOG(FATAL) << "data state " << file << " does not fit this solver: it holds " << count << " samplers, the nets have " << layers.size() << " VIDEO_SAMPLED_SHOTS_DATA layers";
  vector<string> blobs(count);
  for (uint32_t i = 0; i < count; ++i) {
    string name;
    CHECK(GetBlob(f, &name) && GetBlob(f, &blobs[i])) << file << " is truncated";
    if (name != layers[i].first) LOG(FATAL) << "data state " << file << " does not fit this solver: its sampler " << i << " belongs to layer " << name << ", here that is " << layers[i].first;
  }
  string run;
  CHECK(GetBlob(f, &run)) << file << " is truncated";
  fclose(f);
  // the order of include/videovec.h: parameters, histories and the update count are in place (Restore) -- then the run state, which
  // vv_params_set would reset in part; the samplers are independent of it
  if (vv_run_state_put(Caffe::ctx(), run.data(), (int64_t)run.size()) != 0)
    LOG(FATAL) << "data state " << file << " does not fit this solver: " << vv_last_error();
  for (uint32_t i = 0; i < count; ++i) layers[i].second->RestoreSamplerState(blobs[i]);
  LOG(INFO) << "Restoring data state from " << file << ": " << count << " sampler" << (count == 1 ? "" : "s") << " and the step's carried state continue where the snapshot left them";
}

// Solver::Snapshot (solver.cpp:320-341): <prefix>_iter_<N>.caffemodel + .solverstate naming the model file.
template <typename Dtype>
void Solver<Dtype>::Snapshot() {
  // data-parallel: parameters are identical on every rank, rank 0 writes.  (Under the sharded update the fp32 master rows live on
  // their owners: reading them back is a collective of the library -- vv_params_get -- so EVERY rank makes the call, then the others leave.)
  if (Caffe::world() > 1) net_->params();
  if (Caffe::rank() != 0) return;
  const string stem = param_.get_str("snapshot_prefix") + "_iter_" + std::to_string(iter_);
  const string model_file = stem + ".caffemodel", state_file = stem + ".solverstate";
  NetParameter learned("NetParameter");
  net_->ToProto(&learned, param_.get_bool("snapshot_diff"));
  LOG(INFO) << "Snapshotting to " << model_file;
  pl::WriteProtoToBinaryFile(learned, model_file);
  SolverState state("SolverState");
  SnapshotSolverState(&state);
  state.set_int("iter", iter_);
  state.set_str("learned_net", model_file);
  LOG(INFO) << "Snapshotting solver state to " << state_file;
  pl::WriteProtoToBinaryFile(state, state_file);
  if (ema_decay_ >= 0) {                            // the average, under the same layer and blob names (the solverstate does not name it)
    const string ema_file = stem + ".ema.caffemodel";
    NetParameter averaged("NetParameter");
    net_->ToProtoAveraged(&averaged);
    LOG(INFO) << "Snapshotting the moving average to " << ema_file;
    pl::WriteProtoToBinaryFile(averaged, ema_file);
  }
  if (param_.get_bool("snapshot_data_state")) SnapshotDataState(stem + ".datastate");
}

// Solver::Restore (solver.cpp:418-429)
template <typename Dtype>
void Solver<Dtype>::Restore(const char* state_file) {
  SolverState state("SolverState");
  pl::ReadProtoFromBinaryFileOrDie(state_file, &state);
  if (state.has("learned_net")) {
    NetParameter learned("NetParameter");
    pl::ReadProtoFromBinaryFileOrDie(state.get_str("learned_net"), &learned);
    net_->CopyTrainedLayersFrom(learned);
  }
  iter_ = (int)state.get_int("iter");
  RestoreSolverState(state);
  if (ema_decay_ >= 0) {                            // (behind the history: every vv_params_set starts the average from the weights)
    string ema_file;
    if (state.has("learned_net")) {
      const string model = state.get_str("learned_net"), ext = ".caffemodel";
      if (model.size() > ext.size() && model.compare(model.size() - ext.size(), ext.size(), ext) == 0)
        ema_file = model.substr(0, model.size() - ext.size()) + ".ema.caffemodel";
    }
    FILE* f = ema_file.empty() ? nullptr : fopen(ema_file.c_str(), "rb");
    if (f) {
      fclose(f);
      NetParameter averaged("NetParameter");
      pl::ReadProtoFromBinaryFileOrDie(ema_file, &averaged);
      net_->CopyAveragedLayersFrom(averaged);
      LOG(INFO) << "Restoring the moving average from " << ema_file;
    } else {
      LOG(INFO) << "No averaged model beside the restored weights" << (ema_file.empty() ? string() : " (" + ema_file + ")") << ": the moving average starts from the restored weights";
    }
  }
  // last: everything above goes through vv_params_set, which resets part of the run state
  if (param_.get_bool("snapshot_data_state")) RestoreDataState(DataStateFileOf(state_file, ".solverstate"));
}

// ------------------------------------------------------------------------------- SGD -----------
template <typename Dtype>
Dtype SGDSolver<Dtype>::GetLearningRate() {
  const SolverParameter& p = this->param_;
  const string lr_policy = p.get_str("lr_policy");
  const Dtype base = (Dtype)p.get_num("base_lr"), gamma = (Dtype)p.get_num("gamma");
  Dtype rate;
  if (lr_policy == "fixed") rate = base;
  else if (lr_policy == "step") rate = base * std::pow(gamma, (Dtype)(this->iter_ / (int)p.get_int("stepsize")));
  else if (lr_policy == "exp") rate = base * std::pow(gamma, (Dtype)this->iter_);
  else if (lr_policy == "inv") rate = base * std::pow(Dtype(1) + gamma * this->iter_, -(Dtype)p.get_num("power"));
  else { LOG(FATAL) << "Unknown learning rate policy: " << lr_policy; rate = 0; }
  return rate;
}
template <typename Dtype>
void SGDSolver<Dtype>::PreSolve() {}     // history lives on the device, zero-initialised with the parameters

template <typename Dtype>
void SGDSolver<Dtype>::ComputeUpdateValue() {
  const Dtype rate = GetLearningRate();
  if (this->param_.get_int("display") && this->iter_ % this->param_.get_int("display") == 0)
    LOG(INFO) << "Iteration " << this->iter_ << ", lr = " << rate;                    // solver.cpp:492-494
  this->net_->SetUpdateHyperParams(rate, (float)this->param_.get_num("momentum"), (float)this->param_.get_num("weight_decay"),
                                   this->param_.get_str("regularization_type"), solver_type(), (float)this->param_.get_num("delta"));
}
template <typename Dtype>
void SGDSolver<Dtype>::PrepareUpdate() {
  if (solver_type() == VV_SOLVER_RMSPROP || solver_type() == VV_SOLVER_ADAM)
    this->net_->SetSolverExt((float)this->param_.get_num("momentum2"), (float)this->param_.get_num("rms_decay"));
  this->net_->SetUpdateHyperParams(GetLearningRate(), (float)this->param_.get_num("momentum"), (float)this->param_.get_num("weight_decay"),
                                   this->param_.get_str("regularization_type"), solver_type(), (float)this->param_.get_num("delta"));
}
template <typename Dtype>
const vector<shared_ptr<Blob<Dtype> > >& SGDSolver<Dtype>::history() { this->net_->GetHistory(&history_); return history_; }
template <typename Dtype>
void SGDSolver<Dtype>::SnapshotSolverState(SolverState* state) {
  state->clear("history");
  const vector<shared_ptr<Blob<Dtype> > >& h = history();
  for (size_t i = 0; i < h.size(); ++i) h[i]->ToProto(state->add_msg("history"));
}
template <typename Dtype>
void SGDSolver<Dtype>::RestoreSolverState(const SolverState& state) {
  CHECK_EQ(state.size("history"), 2) << "Incorrect length of history blobs.";
  LOG(INFO) << "SGDSolver: restoring history";
  vector<shared_ptr<Blob<Dtype> > > h(2);
  for (int i = 0; i < 2; ++i) { h[i].reset(new Blob<Dtype>()); h[i]->FromProto(state.get_msg("history", i)); }
  this->net_->SetHistory(h);
}

template <typename Dtype, int RULE>
void UpdateRuleSolver<Dtype, RULE>::SnapshotSolverState(SolverState* state) {
  SGDSolver<Dtype>::SnapshotSolverState(state);              // m of W, m of b (the other rules: their one history)
  if (RULE != VV_SOLVER_ADAM) return;
  vector<shared_ptr<Blob<Dtype> > > v;
  this->net_->GetHistory2(&v);
  for (size_t i = 0; i < v.size(); ++i) v[i]->ToProto(state->add_msg("history"));     // then v of W, v of b
}
template <typename Dtype, int RULE>
void UpdateRuleSolver<Dtype, RULE>::RestoreSolverState(const SolverState& state) {
  if (RULE != VV_SOLVER_ADAM) { SGDSolver<Dtype>::RestoreSolverState(state); return; }
  CHECK_EQ(state.size("history"), 4) << "Incorrect length of history blobs: an Adam solverstate holds 4 (m of W, m of b, v of W, v of b).";
  LOG(INFO) << "AdamSolver: restoring history";
  vector<shared_ptr<Blob<Dtype> > > h(4);
  for (int i = 0; i < 4; ++i) { h[i].reset(new Blob<Dtype>()); h[i]->FromProto(state.get_msg("history", i)); }
  this->net_->SetHistory(vector<shared_ptr<Blob<Dtype> > >(h.begin(), h.begin() + 2));
  this->net_->SetHistory2(vector<shared_ptr<Blob<Dtype> > >(h.begin() + 2, h.end()), this->iter_);      // t continues at iter + 1
}

template <typename Dtype>
Solver<Dtype>* GetSolver(const SolverParameter& param) {
  const string type = param.get_enum("solver_type");
  if (type == "SGD") return new SGDSolver<Dtype>(param);
  if (type == "NESTEROV") return new NesterovSolver<Dtype>(param);
  if (type == "ADAGRAD") return new AdaGradSolver<Dtype>(param);
  if (type == "RMSPROP") return new RMSPropSolver<Dtype>(param);
  if (type == "ADAM") return new AdamSolver<Dtype>(param);
  if (type == "ADADELTA") LOG(FATAL) << "SolverType ADADELTA is not implemented (SGD, NESTEROV, ADAGRAD, RMSPROP, ADAM are)";
  LOG(FATAL) << "Unknown SolverType: " << type;                                        // solver.hpp:141
  return nullptr;
}

template class Solver<float>;
template class SGDSolver<float>;
template class UpdateRuleSolver<float, VV_SOLVER_NESTEROV>;
template class UpdateRuleSolver<float, VV_SOLVER_ADAGRAD>;
template class UpdateRuleSolver<float, VV_SOLVER_RMSPROP>;
template class UpdateRuleSolver<float, VV_SOLVER_ADAM>;
template Solver<float>* GetSolver(const SolverParameter& param);

}  // namespace caffe
