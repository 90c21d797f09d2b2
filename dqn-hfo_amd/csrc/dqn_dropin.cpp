// dqn_dropin.cpp — what replaces the reference's src/dqn.cpp in its build: the out-of-line part
// of include/dqn.hpp's `dqn::DQN` (src/dqn.hpp:56-134) and the free functions (:204-242) as a thin
// host adaptor over the C-ABI of libdqnhip.so.  It uses the same glog / gflags / boost / caffe
// NAMES as the file it replaces, so it builds against the real libraries in the reference's
// environment and against include/shim/ where they are absent (this image).  All arithmetic is in
// the library; what stays here is what must stay on the host to keep the reference's behaviour:
// the std::mt19937 draws in the reference's call order (epsilon per SelectActions call :700,
// GetRandomActorOutput :664-682, SampleTransitionsFromMemory :501-509, SampleAction :180-194),
// the Update() gate / smoothed logs / snapshot cadence (:799-826), and the 11 learner gflags
// (:21-31), which must be DEFINED here because the driver's ParseCommandLineFlags owns the single
// flag namespace (src/dqn_main.cpp:393).
#include "dqn.hpp"

#include <glog/logging.h>
#include <gflags/gflags.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>

namespace dqn {

using namespace hfo;

// the reference's learner flags, same names / defaults / help (src/dqn.cpp:21-31)
DEFINE_int32(seed, 0, "Seed the RNG. Default: time");
DEFINE_double(tau, .001, "Step size for soft updates.");
DEFINE_int32(soft_update_freq, 1, "Do SoftUpdateNet this frequently");
DEFINE_double(gamma, .99, "Discount factor of future rewards (0,1]");
DEFINE_int32(memory, 500000, "Capacity of replay memory");
DEFINE_int32(memory_threshold, 1000, "Number of transitions required to start learning");
DEFINE_int32(loss_display_iter, 1000, "Frequency of loss display");
DEFINE_int32(snapshot_freq, 10000, "Frequency (steps) snapshots");
DEFINE_bool(remove_old_snapshots, true, "Remove old snapshots when writing more recent ones.");
DEFINE_bool(snapshot_memory, true, "Snapshot the replay memory along with the network.");
DEFINE_double(beta, .5, "Mix between off-policy and on-policy updates.");
// MI355X learner flags (no counterpart in the reference; defaults reproduce its behaviour)
DEFINE_int32(minibatch, kMinibatchSize, "Minibatch size of the HIP learner (reference: kMinibatchSize = 32); multiple of 32.");
DEFINE_double(lr_gamma, 0, "-lr_policy step / exp / inv / multistep / sigmoid: Caffe's SolverParameter.gamma (NOT the discount: that is -gamma). "
              "0: what the solver parameters carry (the reference's driver sets none: 0).");
DEFINE_double(lr_power, 0, "-lr_policy inv / poly: SolverParameter.power. 0: what the solver parameters carry.");
DEFINE_int32(lr_stepsize, 0, "-lr_policy step / sigmoid: SolverParameter.stepsize. 0: what the solver parameters carry.");
DEFINE_string(lr_stepvalues, "", "-lr_policy multistep: SolverParameter.stepvalue as a comma-separated list, strictly increasing (at most 16). "
              "Empty: what the solver parameters carry.");
DEFINE_double(weight_decay, 0, "SolverParameter.weight_decay: SGDSolver::Regularize inside the optimiser pass (0: none, or what the solver parameters carry).");
DEFINE_string(regularization_type, "", "L2 or L1 (SolverParameter.regularization_type). Empty: what the solver parameters carry (L2).");
DEFINE_int32(select_actions_cap, 0, "Largest batch SelectActions accepts. 0: the reference's CHECK_LE(states_batch.size(), kMinibatchSize) "
                                    "(src/dqn.cpp:699) with this learner's -minibatch; -1: any batch (the device path has no MemoryData layer); n > 0: n.");
DEFINE_int32(hip_device, 0, "HIP device ordinal of this process's learners.");
DEFINE_bool(hip_graph, true, "Replay each update as one captured hipGraph.");
DEFINE_string(precision, "fp32", "fp32 (exact-fp32 MFMA, the parity path) or fp16 (fp16 MFMA operands, fp32 accumulate).");
DEFINE_string(act_precision, "fp32", "fp32: SelectActions / EvaluateAction run the exact-fp32 kernels on the master weights. fp16 (-precision fp16 only): "
              "they compute what the update's own forward passes compute, on the learner's fp16 weight mirrors (dqnhip_set_act_precision).");
DEFINE_bool(dynamic_loss_scale, false, "-precision fp16 only: the learner halves a per-net multiplier of its loss scales when a gradient norm is not "
                                       "finite (the step is skipped, nothing is reported) and doubles it after -loss_scale_growth_interval finite "
                                       "steps, on the device (dqnhip_config.loss_scale_mode). Off: the static scales; an overflow is fatal.");
DEFINE_int32(loss_scale_growth_interval, 2000, "-dynamic_loss_scale: finite steps in a row before a multiplier doubles (0: never grow).");
DEFINE_int32(debug_info_iter, 0, "Every this many critic iterations Update() logs the update diagnostics the device reduces from what that update left "
             "(dqnhip_diag_collect; Caffe's debug_info of the reference's debug builds): gradient norms and clip scales, per-blob mean "
             "|w| / |g| / |step| / |lag|, per-panel mean |a|, leaky fraction and dead units, Q / TD spreads, actor outputs out of bounds. "
             "Every line starts \"[Agent<t>] [Diag]\". 0: off, nothing is collected and the log is what it was.");
DEFINE_int32(evaluate_memory_freq, 0, "Every this many critic iterations Update() evaluates the nets as they stand over the WHOLE replay memory on the "
             "device (dqnhip_evaluate_memory: the update's forward passes, no step) and logs one line \"[Agent<t>] [Memory]\": mean and rms TD "
             "error, mean Q(s,a), TD target, Q(s,mu(s)) and Q(s,a) - on_policy_target, and how often mu(s) picks the stored action. "
             "0: off, nothing runs and the log is what it was. -precision fp32, single learner.");
DEFINE_bool(per_refresh_on_load, false, "-prioritized_replay: LoadReplayMemory() recomputes every loaded transition's priority from its TD error under the "
            "nets as they stand (dqnhip_per_refresh) instead of leaving all of them at p_max, and logs one \"[Agent<t>] [Memory]\" line.");
DEFINE_bool(prioritized_replay, false, "Proportional prioritized experience replay (Schaul et al. 2016) on the device: minibatches are drawn with "
            "probability p^alpha / sum from a sum tree over the replay memory, the critic's loss carries importance weights, |TD error| is "
            "written back. UpdateActorCritic() then draws nothing from the host engine. Not combinable with -deferred_updates, "
            "-pipelined_stats or -dp_rendezvous.");
DEFINE_double(per_alpha, 0.6, "-prioritized_replay: the priority exponent (0: uniform). The paper's customary value, not measured on this workload.");
DEFINE_double(per_beta, 0.4, "-prioritized_replay: the importance exponent at critic iteration 0. The paper's customary value, not measured on this workload.");
DEFINE_int32(per_beta_anneal_iters, 0, "-prioritized_replay: critic iterations over which the importance exponent rises linearly to 1 (0: constant).");
DEFINE_int32(n_step, 1, "N-step returns on the device (dqnhip_nstep_enable): the off-policy target of a sampled transition becomes "
             "sum_{k<m} gamma^k r_{t+k} + gamma^m Q'(s_{t+m}, mu'(s_{t+m})), m <= N, shorter at an episode's end and at the memory's end. "
             "1: off, nothing is called and the learner is what it was. Typical N (3 - 5) is the literature's value (D4PG, Rainbow), not "
             "measured on this workload. Composes with -prioritized_replay; not combinable with -deferred_updates, -pipelined_stats, "
             "-dp_world > 1, -evaluate_memory_freq or -per_refresh_on_load.");
DEFINE_double(explore_noise_sigma, 0.0, "Ornstein-Uhlenbeck exploration noise on the six action parameters of SelectAction's GREEDY output, in units of "
              "each parameter's range (100 for the powers, 360 for the angles), clamped to the parameter's bounds; the four action logits "
              "and the epsilon-random outputs stay as they are. One state per learner, reset by LabelTransitions (the episode's end). The "
              "noise has its own counter-based generator: random_engine's call order stays the reference's. 0: off. The literature's "
              "value is 0.1 (not measured on this workload).");
DEFINE_double(explore_noise_theta, 0.15, "-explore_noise_sigma: the mean reversion of the OU state, in (0, 1]; 1 is white Gaussian noise.");
DEFINE_double(target_noise_sigma, 0.0, "Target policy smoothing (TD3; dqnhip_target_noise_enable): the critic-target's action input becomes "
              "clamp(mu'(s') + range * clip(sigma * z)) with z standard normal per row and column, sigma in units of each column's range "
              "(2 for the logits, 100 for the powers, 360 for the angles). 0: off, nothing is called. TD3's value is 0.1 (0.2 on a "
              "range of 2; not measured on this workload). -precision fp32, single learner, not with -deferred_updates or -pipelined_stats.");
DEFINE_double(target_noise_clip, 0.25, "-target_noise_sigma: the bound on sigma * z, in units of the range (TD3's 0.5 on a range of 2); 0: no clip.");
DEFINE_bool(n_step_validate_on_load, false, "LoadReplayMemory() checks, on the device, that every loaded non-terminal transition's next state is its "
            "successor's state (dqnhip_nstep_validate: what n-step windows rely on) and aborts on a violation.");
DEFINE_bool(native_state, false, "Snapshot() additionally writes <prefix>_iter_<N>.learnerstate (dqnhip_save_state: targets, sampling counters, loss-scale "
            "state, the ring's position, priorities, this object's random_engine and smoothed sums), and RestoreCriticSolver() loads the one "
            "that belongs to the restored iterations: resume is then bit-identical to never having stopped. The reference's files are "
            "written and read as without the flag.");
DEFINE_bool(native_state_async, false, "-native_state: the learner state is written behind training (dqnhip_save_state_async: frozen on the device at the "
            "snapshot, written by a writer thread). The save is joined - and older .learnerstate files removed - at the next learner-state "
            "snapshot, at a restore and when the learner is destroyed; a failed save aborts there. Same file, byte for byte.");
DEFINE_bool(snapshot_async, false, "Snapshot() writes the Caffe snapshot's files behind training (dqnhip_snapshot_async: frozen on the device at the snapshot, "
            "built and compressed by the learner's writer thread and -snapshot_async_threads compressor threads; same names, same protobuf bytes, "
            "same decompressed replay memory). The snapshot is joined - \"Snapshotting Finished!\" - before the next snapshot, before a restore or "
            "load and when the learner is destroyed; a failed snapshot aborts there. Where the library refuses (shared or data-parallel "
            "learners), the snapshot is taken synchronously.");
DEFINE_int32(snapshot_async_threads, 0, "-snapshot_async: compressor threads for the replay memory (0: the library's default, 8).");
DEFINE_bool(native_state_only_memory, false, "-native_state: a snapshot that is asked for the replay memory writes no gzip .replaymemory; the learner-state "
            "file is the memory's only copy and restores it on resume.");
DEFINE_bool(device_sampling, false, "Sample minibatch indices on the device (counter-based) instead of the host std::mt19937.");
DEFINE_bool(chained_updates, true, "UpdateActorCritic() tells the library which indices the NEXT call will draw (a copy of the engine runs ahead; "
            "dqnhip_update_chained): bursts of Update() get the launch schedule of a multi-update graph.  Same results, same RNG order.");
DEFINE_bool(pipelined_stats, false, "UpdateActorCritic() returns the (loss, avg_q) of the PREVIOUS update (dqnhip_update_pipelined): "
                                    "the device does not idle on the per-update read-back; the logged / smoothed values lag by one update.");
DEFINE_bool(deferred_updates, false, "Update() draws its indices as always but does not wait for the update: sixteen at a time are enqueued as one "
            "multi-update graph (dqnhip_update_indexed_n) and the (loss, avg_q) pairs are collected where Update() logs or snapshots "
            "(dqnhip_collect_stats).  Same weights, same log lines, same snapshots; a non-finite target aborts at the next collection.");
// Data parallelism for the UNCHANGED driver: start one process of this binary per GPU — each with its own HFO
// workers, its own replay shard, its own -save prefix and -hip_device — and the ranks' gradients are summed by RCCL inside
// libdqnhip.so twice per update (after the critic's backward and after the actor's).  Every rank's k-th UpdateActorCritic()
// pairs with every other rank's k-th: a rank that asks for an update early simply waits inside the collective until the
// others ask for theirs (episodes differ in length), and once max_iter is reached Update() becomes a no-op on every rank at
// the same update, so nobody is left waiting at the end.
DEFINE_int32(dp_world, 1, "Data-parallel group size (processes of this binary, one per GPU). 1: no group unless -dp_rendezvous is given.");
DEFINE_int32(dp_rank, 0, "This process's rank in the data-parallel group.");
DEFINE_string(dp_rendezvous, "", "File path shared by the ranks of the group (dqnhip_dp_init_file; needs no launcher). Empty: no data parallelism.");
DEFINE_bool(dp_half_grads, false, "Exchange gradients as bf16 (half the bytes on the links; meant for -precision fp16).");
DEFINE_int32(hip_agent_device_stride, 0, "Agent thread t of this process uses HIP device -hip_device + t * stride (0: all agents on -hip_device). "
                                         "BASELINE configs[3] on 4 GPUs = 2 processes x 2 agents, -dp_world 2, stride 2: agent a's rank r on GPU 2a + r.");


#define DQNHIP_CK(call) CHECK((call) == 0) << dqnhip_last_error()
static void LogMemorySweep(const dqnhip_sweep_report& r, int tid, const char* what);      // (beside LogDiagnostics, below)

namespace {

// tower widths = num_output of the InnerProduct layers named ip<i>_layer (src/dqn.cpp:406)
std::vector<int> TowerWidths(const caffe::NetParameter& np) {
  std::vector<int> widths;
  for (int i = 0; i < np.layer_size(); ++i) {
    const auto& l = np.layer(i);
    if (l.type() != "InnerProduct") continue;
    const std::string want = "ip" + std::to_string(widths.size() + 1) + "_layer";
    if (l.name() == want) widths.push_back(l.inner_product_param().num_output());
  }
  return widths;
}

void AddLayer(caffe::NetParameter& np, const std::string& name, const std::string& type,
              const std::vector<std::string>& bottoms, const std::vector<std::string>& tops) {
  caffe::LayerParameter* l = np.add_layer();
  l->set_name(name); l->set_type(type);
  for (const auto& b : bottoms) l->add_bottom(b);
  for (const auto& t : tops) l->add_top(t);
}
void AddMemoryData(caffe::NetParameter& np, const std::string& name, const std::vector<std::string>& tops, int n, int c, int h, int w) {
  AddLayer(np, name, "MemoryData", {}, tops);
  auto* p = np.mutable_layer(np.layer_size() - 1)->mutable_memory_data_param();
  p->set_batch_size(n); p->set_channels(c); p->set_height(h); p->set_width(w);
}
void AddInnerProduct(caffe::NetParameter& np, const std::string& name, const std::string& bottom, const std::string& top, int num_output) {
  AddLayer(np, name, "InnerProduct", {bottom}, {top});
  np.mutable_layer(np.layer_size() - 1)->mutable_inner_product_param()->set_num_output(num_output);   // gaussian(0.01) filler, :348-352
}
// ip<i>_layer (InnerProduct) + ip<i>_relu_layer (ReLU 0.01, in place) per width (src/dqn.cpp:400-416)
std::string AddTower(caffe::NetParameter& np, std::string input, const std::vector<int>& widths) {
  for (size_t i = 1; i <= widths.size(); ++i) {
    const std::string top = "ip" + std::to_string(i);
    AddInnerProduct(np, top + "_layer", input, top, widths[i - 1]);
    AddLayer(np, top + "_relu_layer", "ReLU", {top}, {top});
    np.mutable_layer(np.layer_size() - 1)->mutable_relu_param()->set_negative_slope(0.01f);
    input = top;
  }
  return input;
}
const std::vector<int> kDefaultTower = {1024, 512, 256, 128};     // src/dqn.cpp:425, 449

}  // namespace

caffe::NetParameter CreateActorNet(int state_size) {
  caffe::NetParameter np;
  np.set_name("Actor");
  np.set_force_backward(true);
  AddMemoryData(np, state_input_layer_name, {states_blob_name, "dummy1"}, kMinibatchSize, kStateInputCount, state_size, 1);
  AddLayer(np, "silence", "Silence", {"dummy1"}, {});
  const std::string top = AddTower(np, states_blob_name, kDefaultTower);
  AddInnerProduct(np, "action_layer", top, actions_blob_name, kActionSize);
  AddInnerProduct(np, "actionpara_layer", top, action_params_blob_name, kActionParamSize);
  return np;
}

caffe::NetParameter CreateCriticNet(int state_size) {
  caffe::NetParameter np;
  np.set_name("Critic");
  np.set_force_backward(true);
  AddMemoryData(np, state_input_layer_name, {states_blob_name, "dummy1"}, kMinibatchSize, kStateInputCount, state_size, 1);
  AddMemoryData(np, action_input_layer_name, {actions_blob_name, "dummy2"}, kMinibatchSize, kStateInputCount, kActionSize, 1);
  AddMemoryData(np, action_params_input_layer_name, {action_params_blob_name, "dummy3"}, kMinibatchSize, kStateInputCount, kActionParamSize, 1);
  AddMemoryData(np, target_input_layer_name, {targets_blob_name, "dummy4"}, kMinibatchSize, 1, 1, 1);
  AddLayer(np, "silence", "Silence", {"dummy1", "dummy2", "dummy3", "dummy4"}, {});
  AddLayer(np, "concat", "Concat", {states_blob_name, actions_blob_name, action_params_blob_name}, {"state_actions"});
  np.mutable_layer(np.layer_size() - 1)->mutable_concat_param()->set_axis(2);
  const std::string top = AddTower(np, "state_actions", kDefaultTower);
  AddInnerProduct(np, q_values_layer_name, top, q_values_blob_name, 1);
  AddLayer(np, "loss", "EuclideanLoss", {q_values_blob_name, targets_blob_name}, {loss_blob_name});
  return np;
}

int GetParamOffset(const action_t action, const int arg_num) {
  if (arg_num < 0 || arg_num > 1) return -1;
  switch (action) {
    case DASH: return arg_num;
    case TURN: return arg_num == 0 ? 2 : -1;
    case TACKLE: return arg_num == 0 ? 3 : -1;
    case KICK: return 4 + arg_num;
    default: LOG(FATAL) << "Unrecognized action: " << action;
  }
  return -1;
}

Action GetAction(const ActorOutput& actor_output) {
  ActorOutput logits(actor_output);
  logits[TACKLE] = -99999;                                    // TACKLE is never chosen (src/dqn.cpp:198)
  const action_t best = (action_t)std::distance(logits.begin(), std::max_element(logits.begin(), logits.begin() + kActionSize));
  const int o1 = GetParamOffset(best, 0), o2 = GetParamOffset(best, 1);
  CHECK_GE(o1, 0);
  Action a;
  a.action = best;
  a.arg1 = actor_output[kActionSize + o1];
  a.arg2 = o2 < 0 ? 0 : actor_output[kActionSize + o2];
  return a;
}

std::string PrintActorOutput(const ActorOutput& o) {
  auto s = [](float v) { return std::to_string(v); };
  return "Dash(" + s(o[4]) + ", " + s(o[5]) + ")=" + s(o[0]) + ", Turn(" + s(o[6]) + ")=" + s(o[1]) + ", Tackle(" + s(o[7]) + ")=" + s(o[2]) +
         ", Kick(" + s(o[8]) + ", " + s(o[9]) + ")=" + s(o[3]);
}

std::vector<std::string> FilesMatchingRegexp(const std::string& regexp) {
  std::vector<char> buf(1 << 16);
  int32_t n = 0;
  while (dqnhip_files_matching_regexp(regexp.c_str(), buf.data(), buf.size(), &n) != 0) {
    CHECK(std::string(dqnhip_last_error()).find("buffer too small") != std::string::npos && buf.size() < (1u << 28)) << dqnhip_last_error();
    buf.resize(buf.size() * 4);
  }
  std::vector<std::string> out;
  std::istringstream ss(buf.data());
  for (std::string line; std::getline(ss, line);) if (!line.empty()) out.push_back(line);
  return out;
}
void RemoveFilesMatchingRegexp(const std::string& regexp) { DQNHIP_CK(dqnhip_remove_files_matching_regexp(regexp.c_str())); }
void RemoveSnapshots(const std::string& regexp, int min_iter) { DQNHIP_CK(dqnhip_remove_snapshots(regexp.c_str(), min_iter)); }
void FindLatestSnapshot(const std::string& snapshot_prefix, std::string& actor_snapshot, std::string& critic_snapshot,
                        std::string& memory_snapshot) {
  char a[4096], c[4096], m[4096];
  DQNHIP_CK(dqnhip_find_latest_snapshot(snapshot_prefix.c_str(), a, c, m, sizeof a));
  if (a[0]) actor_snapshot = a;
  if (c[0]) critic_snapshot = c;
  if (m[0]) memory_snapshot = m;
}
int FindHiScore(const std::string& snapshot_prefix) {
  int32_t s = 0;
  DQNHIP_CK(dqnhip_find_hiscore(snapshot_prefix.c_str(), &s));
  return s;
}

// ---------------------------------------------------------------------------------------------
DQN::DQN(caffe::SolverParameter& actor_solver_param, caffe::SolverParameter& critic_solver_param, std::string save_path,
         int state_size, int tid)
    : actor_solver_param_(actor_solver_param), critic_solver_param_(critic_solver_param), replay_memory_capacity_(FLAGS_memory),
      gamma_(FLAGS_gamma), random_engine(), smoothed_critic_loss_(0), smoothed_actor_loss_(0), last_snapshot_iter_(0),
      save_path_(save_path), state_size_(state_size), tid_(tid), unum_(0), minibatch_(FLAGS_minibatch), h_(nullptr) {
  unsigned seed;
  if (FLAGS_seed <= 0) {
    seed = (unsigned)std::chrono::system_clock::now().time_since_epoch().count();
    LOG(INFO) << "Seeding RNG to time (seed = " << seed << ")";
  } else {
    seed = (unsigned)FLAGS_seed;
    LOG(INFO) << "Seeding RNG with seed = " << FLAGS_seed;
  }
  random_engine.seed(seed);
  explore_seed_ = seed;          // (-explore_noise_sigma: the key of the noise draws; random_engine itself is not drawn from for them)
  // -gpu=false selects Caffe's CPU solver in the reference (KeepPlayingGames: Caffe::set_mode(Caffe::CPU),
  // src/dqn_main.cpp:208-212).  This library replaces the GPU path only and by design has no CPU fallback — a learner that
  // silently computed somewhere else would void every measurement — so the flag ends here, through the driver's own logging
  // path, with what to do instead of a bare CHECK on an internal condition.
  if (caffe::Caffe::mode() != caffe::Caffe::GPU)
    LOG(FATAL) << "[Agent" << tid << "] -gpu=false: Caffe CPU mode (src/dqn_main.cpp:208-212) is not provided by the MI355X drop-in "
               << "(libdqnhip.so has no CPU backend). Run the reference's own Caffe build for the CPU solver, or start this binary with -gpu=true.";
  CHECK(!(FLAGS_deferred_updates && FLAGS_pipelined_stats)) << "-deferred_updates cannot be combined with -pipelined_stats (both decide when an update's (loss, avg_q) reach the host)";
  CHECK(!(FLAGS_deferred_updates && FLAGS_device_sampling)) << "-deferred_updates cannot be combined with -device_sampling (deferred updates run on the indices random_engine draws)";
  CHECK(!FLAGS_per_refresh_on_load || FLAGS_prioritized_replay) << "-per_refresh_on_load needs -prioritized_replay (it rewrites the priorities a load leaves at p_max; a uniform learner has none)";
  if (FLAGS_evaluate_memory_freq > 0 || FLAGS_per_refresh_on_load) {
    CHECK(FLAGS_precision == "fp32") << "-evaluate_memory_freq / -per_refresh_on_load need -precision fp32 (the replay sweep has no fp16 form in this version)";
    CHECK(FLAGS_dp_world == 1 && FLAGS_dp_rendezvous.empty()) << "-evaluate_memory_freq / -per_refresh_on_load are single-learner options (-dp_world 1, no -dp_rendezvous)";
  }
  if (FLAGS_prioritized_replay) {
    CHECK(!FLAGS_deferred_updates) << "-prioritized_replay cannot be combined with -deferred_updates (a deferred burst runs on indices drawn ahead; a prioritized update's indices do not exist before its predecessor's write-back)";
    CHECK(!FLAGS_pipelined_stats) << "-prioritized_replay cannot be combined with -pipelined_stats";
    CHECK(FLAGS_dp_world == 1 && FLAGS_dp_rendezvous.empty()) << "-prioritized_replay is a single-learner option (-dp_world 1, no -dp_rendezvous)";
  }
  CHECK(FLAGS_explore_noise_sigma >= 0.0 && std::isfinite(FLAGS_explore_noise_sigma)) << "-explore_noise_sigma must be >= 0 and finite (got " << FLAGS_explore_noise_sigma << ")";
  CHECK(FLAGS_explore_noise_theta > 0.0 && FLAGS_explore_noise_theta <= 1.0) << "-explore_noise_theta must lie in (0, 1] (got " << FLAGS_explore_noise_theta << ")";
  CHECK(FLAGS_target_noise_sigma >= 0.0 && std::isfinite(FLAGS_target_noise_sigma)) << "-target_noise_sigma must be >= 0 and finite (got " << FLAGS_target_noise_sigma << ")";
  CHECK(FLAGS_target_noise_clip >= 0.0 && std::isfinite(FLAGS_target_noise_clip)) << "-target_noise_clip must be >= 0 and finite (got " << FLAGS_target_noise_clip << ")";
  if (FLAGS_target_noise_sigma > 0.0) {
    CHECK(!FLAGS_deferred_updates) << "-target_noise_sigma cannot be combined with -deferred_updates (target smoothing has no host-indexed graph form in this version)";
    CHECK(!FLAGS_pipelined_stats) << "-target_noise_sigma cannot be combined with -pipelined_stats";
    CHECK(FLAGS_dp_world == 1 && FLAGS_dp_rendezvous.empty()) << "-target_noise_sigma is a single-learner option (-dp_world 1, no -dp_rendezvous)";
    CHECK(FLAGS_precision != "fp16") << "-target_noise_sigma needs -precision fp32 (target smoothing has no fp16 form in this version)";
  }
  CHECK(FLAGS_n_step >= 1 && FLAGS_n_step <= DQNHIP_NSTEP_MAX) << "-n_step must lie in [1, " << DQNHIP_NSTEP_MAX << "] (got " << FLAGS_n_step << ")";
  if (FLAGS_n_step > 1) {
    CHECK(!FLAGS_deferred_updates) << "-n_step cannot be combined with -deferred_updates (a deferred burst runs as multi-update graphs on host-drawn indices, which n-step returns do not have in this version)";
    CHECK(!FLAGS_pipelined_stats) << "-n_step cannot be combined with -pipelined_stats";
    CHECK(FLAGS_dp_world == 1 && FLAGS_dp_rendezvous.empty()) << "-n_step is a single-learner option (-dp_world 1, no -dp_rendezvous)";
    CHECK(FLAGS_evaluate_memory_freq == 0 && !FLAGS_per_refresh_on_load) << "-n_step cannot be combined with -evaluate_memory_freq / -per_refresh_on_load (the replay sweep forms 1-step targets)";
  }
  std::vector<int> wa = TowerWidths(actor_solver_param_.net_param()), wc = TowerWidths(critic_solver_param_.net_param());
  if (wa.empty()) wa = kDefaultTower;
  if (wc.empty()) wc = kDefaultTower;
  CHECK(wa == wc) << "actor and critic towers must have the same widths";
  CHECK_LE(wa.size(), (size_t)DQNHIP_MAX_HIDDEN);
  dqnhip_config c;
  dqnhip_default_config(&c, state_size);
  c.minibatch = FLAGS_minibatch;
  c.num_hidden = (int)wa.size();
  for (size_t i = 0; i < wa.size(); ++i) c.hidden[i] = wa[i];
  c.replay_capacity = FLAGS_memory;
  c.soft_update_freq = FLAGS_soft_update_freq;
  c.gamma = FLAGS_gamma; c.beta = FLAGS_beta; c.tau = FLAGS_tau;
  // each solver's own hyper-parameters; the fused optimiser pass takes ONE (momentum, momentum2,
  // delta, clip) pair, so the two solvers must agree on those (the driver sets them from the same flags)
  c.actor_lr = actor_solver_param_.base_lr(); c.critic_lr = critic_solver_param_.base_lr();
  CHECK(actor_solver_param_.momentum() == critic_solver_param_.momentum() && actor_solver_param_.momentum2() == critic_solver_param_.momentum2() &&
        actor_solver_param_.clip_gradients() == critic_solver_param_.clip_gradients() && actor_solver_param_.delta() == critic_solver_param_.delta())
      << "actor and critic solvers must share momentum / momentum2 / delta / clip_gradients";
  c.momentum = critic_solver_param_.momentum(); c.momentum2 = critic_solver_param_.momentum2();
  c.delta = critic_solver_param_.delta(); c.clip_gradients = critic_solver_param_.clip_gradients();
  // -lr_policy / -max_iter (src/dqn_main.cpp:36-37, 249-256) and what else SGDSolver::GetLearningRate / Regularize read of the solver
  // parameters: ONE schedule and ONE decay serve both nets (the base rates are the solvers' own), so the two must agree.  The driver
  // sets the policy and max_iter alone; the adaptor's -lr_* / -weight_decay / -regularization_type flags supply the rest.
  {
    const caffe::SolverParameter &a = actor_solver_param_, &k = critic_solver_param_;
    bool same = a.lr_policy() == k.lr_policy() && a.max_iter() == k.max_iter() && a.gamma() == k.gamma() && a.power() == k.power() && a.stepsize() == k.stepsize() &&
                a.weight_decay() == k.weight_decay() && a.regularization_type() == k.regularization_type() && a.stepvalue_size() == k.stepvalue_size();
    for (int i = 0; same && i < a.stepvalue_size(); ++i) same = a.stepvalue(i) == k.stepvalue(i);
    CHECK(same) << "actor and critic solvers must share lr_policy / max_iter / gamma / power / stepsize / stepvalue / weight_decay / regularization_type";
    const std::string policy = k.lr_policy().empty() ? "fixed" : k.lr_policy();
    c.lr_policy = -1;
    for (int p = 0; dqnhip_lr_policy_name(p) != nullptr; ++p)
      if (policy == dqnhip_lr_policy_name(p)) c.lr_policy = p;
    CHECK(c.lr_policy >= 0) << "Unknown learning rate policy: " << policy;
    c.lr_gamma = FLAGS_lr_gamma != 0 ? (float)FLAGS_lr_gamma : k.gamma();
    c.lr_power = FLAGS_lr_power != 0 ? (float)FLAGS_lr_power : k.power();
    c.lr_stepsize = FLAGS_lr_stepsize != 0 ? FLAGS_lr_stepsize : k.stepsize();
    c.lr_max_iter = k.max_iter();
    std::vector<int> sv;
    if (!FLAGS_lr_stepvalues.empty()) {
      std::stringstream ss(FLAGS_lr_stepvalues);
      for (std::string tok; std::getline(ss, tok, ',');) {
        char* end = nullptr;
        const long v = strtol(tok.c_str(), &end, 10);
        CHECK(end != tok.c_str() && *end == 0) << "-lr_stepvalues: '" << tok << "' is not an integer (a comma-separated list, e.g. 1000,5000)";
        sv.push_back((int)v);
      }
    } else for (int i = 0; i < k.stepvalue_size(); ++i) sv.push_back(k.stepvalue(i));
    CHECK_LE(sv.size(), (size_t)DQNHIP_LR_MAX_STEPVALUES) << "lr_policy multistep: 1 to " << DQNHIP_LR_MAX_STEPVALUES << " stepvalues required";
    c.lr_n_stepvalue = (int)sv.size();
    for (size_t i = 0; i < sv.size(); ++i) c.lr_stepvalue[i] = sv[i];
    c.weight_decay = FLAGS_weight_decay != 0 ? (float)FLAGS_weight_decay : k.weight_decay();
    const std::string reg = !FLAGS_regularization_type.empty() ? FLAGS_regularization_type : k.regularization_type();
    CHECK(reg == "L2" || reg == "L1") << "Unknown regularization type: " << reg;
    c.regularization_type = reg == "L1" ? DQNHIP_REG_L1 : DQNHIP_REG_L2;
    if (c.lr_policy != DQNHIP_LR_FIXED || c.weight_decay != 0) {
      // v1: a single learner without diagnostics (the library refuses the same; here it is the driver's abort, before anything is allocated)
      CHECK_LE(FLAGS_debug_info_iter, 0) << "-debug_info_iter is not available with -lr_policy " << policy << " / -weight_decay " << c.weight_decay
                                         << " (the diagnostics price the step as lr x Adam's correction)";
      CHECK(FLAGS_dp_world == 1 && FLAGS_dp_rendezvous.empty()) << "-lr_policy " << policy << " / -weight_decay " << c.weight_decay
                                                               << " are single-learner options (-dp_world 1, no -dp_rendezvous)";
    }
  }
  // -solver (src/dqn_main.cpp:30 -> SolverParameter::set_type -> SolverRegistry::CreateSolver, src/dqn.cpp:628-629): Caffe's six type
  // strings; the fused optimiser pass runs ONE rule, so the two solvers must name the same type (the driver sets both from the flag)
  CHECK(actor_solver_param_.type() == critic_solver_param_.type()) << "actor and critic solvers must be of the same type (got '"
      << actor_solver_param_.type() << "' and '" << critic_solver_param_.type() << "')";
  CHECK(actor_solver_param_.rms_decay() == critic_solver_param_.rms_decay()) << "actor and critic solvers must share rms_decay";
  c.solver_type = -1;
  for (int s = 0; dqnhip_solver_name(s) != nullptr; ++s)
    if (critic_solver_param_.type() == dqnhip_solver_name(s)) c.solver_type = s;
  CHECK(c.solver_type >= 0) << "Unknown solver type: " << critic_solver_param_.type() << " (known types: Adam, SGD, Nesterov, AdaGrad, RMSProp, AdaDelta)";
  c.rms_decay = critic_solver_param_.rms_decay();
  // Caffe's solver constructors, with their wording (the library refuses the same; here it is the reference's abort)
  if (c.solver_type == DQNHIP_SOLVER_ADAGRAD) CHECK_EQ(0, c.momentum) << "Momentum cannot be used with AdaGrad.";
  if (c.solver_type == DQNHIP_SOLVER_RMSPROP) {
    CHECK_EQ(0, c.momentum) << "Momentum cannot be used with RMSProp.";
    CHECK_GE(c.rms_decay, 0) << "rms_decay should lie between 0 and 1.";
    CHECK_LT(c.rms_decay, 1) << "rms_decay should lie between 0 and 1.";
  }
  if (c.solver_type != DQNHIP_SOLVER_ADAM) CHECK_LE(FLAGS_debug_info_iter, 0) << "-debug_info_iter needs -solver Adam (the diagnostics are defined through Adam's m and v)";
  if (c.solver_type != DQNHIP_SOLVER_ADAM)
    CHECK(FLAGS_dp_world == 1 && FLAGS_dp_rendezvous.empty()) << "-solver " << critic_solver_param_.type() << " is a single-learner option (-dp_world 1, no -dp_rendezvous)";
  c.device = FLAGS_hip_device + tid * FLAGS_hip_agent_device_stride;
  c.use_graph = FLAGS_hip_graph ? 1 : 0;
  c.seed = seed;
  CHECK(!FLAGS_native_state_async || FLAGS_native_state) << "-native_state_async needs -native_state (it changes how the learner-state file is written)";
  CHECK(!FLAGS_native_state_only_memory || FLAGS_native_state) << "-native_state_only_memory needs -native_state (the learner-state file is then the memory's only copy)";
  CHECK(FLAGS_precision == "fp32" || FLAGS_precision == "fp16") << "-precision must be fp32 or fp16";
  c.precision = FLAGS_precision == "fp16" ? DQNHIP_FP16 : DQNHIP_FP32;
  CHECK(FLAGS_act_precision == "fp32" || FLAGS_act_precision == "fp16") << "-act_precision must be fp32 or fp16";
  CHECK(FLAGS_act_precision == "fp32" || FLAGS_precision == "fp16") << "-act_precision fp16 needs -precision fp16 (the fp32 learner keeps no fp16 weight mirrors)";
  if (FLAGS_dynamic_loss_scale) {
    CHECK(FLAGS_precision == "fp16") << "-dynamic_loss_scale needs -precision fp16 (the fp32 learner scales nothing)";
    CHECK(FLAGS_dp_world == 1 && FLAGS_dp_rendezvous.empty()) << "-dynamic_loss_scale is a single-learner option (-dp_world 1, no -dp_rendezvous)";
    CHECK_GE(FLAGS_loss_scale_growth_interval, 0) << "-loss_scale_growth_interval must be >= 0 (0: never grow)";
    c.loss_scale_mode = DQNHIP_LOSS_SCALE_DYNAMIC;
    c.loss_scale_growth_interval = FLAGS_loss_scale_growth_interval;
  }
  dp_ = !FLAGS_dp_rendezvous.empty();
  deferred_ = FLAGS_deferred_updates && !dp_;          // (data parallel: every update is a collective the ranks enter together)
  CHECK(dp_ || FLAGS_dp_world == 1) << "-dp_world > 1 needs -dp_rendezvous <path shared by the ranks>";
  if (dp_) {
    CHECK(!FLAGS_pipelined_stats) << "-pipelined_stats is a single-learner option (the data-parallel update reports its own scalars)";
    // Every agent thread's learner is its own group with its own communicator.  Two communicators whose collectives are
    // enqueued on ONE device in an order nothing coordinates is what RCCL documents as unsafe, and with a shared replay the
    // driver's global MTX around every Update() burst (src/dqn_main.cpp:358-362) closes a cross-process cycle (rank 0's agent 0
    // holds MTX inside a collective whose peer waits for rank 1's MTX, held by agent 1, whose peer waits for rank 0's MTX).
    // So: a second agent needs its own device, and ShareReplayMemory refuses data-parallel learners (below).
    CHECK(tid == 0 || FLAGS_hip_agent_device_stride > 0)
        << "-dp_rendezvous with more than one agent thread needs -hip_agent_device_stride > 0 (one device per agent: each agent's "
        << "data-parallel group has its own RCCL communicator, and two communicators must not share a device)";
    c.dp_world = FLAGS_dp_world; c.dp_rank = FLAGS_dp_rank;
  }
  DQNHIP_CK(dqnhip_create(&c, &h_));
  if (FLAGS_act_precision == "fp16") DQNHIP_CK(dqnhip_set_act_precision(h_, DQNHIP_FP16));
  if (FLAGS_prioritized_replay) {
    dqnhip_per_config pc;
    dqnhip_per_default_config(&pc);
    pc.alpha = (float)FLAGS_per_alpha; pc.beta0 = (float)FLAGS_per_beta; pc.beta_anneal_iters = FLAGS_per_beta_anneal_iters;
    pc.seed = (uint64_t)seed;
    DQNHIP_CK(dqnhip_per_enable(h_, &pc));
  }
  if (FLAGS_target_noise_sigma > 0.0) {
    dqnhip_noise_config nc;
    DQNHIP_CK(dqnhip_noise_default_config(&nc, DQNHIP_NOISE_TARGET));
    nc.sigma_logits = nc.sigma_params = (float)FLAGS_target_noise_sigma; nc.clip = (float)FLAGS_target_noise_clip; nc.seed = (uint64_t)seed;
    DQNHIP_CK(dqnhip_target_noise_enable(h_, &nc));
    LOG(INFO) << "[Agent" << tid << "] target smoothing: sigma = " << FLAGS_target_noise_sigma << ", clip = " << FLAGS_target_noise_clip;
  }
  if (FLAGS_n_step > 1) {
    DQNHIP_CK(dqnhip_nstep_enable(h_, FLAGS_n_step));
    LOG(INFO) << "[Agent" << tid << "] n-step returns: n = " << FLAGS_n_step;
  }
  if (dp_) {
    // one communicator per agent thread's learner: agents are independent DQNs (src/dqn_main.cpp:264), each its own group
    const std::string rv = FLAGS_dp_rendezvous + "_agent" + std::to_string(tid);
    LOG(INFO) << "[Agent" << tid << "] data-parallel rank " << FLAGS_dp_rank << " of " << FLAGS_dp_world << " (rendezvous " << rv << ")";
    DQNHIP_CK(dqnhip_dp_init_file(h_, rv.c_str(), FLAGS_dp_half_grads ? DQNHIP_DP_HALF_GRADS : 0, 300));
    // every rank re-synchronises at its first Update(), whether or not IT restored anything: a rank that found a snapshot under
    // its own -save prefix and a rank that did not must still enter the same collective (see SyncReplicasIfPending)
    dp_sync_pending_ = true;
    int32_t ver = 0; char path[1024] = {0};
    if (dqnhip_dp_info(&ver, path, sizeof path) == 0) LOG(INFO) << "[Agent" << tid << "] RCCL " << ver << " from " << path;
  }
}

// The driver restores / preloads AFTER construction (RestoreActorSolver, RestoreCriticSolver, LoadActorWeights, LoadCriticWeights:
// src/dqn_main.cpp:268-282), i.e. after dqnhip_dp_init's broadcast.  Ranks that resume from their own -save prefixes would then
// train diverged replicas on summed gradients, and ranks whose iteration counters differ would leave the max_iter gate of
// Update() at different updates — one of them waiting in a collective for ever.  So every such call re-arms a broadcast of
// rank 0's weights, Adam history and iterations, taken at the next Update() / UpdateActorCritic(): the first point every rank
// passes in the same order.  The flag is also set by the constructor, so the FIRST update of every rank broadcasts whether or not
// that rank restored anything (symmetric: one rank with a snapshot and one without still meet in the same collective).
// That broadcast is symmetric only BEFORE the first update: afterwards a Restore* / Load* on one rank alone would arm it on that rank
// alone (a collective with no peer), and ranks may pass Update() a different number of times per episode.  So after the group's
// first update these four calls are refused on a data-parallel learner (RearmReplicaSync): restore before training starts, on every
// rank alike — what the reference's driver does (src/dqn_main.cpp:268-282).
void DQN::SyncReplicasIfPending() {
  if (!dp_ || !dp_sync_pending_) return;
  LOG(INFO) << "[Agent" << tid_ << "] data-parallel: re-synchronising the replicas from rank 0 (weights, Adam history, iterations)";
  DQNHIP_CK(dqnhip_dp_broadcast_params(h_, 0));
  dp_sync_pending_ = false;
  dp_synced_once_ = true;
  last_snapshot_iter_ = max_iter();
}
void DQN::RearmReplicaSync(const char* what) {
  if (!dp_) return;
  if (dp_synced_once_)
    LOG(FATAL) << "[Agent" << tid_ << "] " << what << " on a data-parallel learner after its first Update(): the re-synchronising broadcast is a "
               << "collective that only this rank would enter.  Restore / load before the first update, with the same calls on every rank.";
  dp_sync_pending_ = true;
}

DQN::~DQN() { CollectDeferred(); JoinSnapshot(); JoinNativeState(); DQNHIP_CK(dqnhip_destroy(h_)); }

// ---- -deferred_updates ------------------------------------------------------------------------------------------------------
// The driver calls Update() in bursts and discards the result (src/dqn_main.cpp:340-343, 359-361; Update() is void, src/dqn.hpp:103):
// between calls it reads max_iter() only.  So Update() draws its indices where the blocking form draws them and returns; every
// other entry point that touches the learner submits what is pending first and stream order does the rest.  The pairs are collected
// - and Update()'s bookkeeping replayed in update order, each update with its own iteration numbers - at the Update() whose
// iteration numbers make a log line or a snapshot due, so both see exactly the updates the blocking form's would; and, so that the
// library's uncollected pairs (8 bytes each) stay bounded, once kMaxUncollected updates are outstanding (32 KiB).
namespace { constexpr int kSubmitEvery = 16, kMaxUncollected = 4096; }

void DQN::SubmitPending() {
  if (pend_n_ == 0) return;
  static_assert(sizeof(int) == sizeof(int32_t), "indices travel as int32");
  DQNHIP_CK(dqnhip_update_indexed_n(h_, reinterpret_cast<const int32_t*>(pend_idx_.data()), pend_n_));
  uncollected_ += pend_n_;
  pend_n_ = 0;
}

void DQN::CollectDeferred(bool bookkeep) {
  SubmitPending();
  float loss[256], avgq[256];
  while (uncollected_ > 0) {
    int32_t n = 0;
    const int rc = dqnhip_collect_stats(h_, loss, avgq, 256, &n);
    if (rc != 0) LOG(FATAL) << "[Agent" << tid_ << "] deferred update: " << dqnhip_last_error();
    CHECK_GT(n, 0) << "dqnhip_collect_stats returned nothing with " << uncollected_ << " updates outstanding";
    for (int i = 0; i < n; ++i) {
      book_critic_iter_ += 1; book_actor_iter_ += 1;
      if (bookkeep) Bookkeep(std::make_pair(loss[i], avgq[i]), book_critic_iter_, book_actor_iter_);
    }
    uncollected_ -= n;
  }
}

void DQN::StopDeferring() { CollectDeferred(); deferred_ = false; }

// src/dqn.cpp:487-498: a wall-clock timer around `iterations` calls of UpdateActorCritic() — host-drawn
// indices and a blocking (loss, avg_q) per call, unless -device_sampling / -pipelined_stats say otherwise
void DQN::Benchmark(int iterations) {
  LOG(INFO) << "*** Benchmark begins ***";
  CollectDeferred();
  const auto t0 = std::chrono::steady_clock::now();
  if (deferred_ && iterations > 0) {
    // the loop below through the deferred path: the same draws, a submit every sixteen updates, one collection at the end
    // (UpdateActorCritic() does none of Update()'s bookkeeping: the pairs are dropped)
    SyncReplicasIfPending();
    book_actor_iter_ = actor_iter(); book_critic_iter_ = critic_iter();
    pend_idx_.resize((size_t)kSubmitEvery * minibatch_);
    for (int i = 0; i < iterations; ++i) {
      const std::vector<int> idx = SampleTransitionsFromMemory(minibatch_);
      std::copy(idx.begin(), idx.end(), pend_idx_.begin() + (size_t)pend_n_ * minibatch_);
      if (++pend_n_ == kSubmitEvery) SubmitPending();
      if (uncollected_ >= kMaxUncollected) CollectDeferred(false);
    }
    CollectDeferred(false);
  } else if (FLAGS_device_sampling && !FLAGS_pipelined_stats && !dp_ && iterations > 0) {
    // nothing between the updates needs the host: the whole loop is one call (sixteen updates per hipGraph launch)
    float loss = 0.0f, avg_q = 0.0f;
    DQNHIP_CK(dqnhip_update_async_n(h_, iterations));
    DQNHIP_CK(dqnhip_read_stats(h_, &loss, &avg_q));          // blocks until the last update is done
  } else
    for (int i = 0; i < iterations; ++i) UpdateActorCritic();
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  LOG(INFO) << "Average Update: " << ms / iterations << " ms.";
  LOG(INFO) << "*** Benchmark ends ***";
}

void DQN::RestoreActorSolver(const std::string& f) { CollectDeferred(); JoinSnapshot(); RearmReplicaSync("RestoreActorSolver"); DQNHIP_CK(dqnhip_solver_restore(h_, DQNHIP_ACTOR, f.c_str())); last_snapshot_iter_ = max_iter(); }
void DQN::RestoreCriticSolver(const std::string& f) {
  CollectDeferred(); JoinSnapshot(); RearmReplicaSync("RestoreCriticSolver"); DQNHIP_CK(dqnhip_solver_restore(h_, DQNHIP_CRITIC, f.c_str())); last_snapshot_iter_ = max_iter();
  if (FLAGS_native_state) LoadNativeState(f);      // (the later of the driver's two restore calls, src/dqn_main.cpp:268-275)
}
void DQN::LoadActorWeights(const std::string& f) { CollectDeferred(); JoinSnapshot(); RearmReplicaSync("LoadActorWeights"); DQNHIP_CK(dqnhip_load_caffemodel(h_, DQNHIP_ACTOR, f.c_str())); }
void DQN::LoadCriticWeights(const std::string& f) { CollectDeferred(); JoinSnapshot(); RearmReplicaSync("LoadCriticWeights"); DQNHIP_CK(dqnhip_load_caffemodel(h_, DQNHIP_CRITIC, f.c_str())); }
void DQN::LoadReplayMemory(const std::string& f) {
  SubmitPending();
  JoinSnapshot();
  if (FLAGS_native_state && native_has_memory_) {
    // <stem>_iter_<N>.replaymemory of the prefix the learner state came from: loading it would put logical 0 back at slot 0 and reset the priorities
    const std::string head = native_stem_ + "_iter_", tail = ".replaymemory";
    if (f.size() > head.size() + tail.size() && f.compare(0, head.size(), head) == 0 && f.compare(f.size() - tail.size(), tail.size(), tail) == 0 &&
        f.find_first_not_of("0123456789", head.size()) == f.size() - tail.size()) {
      LOG(INFO) << "Skipping " << f << ": the learner state already restored the replay memory (replay_mem_size = " << memory_size() << ")";
      return;
    }
  }
  LOG(INFO) << "Loading replay memory from " << f;
  DQNHIP_CK(dqnhip_load_replay_memory(h_, f.c_str()));
  LOG(INFO) << "replay_mem_size = " << memory_size();
  if (FLAGS_n_step_validate_on_load && memory_size() > 0) {
    int64_t bad = 0; int32_t first_bad = -1;
    DQNHIP_CK(dqnhip_nstep_validate(h_, 0, -1, &bad, &first_bad));
    if (bad != 0) LOG(FATAL) << "[Agent" << tid_ << "] " << f << ": " << bad << " non-terminal transition(s) whose next state is not their successor's state (first: " << first_bad
                             << "): n-step windows would mix episodes";
    LOG(INFO) << "[Agent" << tid_ << "] [Memory] " << memory_size() << " transitions validated: every non-terminal transition is followed by its successor";
  }
  if (FLAGS_per_refresh_on_load && memory_size() > 0) {
    dqnhip_sweep_report r;
    r.struct_size = (int32_t)sizeof r;
    DQNHIP_CK(dqnhip_per_refresh(h_, 0, -1, &r));
    LogMemorySweep(r, tid_, "priorities refreshed at");
  }
}
void DQN::SnapshotReplayMemory(const std::string& f) { SubmitPending(); JoinSnapshot(); DQNHIP_CK(dqnhip_snapshot_replay_memory(h_, f.c_str())); }

void DQN::Snapshot() { Snapshot(save_path_, FLAGS_remove_old_snapshots, FLAGS_snapshot_memory); }
void DQN::Snapshot(const std::string& snapshot_prefix, bool remove_old, bool snapshot_memory) {
  SubmitPending();
  JoinSnapshot();                                    // (-snapshot_async: the previous snapshot's "Snapshotting Finished!" comes before this one's lines)
  // -native_state_only_memory: the learner-state file below carries the memory (a data-parallel learner writes none: it keeps the gzip file)
  const bool gzip_memory = snapshot_memory && !(FLAGS_native_state_only_memory && !dp_);
  if (gzip_memory) LOG(INFO) << "Snapshotting memory to " << snapshot_prefix << "_iter_" << max_iter() << ".replaymemory";
  if (FLAGS_snapshot_async) {
    if (dqnhip_snapshot_async(h_, save_path_.c_str(), snapshot_prefix.c_str(), remove_old, gzip_memory, FLAGS_snapshot_async_threads) == 0) {
      snapshot_in_flight_ = true;                    // ("Snapshotting Finished!" is printed when the snapshot is joined)
      if (FLAGS_native_state) SaveNativeState(snapshot_prefix, remove_old, snapshot_memory);
      return;
    }
    LOG(WARNING) << "[Agent" << tid_ << "] -snapshot_async: " << dqnhip_last_error() << "; this snapshot is taken synchronously";
  }
  DQNHIP_CK(dqnhip_snapshot(h_, save_path_.c_str(), snapshot_prefix.c_str(), remove_old, gzip_memory));
  if (FLAGS_native_state) SaveNativeState(snapshot_prefix, remove_old, snapshot_memory);
  LOG(INFO) << "Snapshotting Finished!";
}

// -snapshot_async: waits for the snapshot in flight (a failure aborts, as a failed synchronous snapshot does)
void DQN::JoinSnapshot() {
  if (!snapshot_in_flight_) return;
  snapshot_in_flight_ = false;
  DQNHIP_CK(dqnhip_snapshot_wait(h_, nullptr, nullptr));
  LOG(INFO) << "Snapshotting Finished!";
}

// ---- -native_state ----------------------------------------------------------------------------------------------------------
// What the learner-state file's user section carries of THIS object: the engine's operator<< text, the two running sums behind the
// smoothed log lines (their float bits: nothing else accumulates, the divisor is the flag) and last_snapshot_iter_ as it stands
// once the snapshot is done (Update()'s own snapshot assigns max_iter() right after Snapshot() returns).
void DQN::SaveNativeState(const std::string& snapshot_prefix, bool remove_old, bool snapshot_memory) {
  if (dp_) { LOG(WARNING) << "[Agent" << tid_ << "] -native_state: a data-parallel learner writes no learner state (not supported in this version)"; return; }
  if (!snapshot_from_update_) CollectDeferred();   // (a snapshot the driver asks for: the sums below must hold every update the learner has run)
  const std::string f = snapshot_prefix + "_iter_" + std::to_string(max_iter()) + ".learnerstate";
  LOG(INFO) << "Snapshotting learner state to " << f;
  uint32_t bits[2];
  static_assert(sizeof(float) == sizeof(uint32_t), "the sums travel as their bits");
  memcpy(&bits[0], &smoothed_critic_loss_, 4); memcpy(&bits[1], &smoothed_actor_loss_, 4);
  std::ostringstream user;
  user << "dqn_dropin_state 1\n" << random_engine << "\n" << bits[0] << " " << bits[1] << "\n"
       << (snapshot_from_update_ ? max_iter() : last_snapshot_iter_) << "\n";
  const std::string u = user.str();
  const std::string older = snapshot_prefix + "_iter_[0-9]+\\.learnerstate";
  if (FLAGS_native_state_async) {
    // the previous save is joined first; this one's older files go when IT is joined: a process killed while the writer runs still
    // leaves the previous complete file
    JoinNativeState();
    DQNHIP_CK(dqnhip_save_state_async(h_, f.c_str(), snapshot_memory ? 0 : DQNHIP_STATE_NO_MEMORY, u.data(), u.size()));
    native_in_flight_ = true;
    native_remove_ = remove_old ? older : std::string(); native_remove_below_ = critic_iter() - 1;
    return;
  }
  DQNHIP_CK(dqnhip_save_state(h_, f.c_str(), snapshot_memory ? 0 : DQNHIP_STATE_NO_MEMORY, u.data(), u.size()));
  if (remove_old) RemoveSnapshots(older, critic_iter() - 1);      // the .replaymemory files' rule (src/dqn.cpp:612-618)
}

// -native_state_async: waits for the save in flight (a failure aborts, as a failed synchronous save does) and removes the files it superseded
void DQN::JoinNativeState() {
  if (!native_in_flight_) return;
  native_in_flight_ = false;
  DQNHIP_CK(dqnhip_save_state_wait(h_));
  if (!native_remove_.empty()) RemoveSnapshots(native_remove_, native_remove_below_);
}

// f: <stem>_critic_iter_<N>.solverstate, just restored.  The learner state of the same snapshot is <stem>_iter_<max_iter()>.learnerstate
// and says which iterations it was taken at: only a file of exactly the restored pair is loaded.
void DQN::LoadNativeState(const std::string& f) {
  JoinNativeState();
  const size_t pos = f.rfind("_critic_iter_");
  if (pos == std::string::npos) return;
  const std::string stem = f.substr(0, pos), file = stem + "_iter_" + std::to_string(max_iter()) + ".learnerstate";
  if (!std::ifstream(file).good()) { LOG(INFO) << "[Agent" << tid_ << "] -native_state: no " << file << ", resuming from the solver states alone"; return; }
  if (dp_) { LOG(WARNING) << "[Agent" << tid_ << "] -native_state: " << file << " is not loaded into a data-parallel learner (not supported in this version)"; return; }
  dqnhip_state_info_t info;
  info.struct_size = (int32_t)sizeof info;
  if (dqnhip_state_info(file.c_str(), &info) != 0) {
    LOG(WARNING) << "[Agent" << tid_ << "] -native_state: " << dqnhip_last_error() << " - resuming from the solver states alone";
    return;
  }
  if (info.actor_iter != actor_iter() || info.critic_iter != critic_iter()) {
    LOG(WARNING) << "[Agent" << tid_ << "] -native_state: " << file << " was taken at (actor_iter, critic_iter) = (" << info.actor_iter << ", " << info.critic_iter
                 << "), the solver states restored (" << actor_iter() << ", " << critic_iter() << ") - resuming from the solver states alone";
    return;
  }
  DQNHIP_CK(dqnhip_load_state(h_, file.c_str()));
  std::string u((size_t)info.user_bytes, '\0');
  size_t n = 0;
  DQNHIP_CK(dqnhip_state_read_user(file.c_str(), &u[0], u.size(), &n));
  std::istringstream in(u.substr(0, n));
  std::string magic; int version = 0; uint32_t bits[2] = {0, 0}; int last = 0;
  std::mt19937 engine;
  in >> magic >> version >> engine >> bits[0] >> bits[1] >> last;
  if (!in || magic != "dqn_dropin_state" || version != 1)
    LOG(FATAL) << "[Agent" << tid_ << "] -native_state: " << file << ": the user section is not this adaptor's (the learner itself has been restored)";
  random_engine = engine;
  memcpy(&smoothed_critic_loss_, &bits[0], 4); memcpy(&smoothed_actor_loss_, &bits[1], 4);
  last_snapshot_iter_ = last;
  spec_valid_ = false;                             // (a prediction drawn before the restore is nobody's next minibatch)
  native_stem_ = stem; native_has_memory_ = info.has_memory != 0;
  LOG(INFO) << "[Agent" << tid_ << "] -native_state: resumed from " << file << (native_has_memory_ ? " (with the replay memory: replay_mem_size = " + std::to_string(memory_size()) + ")" : " (without a replay memory)");
}

ActorOutput DQN::GetRandomActorOutput() {
  auto u = [this](float lo, float hi) { return std::uniform_real_distribution<float>(lo, hi)(random_engine); };
  ActorOutput o;
  for (int i = 0; i < kActionSize; ++i) o[i] = u(-1.0, 1.0);
  o[kActionSize + 0] = u(-100.0, 100.0);      // Dash Power   (draw order = src/dqn.cpp:669-680)
  o[kActionSize + 1] = u(-180.0, 180.0);      // Dash Angle
  o[kActionSize + 2] = u(-180.0, 180.0);      // Turn Angle
  o[kActionSize + 3] = u(-180.0, 180.0);      // Tackle Angle
  o[kActionSize + 4] = u(0.0, 100.0);         // Kick Power
  o[kActionSize + 5] = u(-180.0, 180.0);      // Kick Angle
  return o;
}

ActorOutput DQN::SelectAction(const InputStates& last_states, const double epsilon) {
  return SelectActions(std::vector<InputStates>{{last_states}}, epsilon)[0];
}

std::vector<ActorOutput> DQN::SelectActions(const std::vector<InputStates>& states_batch, const double epsilon) {
  CHECK(epsilon >= 0.0 && epsilon <= 1.0);
  SubmitPending();
  // :699 CHECK_LE(states_batch.size(), kMinibatchSize): the MemoryData layer is that wide there; here the cap is kept as the
  // reference's behaviour with this learner's minibatch, and -select_actions_cap widens it (the device path takes any n)
  const int cap = FLAGS_select_actions_cap == 0 ? minibatch_ : FLAGS_select_actions_cap;
  if (cap >= 0) CHECK_LE((int)states_batch.size(), cap);
  std::vector<ActorOutput> out(states_batch.size());
  if (std::uniform_real_distribution<double>(0.0, 1.0)(random_engine) < epsilon) {      // ONE draw per call (:700)
    for (auto& o : out) o = GetRandomActorOutput();
    return out;
  }
  if (states_batch.empty()) return out;
  std::vector<float> s(states_batch.size() * (size_t)state_size_);
  for (size_t n = 0; n < states_batch.size(); ++n) {
    const StateDataSp& sp = states_batch[n][0];
    CHECK(sp) << "null state";
    CHECK_EQ((int)sp->size(), state_size_);
    std::copy(sp->begin(), sp->end(), s.begin() + n * state_size_);
  }
  DQNHIP_CK(dqnhip_select_actions(h_, s.data(), (int)states_batch.size(), out[0].data()));
  if (FLAGS_explore_noise_sigma > 0.0) {
    dqnhip_noise_config nc;
    DQNHIP_CK(dqnhip_noise_default_config(&nc, DQNHIP_NOISE_EXPLORE));
    nc.sigma_params = (float)FLAGS_explore_noise_sigma; nc.theta = (float)FLAGS_explore_noise_theta; nc.seed = explore_seed_;
    if (explore_ou_.size() < out.size() * out[0].size()) explore_ou_.resize(out.size() * out[0].size(), 0.f);
    for (size_t n = 0; n < out.size(); ++n) DQNHIP_CK(dqnhip_noise_explore_host(&nc, explore_calls_, (int)n, &explore_ou_[n * out[0].size()], out[n].data()));
    explore_calls_ += 1;
  }
  return out;
}

Action DQN::SampleAction(const ActorOutput& actor_output) {
  const float dash = std::max(0., actor_output[DASH] + 1.0), turn = std::max(0., actor_output[TURN] + 1.0);
  const float kick = std::max(0., actor_output[KICK] + 1.0);
  std::discrete_distribution<int> dist{dash, turn, 0 /* tackle removed */, kick};
  const action_t act = (action_t)dist(random_engine);
  const int o1 = GetParamOffset(act, 0), o2 = GetParamOffset(act, 1);
  CHECK_GE(o1, 0);
  Action a;
  a.action = act;
  a.arg1 = actor_output[kActionSize + o1];
  a.arg2 = o2 < 0 ? 0 : actor_output[kActionSize + o2];
  return a;
}

float DQN::EvaluateAction(const InputStates& input_states, const ActorOutput& action) {
  SubmitPending();
  float q = 0;
  DQNHIP_CK(dqnhip_critic_forward(h_, DQNHIP_CRITIC, input_states[0]->data(), action.data(), 1, &q));
  return q;
}

void DQN::AddTransition(const Transition& t) {
  SubmitPending();
  const auto& next = std::get<4>(t);
  DQNHIP_CK(dqnhip_add_transition(h_, std::get<0>(t)[0]->data(), std::get<1>(t).data(), std::get<2>(t), std::get<3>(t),
                                  next ? (*next)->data() : nullptr, next ? 0 : 1));
}

void DQN::AddTransitions(const std::vector<Transition>& ts) {
  SubmitPending();
  const size_t n = ts.size(), S = (size_t)state_size_;
  if (n == 0) { DQNHIP_CK(dqnhip_add_transitions(h_, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0)); return; }   // (:776 still evicts one from a full deque)
  std::vector<float> s(n * S), nx(n * S, 0.f), a(n * (kActionSize + kActionParamSize)), r(n), mc(n);
  std::vector<uint8_t> term(n);
  for (size_t i = 0; i < n; ++i) {
    const Transition& t = ts[i];
    std::copy(std::get<0>(t)[0]->begin(), std::get<0>(t)[0]->end(), s.begin() + i * S);
    std::copy(std::get<1>(t).begin(), std::get<1>(t).end(), a.begin() + i * (kActionSize + kActionParamSize));
    r[i] = std::get<2>(t); mc[i] = std::get<3>(t);
    const auto& next = std::get<4>(t);
    term[i] = next ? 0 : 1;                                  // terminal <=> next_state is none (:878)
    if (next) std::copy((*next)->begin(), (*next)->end(), nx.begin() + i * S);
  }
  DQNHIP_CK(dqnhip_add_transitions(h_, s.data(), a.data(), r.data(), mc.data(), nx.data(), term.data(), (int)n));
}

void DQN::LabelTransitions(std::vector<Transition>& ts) {
  CHECK_GT(ts.size(), 0u) << "Need at least one transition to label.";
  std::fill(explore_ou_.begin(), explore_ou_.end(), 0.f);       // the episode is over: -explore_noise_sigma starts the next one from zero
  std::vector<float> r(ts.size()), mc(ts.size());
  for (size_t i = 0; i < ts.size(); ++i) r[i] = std::get<2>(ts[i]);
  DQNHIP_CK(dqnhip_label_transitions(gamma_, r.data(), (int)ts.size(), mc.data()));
  for (size_t i = 0; i < ts.size(); ++i) std::get<3>(ts[i]) = mc[i];
}

void DQN::Update() {
  SyncReplicasIfPending();       // (before the gates below: they read the iteration counters the broadcast carries)
  // data parallel: every rank's iteration counters advance together, so every rank stops updating at the same update — the
  // driver's own loops only look at max_iter() between bursts of Update() calls (src/dqn_main.cpp:354-362), and a rank left
  // alone in a collective would wait for ever
  if (dp_ && actor_solver_param_.max_iter() > 0 && max_iter() >= actor_solver_param_.max_iter()) return;
  if (memory_size() < FLAGS_memory_threshold) return;
  if (deferred_) {
    if (pend_n_ == 0 && uncollected_ == 0) { book_actor_iter_ = actor_iter(); book_critic_iter_ = critic_iter(); }
    const std::vector<int> idx = SampleTransitionsFromMemory(minibatch_);      // the draw, where the blocking form draws
    pend_idx_.resize((size_t)kSubmitEvery * minibatch_);
    std::copy(idx.begin(), idx.end(), pend_idx_.begin() + (size_t)pend_n_ * minibatch_);
    pend_n_ += 1;
    const int c = critic_iter(), a = actor_iter();                             // this update's numbers
    const bool due = c % FLAGS_loss_display_iter == 0 || a % FLAGS_loss_display_iter == 0 ||
                     c >= last_snapshot_iter_ + FLAGS_snapshot_freq || a >= last_snapshot_iter_ + FLAGS_snapshot_freq ||
                     (FLAGS_debug_info_iter > 0 && c % FLAGS_debug_info_iter == 0) ||      // (the diagnostics describe the last update run)
                     (FLAGS_evaluate_memory_freq > 0 && c % FLAGS_evaluate_memory_freq == 0) ||      // (the sweep sees the nets this update left)
                     pend_n_ + uncollected_ >= kMaxUncollected;
    if (due) CollectDeferred();              // (the last replayed Bookkeep is this update's: it logs / snapshots)
    else if (pend_n_ == kSubmitEvery) SubmitPending();
    return;
  }
  const std::pair<float, float> res = UpdateActorCritic();
  Bookkeep(res, critic_iter(), actor_iter());
}

// -debug_info_iter: one dqnhip_diag_collect, logged (INTEGRATION.md lists the lines).  Means are sum_abs / count.
static void LogDiagnostics(dqnhip_handle h, int tid) {
  std::unique_ptr<dqnhip_diag_report> rp(new dqnhip_diag_report);
  dqnhip_diag_report& r = *rp;
  r.struct_size = (int32_t)sizeof r;
  DQNHIP_CK(dqnhip_diag_collect(h, &r));
  const int L = r.n_panels / 5;
  auto mean = [](const dqnhip_diag_moments& m) { return m.count > 0 ? m.sum_abs / (double)m.count : 0.0; };
  auto layer_name = [&](int net, int layer) -> std::string {
    if (layer < L) return "ip" + std::to_string(layer + 1) + "_layer";
    if (net == DQNHIP_CRITIC) return "q_values_layer";
    return layer == L ? "action_layer" : "actionpara_layer";
  };
  static const char* const kPass[5] = {"actor_target(s')", "actor(s)", "critic_target(s',mu'(s'))", "critic(s,a)", "critic(s,mu(s))"};
  const std::string p = "[Agent" + std::to_string(tid) + "] [Diag] ";
  long long nonfinite = 0;
  for (int b = 0; b < r.n_blobs; ++b) nonfinite += r.blobs[b].w.n_nonfinite + r.blobs[b].g.n_nonfinite;
  LOG(INFO) << p << "iter " << r.critic_iter << ": grad_norm actor = " << r.grad_norm[0] << " (clip x" << r.clip_scale[0] << "), critic = "
            << r.grad_norm[1] << " (clip x" << r.clip_scale[1] << "), non-finite w/g = " << nonfinite;
  for (int b = 0; b < r.n_blobs; ++b) {
    const dqnhip_diag_blob& x = r.blobs[b];
    LOG(INFO) << p << "[Update] " << (x.net == DQNHIP_ACTOR ? "actor " : "critic ") << layer_name(x.net, x.layer) << (x.is_bias ? " bias" : " weight")
              << ": |w| = " << mean(x.w) << ", |g| = " << mean(x.g) << ", |step| = " << mean(x.step) << ", |lag| = " << mean(x.lag);
  }
  for (int q = 0; q < r.n_panels; ++q) {
    const dqnhip_diag_panel& x = r.panels[q];
    LOG(INFO) << p << "[Forward] " << kPass[x.pass] << " ip" << x.layer << "_layer: |a| = " << mean(x.a) << ", leaky = "
              << (x.a.count > 0 ? (double)x.n_negative / (double)x.a.count : 0.0) << ", dead = " << x.dead_units << " / " << x.cols;
  }
  const double B = r.panels[0].rows > 0 ? (double)r.panels[0].rows : 1.0;
  auto row = [&](const dqnhip_diag_row& x) {
    std::ostringstream s; s << "[" << x.min << ", " << x.max << "] mean " << x.sum / B; return s.str();
  };
  LOG(INFO) << p << "[Q] q_target " << row(r.q_target) << ", y " << row(r.y) << ", q_train " << row(r.q_train) << ", q_policy " << row(r.q_policy)
            << ", td " << row(r.td) << " rms " << std::sqrt(r.td.sum_sq / B) << ", terminal = " << r.n_terminal << " / " << (long long)B
            << ", non-finite = " << (r.q_target.n_nonfinite + r.y.n_nonfinite + r.q_train.n_nonfinite + r.q_policy.n_nonfinite);
  std::ostringstream a;
  long long oob = 0;
  for (int j = 0; j < DQNHIP_ACTOR_OUT; ++j) { oob += r.actor_out[j].n_out_of_bounds; a << (j ? " " : "") << r.actor_out[j].sum / B; }
  LOG(INFO) << p << "[Action] mean actor_out = " << a.str() << ", out of bounds = " << oob << " / " << (long long)(B * DQNHIP_ACTOR_OUT)
            << ", |dq_da| = " << r.dq_da_sum_abs / (B * DQNHIP_ACTOR_OUT) << " (max " << r.dq_da_max_abs << ")";
}

// -evaluate_memory_freq / -per_refresh_on_load: one line from a replay sweep's report.  Means are sum / n.
static void LogMemorySweep(const dqnhip_sweep_report& r, int tid, const char* what) {
  const double n = r.n > 0 ? (double)r.n : 1.0;
  LOG(INFO) << "[Agent" << tid << "] [Memory] " << what << " iter " << r.critic_iter << ": td mean " << r.td.sum / n << " rms " << std::sqrt(r.td.sum_sq / n)
            << ", q " << r.q.sum / n << ", y " << r.y.sum / n << ", q_policy " << r.q_policy.sum / n << ", q - mc " << r.q_minus_mc.sum / n
            << ", action match = " << (double)r.n_action_match / n << ", n = " << r.n;
}

// src/dqn.cpp:806-825 behind UpdateActorCritic(), on the iteration numbers that update left
void DQN::Bookkeep(const std::pair<float, float>& res, int critic_it, int actor_it) {
  if (critic_it % FLAGS_loss_display_iter == 0) {
    LOG(INFO) << "[Agent" << tid_ << "] Critic Iteration " << critic_it << ", loss = " << smoothed_critic_loss_;
    smoothed_critic_loss_ = 0;
  }
  smoothed_critic_loss_ += res.first / float(FLAGS_loss_display_iter);
  if (actor_it % FLAGS_loss_display_iter == 0) {
    LOG(INFO) << "[Agent" << tid_ << "] Actor Iteration " << actor_it << ", avg_q_value = " << smoothed_actor_loss_;
    smoothed_actor_loss_ = 0;
  }
  smoothed_actor_loss_ += res.second / float(FLAGS_loss_display_iter);
  // -dynamic_loss_scale: where the multipliers stand, at the same cadence (deferred updates: as of the collection that replays this update)
  if (FLAGS_dynamic_loss_scale && critic_it % FLAGS_loss_display_iter == 0) {
    dqnhip_loss_scale_state ls;
    DQNHIP_CK(dqnhip_get_loss_scale(h_, &ls));
    LOG(INFO) << "[Agent" << tid_ << "] Loss scale: critic x" << ls.mult_critic << ", actor x" << ls.mult_actor << ", skipped steps = " << ls.skipped_steps;
  }
  // -debug_info_iter: the diagnostics of this update (deferred updates: Update() made the collection due at this update, so the
  // replayed Bookkeep that gets here is the last update's and the device still holds what it left)
  if (FLAGS_debug_info_iter > 0 && critic_it % FLAGS_debug_info_iter == 0) LogDiagnostics(h_, tid_);
  // -evaluate_memory_freq: behind the loss lines and the diagnostics (a sweep overwrites the row buffers they are collected from).  Deferred
  // updates: as for the diagnostics, the replayed Bookkeep that gets here is the last update's — everything pending has been run
  if (FLAGS_evaluate_memory_freq > 0 && critic_it % FLAGS_evaluate_memory_freq == 0) {
    dqnhip_sweep_report r;
    r.struct_size = (int32_t)sizeof r;
    DQNHIP_CK(dqnhip_evaluate_memory(h_, 0, -1, &r, nullptr));
    LogMemorySweep(r, tid_, "evaluated at");
  }
  if (critic_it >= last_snapshot_iter_ + FLAGS_snapshot_freq || actor_it >= last_snapshot_iter_ + FLAGS_snapshot_freq) {
    snapshot_from_update_ = true;
    Snapshot();
    snapshot_from_update_ = false;
    last_snapshot_iter_ = max_iter();
  }
}

std::vector<int> DQN::SampleTransitionsFromMemory(int n) {
  std::vector<int> idx(n);
  const int size = memory_size();
  for (int& i : idx) i = std::uniform_int_distribution<int>(0, size - 1)(random_engine);
  return idx;
}

std::vector<InputStates> DQN::SampleStatesFromMemory(int n) {
  SubmitPending();
  const std::vector<int> idx = SampleTransitionsFromMemory(n);
  std::vector<float> flat((size_t)n * state_size_);
  DQNHIP_CK(dqnhip_sample_states(h_, idx.data(), n, flat.data()));
  std::vector<InputStates> out(n);
  for (int i = 0; i < n; ++i)
    out[i][0] = std::make_shared<StateData>(flat.begin() + (size_t)i * state_size_, flat.begin() + (size_t)(i + 1) * state_size_);
  return out;
}

std::pair<float, float> DQN::UpdateActorCritic() {
  CollectDeferred();
  SyncReplicasIfPending();
  // -prioritized_replay: the indices come from the device's sum tree — random_engine is not drawn from for sampling
  if (FLAGS_device_sampling || FLAGS_prioritized_replay) {
    float loss = 0, avgq = 0;
    if (dp_) { DQNHIP_CK(dqnhip_dp_update(h_, nullptr)); DQNHIP_CK(dqnhip_read_stats(h_, &loss, &avgq)); }
    else DQNHIP_CK(dqnhip_update(h_, nullptr, &loss, &avgq));                 // CHECK(isfinite(target / loss)): the call fails
    return std::make_pair(loss, avgq);
  }
  // (-n_step: the unchained call on the host-drawn indices — random_engine advances as the reference's does)
  if (dp_ || FLAGS_pipelined_stats || !FLAGS_chained_updates || FLAGS_n_step > 1 || FLAGS_target_noise_sigma > 0.0) return UpdateActorCritic(SampleTransitionsFromMemory(minibatch_));
  // The driver calls this in bursts (src/dqn_main.cpp:359-361), each call drawing its indices from random_engine (:501-509).  What the
  // NEXT call will draw is known now — unless something else draws from the engine or the memory changes in between: take it from a
  // COPY of the engine and hand it to the library as a prediction (dqnhip_update_chained: the next update's gather and first layers
  // ride in this update's optimiser launches).  The next call adopts the copy's state only if the engine and the memory size are
  // exactly as the prediction left them; otherwise it draws afresh.  Either way random_engine advances as the reference's does.
  const int size = memory_size();
  std::vector<int> idx;
  if (spec_valid_ && size == spec_size_ && random_engine == spec_before_) { idx.swap(spec_idx_); random_engine = spec_after_; }
  else idx = SampleTransitionsFromMemory(minibatch_);
  spec_before_ = random_engine;
  spec_after_ = random_engine;
  spec_idx_.resize(minibatch_);
  for (int& i : spec_idx_) i = std::uniform_int_distribution<int>(0, size - 1)(spec_after_);
  spec_size_ = size; spec_valid_ = true;
  float loss = 0, avgq = 0;
  DQNHIP_CK(dqnhip_update_chained(h_, reinterpret_cast<const int32_t*>(idx.data()), reinterpret_cast<const int32_t*>(spec_idx_.data()), &loss, &avgq));
  return std::make_pair(loss, avgq);
}

std::pair<float, float> DQN::UpdateActorCritic(const std::vector<int>& transitions) {
  CHECK_EQ((int)transitions.size(), minibatch_);
  CollectDeferred();
  SyncReplicasIfPending();
  float loss = 0, avgq = 0;
  static_assert(sizeof(int) == sizeof(int32_t), "indices travel as int32");
  if (dp_) {   // this rank's rows of the global minibatch: phase 0 / all-reduce / phase 1 / all-reduce / phase 2 inside the library
    DQNHIP_CK(dqnhip_dp_update(h_, reinterpret_cast<const int32_t*>(transitions.data())));
    DQNHIP_CK(dqnhip_read_stats(h_, &loss, &avgq));
  } else if (FLAGS_pipelined_stats) DQNHIP_CK(dqnhip_update_pipelined(h_, reinterpret_cast<const int32_t*>(transitions.data()), &loss, &avgq));
  else DQNHIP_CK(dqnhip_update(h_, reinterpret_cast<const int32_t*>(transitions.data()), &loss, &avgq));
  return std::make_pair(loss, avgq);
}

void DQN::ClearReplayMemory() { SubmitPending(); DQNHIP_CK(dqnhip_clear_memory(h_)); }
int DQN::memory_size() const { int32_t n = 0; DQNHIP_CK(dqnhip_memory_size(h_, &n)); return n; }
int DQN::critic_iter() const { int32_t a = 0, c = 0; DQNHIP_CK(dqnhip_get_iters(h_, &a, &c)); return c + pend_n_; }     // (+ drawn, not yet submitted: -deferred_updates)
int DQN::actor_iter() const { int32_t a = 0, c = 0; DQNHIP_CK(dqnhip_get_iters(h_, &a, &c)); return a + pend_n_; }

// (sharing, either side: the driver's global mutex orders one agent's update burst against another agent's writes, and an update
// that ran after the mutex was released would see a different ring - deferral is off for both objects from here on)
void DQN::ShareParameters(DQN& other, int num_actor_layers_to_share, int num_critic_layers_to_share) {
  StopDeferring(); other.StopDeferring();
  DQNHIP_CK(dqnhip_share_parameters(h_, other.h_, num_actor_layers_to_share, num_critic_layers_to_share));
}
// src/dqn.cpp:1037-1045 shares the blobs of two caffe::Layer objects; the nets here are parameter arenas
// in HBM without Layer objects, and the one caller (ShareParameters) is implemented on arena prefixes
void DQN::ShareLayer(caffe::Layer<float>&, caffe::Layer<float>&) {
  LOG(FATAL) << "DQN::ShareLayer: no caffe::Layer objects exist behind this DQN; use ShareParameters(other, n_actor, n_critic)";
}
void DQN::ShareReplayMemory(DQN& other) {
  // (see the constructor: a shared replay puts the driver's global MTX around collectives of two independent groups)
  CHECK(!dp_ && !other.dp_) << "ShareReplayMemory cannot be combined with -dp_rendezvous: the driver holds one mutex around every agent's "
                            << "Update() burst (src/dqn_main.cpp:358-362) and each agent's updates are collectives of its own group";
  StopDeferring(); other.StopDeferring();
  DQNHIP_CK(dqnhip_share_replay_memory(h_, other.h_));
}

}  // namespace dqn
