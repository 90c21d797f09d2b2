// Drives include/dqn.hpp's `dqn::DQN` through long bursts of Update() between episodes, the way src/dqn_main.cpp does under
// -learn_offline (:340-343) or after a long episode (:357-363): bursts of 40 updates, so that -deferred_updates submits whole
// sixteen-update graphs, with a snapshot (-snapshot_freq 25) and the log cadence (-loss_display_iter 7) falling inside them, then
// DQN::Benchmark and one more short burst.  Prints
// a digest of everything the driver could observe afterwards; tests/test_gpu_deferred_adaptor.py runs it with the flag on and off
// and compares.  Built like adaptor_smoke (g++ against libdqnhip.so and include/shim/); run only on the GPU box.
#include <algorithm>
#include <cstdio>

#include <gflags/gflags.h>

#include "dqn.hpp"

using namespace hfo;

DEFINE_string(prefix, "/tmp/dqnhip_deferred_smoke_agent0", "save path of the learner (snapshot prefix)");

int main(int argc, char** argv) {
  gflags::ParseCommandLineFlags(&argc, &argv, true);     // the learner flags are defined by dqn_dropin.cpp
  caffe::Caffe::set_mode(caffe::Caffe::GPU);
  const int num_features = 59;
  caffe::SolverParameter actor_sp, critic_sp;
  const int widths[4] = {128, 64, 64, 64};
  caffe::NetParameter an = dqn::CreateActorNet(num_features), cn = dqn::CreateCriticNet(num_features);
  for (caffe::NetParameter* np : {&an, &cn})
    for (int i = 0, k = 0; i < np->layer_size(); ++i)
      if (np->layer(i).type() == "InnerProduct" && np->layer(i).name().rfind("ip", 0) == 0)
        np->mutable_layer(i)->mutable_inner_product_param()->set_num_output(widths[k++]);
  actor_sp.mutable_net_param()->CopyFrom(an); critic_sp.mutable_net_param()->CopyFrom(cn);
  for (caffe::SolverParameter* sp : {&actor_sp, &critic_sp}) {
    sp->set_type("Adam"); sp->set_momentum(.95f); sp->set_momentum2(.999f); sp->set_clip_gradients(10); sp->set_lr_policy("fixed");
  }
  actor_sp.set_base_lr(1e-5f); critic_sp.set_base_lr(1e-3f);
  dqn::RemoveFilesMatchingRegexp(FLAGS_prefix + "_.*");
  std::mt19937 env(1);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  auto fresh = [&]() { auto s = std::make_shared<dqn::StateData>(num_features); for (auto& v : *s) v = U(env); return s; };
  {
    dqn::DQN dqn(actor_sp, critic_sp, FLAGS_prefix, num_features, 0);
    int bursts_seen = 0;
    for (int episode = 0; episode < 5; ++episode) {
      std::vector<dqn::Transition> ep;
      auto state = fresh();
      const int len = 60;
      for (int t = 0; t < len; ++t) {
        dqn::InputStates in = {{state}};
        dqn::ActorOutput ao = dqn.SelectAction(in, 0.5);
        auto next = fresh();
        const float reward = 0.1f * U(env);
        if (t + 1 < len) ep.emplace_back(in, ao, reward, 0.f, next);
        else ep.emplace_back(in, ao, reward + 5.f, 0.f, boost::none);
        state = next;
      }
      dqn.LabelTransitions(ep);
      dqn.AddTransitions(ep);
      const int before = dqn.max_iter();
      for (int i = 0; i < 40; ++i) dqn.Update();
      // (what the driver reads between bursts: the pending updates count)
      if (dqn.max_iter() != before && dqn.max_iter() != before + 40) { std::fprintf(stderr, "max_iter %d after a burst from %d\n", dqn.max_iter(), before); return 2; }
      bursts_seen += dqn.max_iter() != before;
    }
    if (bursts_seen != 4) { std::fprintf(stderr, "%d bursts ran\n", bursts_seen); return 3; }
    // DQN::Benchmark (src/dqn.cpp:487-498; the driver's -benchmark, src/dqn_main.cpp:332-339) behind a burst, with updates still
    // outstanding when it starts: 40 updates (two whole graphs + 8) on the engine's next draws, no bookkeeping; then a short burst
    dqn.Benchmark(40);
    if (dqn.max_iter() != 200) { std::fprintf(stderr, "max_iter %d after Benchmark(40)\n", dqn.max_iter()); return 4; }
    for (int i = 0; i < 10; ++i) dqn.Update();
    std::printf("digest: actor_iter %d critic_iter %d memory_size %d\n", dqn.actor_iter(), dqn.critic_iter(), dqn.memory_size());
    std::mt19937 probe_rng(99);
    std::printf("q:");
    for (int p = 0; p < 8; ++p) {
      auto s = std::make_shared<dqn::StateData>(num_features);
      for (auto& v : *s) v = U(probe_rng);
      dqn::ActorOutput a;
      for (auto& v : a) v = U(probe_rng);
      std::printf(" %.9g", dqn.EvaluateAction({{s}}, a));
    }
    std::printf("\n");
    for (int p = 0; p < 4; ++p) {
      auto s = std::make_shared<dqn::StateData>(num_features);
      for (auto& v : *s) v = U(probe_rng);
      const dqn::ActorOutput o = dqn.SelectAction({{s}}, 0.0);
      std::printf("mu%d:", p);
      for (float v : o) std::printf(" %.9g", v);
      std::printf("\n");
    }
  }
  std::vector<std::string> files = dqn::FilesMatchingRegexp(FLAGS_prefix + "_.*");
  std::sort(files.begin(), files.end());
  for (const std::string& f : files) std::printf("file: %s\n", f.c_str());
  dqn::RemoveFilesMatchingRegexp(FLAGS_prefix + "_.*");
  std::printf("deferred smoke OK\n");
  return 0;
}
