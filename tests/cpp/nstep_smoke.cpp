// Drives include/dqn.hpp's `dqn::DQN` through an episode loop with bursts of Update(), the way src/dqn_main.cpp does (:357-363), for
// the -n_step flag: tests/test_cpp_nstep.py runs it with the flag on and off (40 updates each) and compares the format of the log
// lines, and starts it with the flag combinations the adaptor CHECKs against — those stop in the constructor, before the device
// is touched.  With -reload_memory it also writes the replay memory to a file and loads it back, which -n_step_validate_on_load validates.
// Built like adaptor_smoke (g++ against libdqnhip.so and include/shim/).
#include <cstdio>

#include <gflags/gflags.h>

#include "dqn.hpp"

using namespace hfo;

DEFINE_string(prefix, "/tmp/dqnhip_nstep_smoke_agent0", "save path of the learner (snapshot prefix)");
DEFINE_bool(reload_memory, false, "after training: write the replay memory to a file, clear it and load it back (-n_step_validate_on_load then validates it)");

int main(int argc, char** argv) {
  gflags::ParseCommandLineFlags(&argc, &argv, true);     // the learner flags are defined by dqn_dropin.cpp
  caffe::Caffe::set_mode(caffe::Caffe::GPU);
  const int num_features = 59;
  caffe::SolverParameter actor_sp, critic_sp;
  const int widths[4] = {128, 128, 128, 128};
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
  std::mt19937 env(1);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  auto fresh = [&]() { auto s = std::make_shared<dqn::StateData>(num_features); for (auto& v : *s) v = U(env); return s; };
  {
    dqn::DQN dqn(actor_sp, critic_sp, FLAGS_prefix, num_features, 0);
    for (int episode = 0; episode < 2; ++episode) {
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
      for (int i = 0; i < 20; ++i) dqn.Update();
    }
    if (FLAGS_reload_memory) {
      const std::string f = FLAGS_prefix + "_nstep_smoke.replaymemory";
      dqn.SnapshotReplayMemory(f);
      dqn.ClearReplayMemory();
      dqn.LoadReplayMemory(f);
      std::remove(f.c_str());
    }
    std::printf("digest: actor_iter %d critic_iter %d memory_size %d\n", dqn.actor_iter(), dqn.critic_iter(), dqn.memory_size());
    std::mt19937 probe_rng(99);
    std::printf("q:");
    for (int p = 0; p < 4; ++p) {
      auto s = std::make_shared<dqn::StateData>(num_features);
      for (auto& v : *s) v = U(probe_rng);
      dqn::ActorOutput a;
      for (auto& v : a) v = U(probe_rng);
      std::printf(" %.9g", dqn.EvaluateAction({{s}}, a));
    }
    std::printf("\n");
  }
  std::printf("nstep smoke OK\n");
  return 0;
}
