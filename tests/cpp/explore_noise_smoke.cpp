// Drives include/dqn.hpp's `dqn::DQN` through two episodes of greedy SelectAction calls for the -explore_noise_sigma / -explore_noise_theta
// flags: tests/test_cpp_explore_noise.py runs it with the flags off and on and compares the printed ActorOutputs (as float32 bit
// patterns) with tests/noise_ref.py applied to the flag-off run's outputs.  No update runs, so the nets stay what the seed made them
// and both runs see the same greedy outputs.  Built like nstep_smoke (g++ against libdqnhip.so and include/shim/).
#include <cstdio>
#include <cstring>

#include <gflags/gflags.h>

#include "dqn.hpp"

using namespace hfo;

DEFINE_string(prefix, "/tmp/dqnhip_explore_noise_smoke_agent0", "save path of the learner (snapshot prefix)");

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
      const int len = 6;
      for (int t = 0; t < len; ++t) {
        dqn::InputStates in = {{state}};
        // epsilon 0: every call is greedy; the one epsilon draw per call is made all the same
        dqn::ActorOutput ao = dqn.SelectAction(in, 0.0);
        std::printf("ao %d %d", episode, t);
        for (float v : ao) { unsigned u; std::memcpy(&u, &v, 4); std::printf(" %08x", u); }
        std::printf("\n");
        auto next = fresh();
        if (t + 1 < len) ep.emplace_back(in, ao, 0.1f, 0.f, next);
        else ep.emplace_back(in, ao, 1.f, 0.f, boost::none);
        state = next;
      }
      dqn.LabelTransitions(ep);        // resets the noise state
      dqn.AddTransitions(ep);
    }
    // the engine's call order is the reference's with the flags on or off: the next random output is the same
    dqn::ActorOutput r = dqn.SelectAction({{fresh()}}, 1.0);
    std::printf("random");
    for (float v : r) { unsigned u; std::memcpy(&u, &v, 4); std::printf(" %08x", u); }
    std::printf("\n");
  }
  std::printf("explore noise smoke OK\n");
  return 0;
}
