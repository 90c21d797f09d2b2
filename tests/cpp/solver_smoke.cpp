// Drives include/dqn.hpp's `dqn::DQN` with the solver type of the reference driver's -solver flag (src/dqn_main.cpp:30: SolverParameter::
// set_type on both solvers, momentum from -momentum): 8 updates, Snapshot(), a second learner of the same type restored from the
// snapshot, 4 more updates on both — which must agree.  tests/test_cpp_solvers.py runs it per type and with the combinations Caffe's
// solver constructors refuse; those stop in the adaptor's constructor, before the device is touched.  Built like per_smoke.
#include <cstdio>

#include <gflags/gflags.h>

#include "dqn.hpp"

using namespace hfo;

DEFINE_string(prefix, "/tmp/dqnhip_solver_smoke_agent0", "save path of the learner (snapshot prefix)");
DEFINE_string(solver_type, "Adam", "SolverParameter.type of both solvers (the driver's -solver)");
DEFINE_double(solver_momentum, 0.95, "SolverParameter.momentum of both solvers (the driver's -momentum)");
DEFINE_double(solver_rms_decay, 0.99, "SolverParameter.rms_decay of both solvers");

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
    sp->set_type(FLAGS_solver_type); sp->set_momentum((float)FLAGS_solver_momentum); sp->set_momentum2(.999f); sp->set_clip_gradients(10);
    sp->set_lr_policy("fixed"); sp->set_rms_decay((float)FLAGS_solver_rms_decay);
  }
  actor_sp.set_base_lr(1e-5f); critic_sp.set_base_lr(1e-3f);
  std::mt19937 env(1);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  auto fresh = [&]() { auto s = std::make_shared<dqn::StateData>(num_features); for (auto& v : *s) v = U(env); return s; };
  auto probe = [&](dqn::DQN& d, const char* who) {
    std::mt19937 probe_rng(99);
    std::printf("%s: actor_iter %d critic_iter %d q:", who, d.actor_iter(), d.critic_iter());
    for (int p = 0; p < 4; ++p) {
      auto s = std::make_shared<dqn::StateData>(num_features);
      for (auto& v : *s) v = U(probe_rng);
      dqn::ActorOutput a;
      for (auto& v : a) v = U(probe_rng);
      std::printf(" %.9g", d.EvaluateAction({{s}}, a));
    }
    std::printf("\n");
  };
  {
    dqn::DQN dqn(actor_sp, critic_sp, FLAGS_prefix, num_features, 0);
    std::vector<dqn::Transition> ep;
    auto state = fresh();
    const int len = 120;
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
    for (int i = 0; i < 8; ++i) dqn.Update();
    dqn.Snapshot(FLAGS_prefix + "_snap", false, true);
    probe(dqn, "trained");
    std::string as, cs, ms;
    dqn::FindLatestSnapshot(FLAGS_prefix + "_snap", as, cs, ms);
    if (as.empty() || cs.empty() || ms.empty()) { std::printf("no snapshot found\n"); return 1; }
    dqn::DQN again(actor_sp, critic_sp, FLAGS_prefix + "_again", num_features, 0);
    again.RestoreActorSolver(as); again.RestoreCriticSolver(cs); again.LoadReplayMemory(ms);
    probe(again, "restored");
    for (int i = 0; i < 4; ++i) { dqn.Update(); again.Update(); }
    probe(dqn, "trained+4");
    probe(again, "restored+4");
  }
  std::printf("solver smoke OK\n");
  return 0;
}
