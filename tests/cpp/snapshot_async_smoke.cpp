// Drives include/dqn.hpp's `dqn::DQN` the way src/dqn_main.cpp does around its snapshots, for the -snapshot_async flag
// (tests/test_cpp_snapshot_async.py; the scheme of state_smoke.cpp): a run fills the memory from a fixed environment stream and calls
// Update() until max_iter() reaches -stop_at, snapshotting every -snapshot_freq updates on the way; with -resume it first goes through
// the driver's own sequence (src/dqn_main.cpp:213-220, 268-286: FindLatestSnapshot, RestoreActorSolver, RestoreCriticSolver,
// LoadReplayMemory) instead of filling.  The learner is destroyed before the digest is printed, so a snapshot in flight has been
// joined by then.  Built like per_smoke (g++ against libdqnhip.so and include/shim/).
#include <cstdio>

#include <gflags/gflags.h>

#include "dqn.hpp"

using namespace hfo;

DEFINE_string(prefix, "/tmp/dqnhip_snapshot_async_smoke_agent0", "save path of the learner (snapshot prefix)");
DEFINE_int32(stop_at, 40, "call Update() until max_iter() reaches this");
DEFINE_bool(resume, false, "restore the latest snapshot of -prefix instead of filling the memory");

int main(int argc, char** argv) {
  gflags::ParseCommandLineFlags(&argc, &argv, true);     // the learner flags are defined by dqn_dropin.cpp
  caffe::Caffe::set_mode(caffe::Caffe::GPU);
  const int num_features = 58;
  caffe::SolverParameter actor_sp, critic_sp;
  const int widths[2] = {128, 128};
  caffe::NetParameter an = dqn::CreateActorNet(num_features), cn = dqn::CreateCriticNet(num_features);
  for (caffe::NetParameter* np : {&an, &cn}) {
    int k = 0;
    for (int i = 0; i < np->layer_size(); ++i)
      if (np->layer(i).type() == "InnerProduct" && np->layer(i).name().rfind("ip", 0) == 0 && k < 4)
        np->mutable_layer(i)->mutable_inner_product_param()->set_num_output(widths[k++ % 2]);
  }
  actor_sp.mutable_net_param()->CopyFrom(an); critic_sp.mutable_net_param()->CopyFrom(cn);
  for (caffe::SolverParameter* sp : {&actor_sp, &critic_sp}) {
    sp->set_type("Adam"); sp->set_momentum(.95f); sp->set_momentum2(.999f); sp->set_clip_gradients(10); sp->set_lr_policy("fixed");
  }
  actor_sp.set_base_lr(1e-5f); critic_sp.set_base_lr(1e-3f);
  char digest[160] = "";
  {
    dqn::DQN dqn(actor_sp, critic_sp, FLAGS_prefix, num_features, 0);
    if (FLAGS_resume) {
      std::string actor, critic, memory;
      dqn::FindLatestSnapshot(FLAGS_prefix, actor, critic, memory);
      if (actor.empty() || critic.empty()) { std::printf("no snapshot under %s\n", FLAGS_prefix.c_str()); return 3; }
      dqn.RestoreActorSolver(actor);
      dqn.RestoreCriticSolver(critic);
      if (!memory.empty()) dqn.LoadReplayMemory(memory);
    } else {
      std::mt19937 env(1);
      std::uniform_real_distribution<float> U(-1.f, 1.f);
      auto fresh = [&]() { auto s = std::make_shared<dqn::StateData>(num_features); for (auto& v : *s) v = U(env); return s; };
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
      }
    }
    for (int guard = 0; dqn.max_iter() < FLAGS_stop_at && guard < 1000; ++guard) dqn.Update();
    uint64_t hash = 1469598103934665603ull;                // FNV-1a over the dense parameters of the four nets
    for (int net = 0; net < 4; ++net) {
      size_t n = 0;
      if (dqnhip_param_count(dqn.handle(), net, &n) != 0) return 4;
      std::vector<float> w(n);
      if (dqnhip_get_params(dqn.handle(), net, DQNHIP_KIND_W, w.data(), n) != 0) return 4;
      const unsigned char* p = reinterpret_cast<const unsigned char*>(w.data());
      for (size_t i = 0; i < n * sizeof(float); ++i) { hash ^= p[i]; hash *= 1099511628211ull; }
    }
    std::snprintf(digest, sizeof digest, "digest: nets %016llx actor_iter %d critic_iter %d memory_size %d", (unsigned long long)hash, dqn.actor_iter(),
                  dqn.critic_iter(), dqn.memory_size());
  }
  std::printf("%s\n", digest);
  std::printf("snapshot async smoke OK\n");
  return 0;
}
