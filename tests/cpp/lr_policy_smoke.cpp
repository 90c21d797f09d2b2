// The lr policy and the weight decay through the adaptor (include/dqn.hpp + dqn_dropin.cpp): the solver parameters are filled the way the
// reference's driver fills them (src/dqn_main.cpp:249-262: type, base_lr, lr_policy, max_iter, momentum, momentum2, clip_gradients on both),
// everything else the policy needs comes from the adaptor's flags (-lr_gamma, -lr_power, -lr_stepsize, -lr_stepvalues, -weight_decay,
// -regularization_type) or, with -sp_*, from the SolverParameter fields themselves.  Prints what reached the learner (dqnhip_get_config on
// the adaptor's handle, dqnhip_get_learning_rate) and, with -dir, trains on the files tests/test_cpp_lr_policy.py left there — weights, a
// replay memory, index vectors, all through the C calls on that handle — and leaves the four nets' weights for the test to compare with a
// Python learner of the same configuration.  A refused configuration aborts in the adaptor's constructor.  Built like solver_smoke.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include <gflags/gflags.h>

#include "dqn.hpp"

using namespace hfo;

DEFINE_string(prefix, "/tmp/dqnhip_lr_policy_smoke_agent0", "save path of the learner (snapshot prefix)");
DEFINE_string(solver_type, "Adam", "SolverParameter.type of both solvers (the driver's -solver)");
DEFINE_double(solver_momentum, 0.95, "SolverParameter.momentum of both solvers (the driver's -momentum)");
DEFINE_string(policy, "fixed", "SolverParameter.lr_policy of both solvers (the driver's -lr_policy)");
DEFINE_int32(solver_max_iter, 10000000, "SolverParameter.max_iter of both solvers (the driver's -max_iter)");
DEFINE_double(sp_gamma, 0, "SolverParameter.gamma of both solvers (the driver sets none)");
DEFINE_int32(sp_stepsize, 0, "SolverParameter.stepsize of both solvers");
DEFINE_double(sp_weight_decay, 0, "SolverParameter.weight_decay of both solvers");
DEFINE_double(sp_critic_gamma, -1, ">= 0: SolverParameter.gamma of the critic's solver alone (a disagreement)");
DEFINE_string(dir, "", "directory with w0..w3.bin, s.bin, a.bin, r.bin, mc.bin, nx.bin, term.bin, idx.bin; out0..out3.bin are written there");
DEFINE_int32(updates, 0, "-dir: updates to run (rows of idx.bin)");

template <class T>
static std::vector<T> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(raw.size() / sizeof(T));
  if (!v.empty()) memcpy(v.data(), raw.data(), v.size() * sizeof(T));
  return v;
}
#define CK(expr) do { if ((expr) != 0) { std::printf("FAILED %s: %s\n", #expr, dqnhip_last_error()); return 1; } } while (0)

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
    sp->set_max_iter(FLAGS_solver_max_iter); sp->set_type(FLAGS_solver_type); sp->set_lr_policy(FLAGS_policy);
    sp->set_momentum((float)FLAGS_solver_momentum); sp->set_momentum2(.999f); sp->set_clip_gradients(10);
    sp->set_gamma((float)FLAGS_sp_gamma); sp->set_stepsize(FLAGS_sp_stepsize); sp->set_weight_decay((float)FLAGS_sp_weight_decay);
  }
  if (FLAGS_sp_critic_gamma >= 0) critic_sp.set_gamma((float)FLAGS_sp_critic_gamma);
  actor_sp.set_base_lr(1e-5f); critic_sp.set_base_lr(1e-3f);
  {
    dqn::DQN dqn(actor_sp, critic_sp, FLAGS_prefix, num_features, 0);
    dqnhip_handle h = dqn.handle();
    dqnhip_config c;
    CK(dqnhip_get_config(h, &c));
    std::printf("config: lr_policy %s gamma %.9g power %.9g stepsize %d max_iter %d stepvalues", dqnhip_lr_policy_name(c.lr_policy), (double)c.lr_gamma,
                (double)c.lr_power, c.lr_stepsize, c.lr_max_iter);
    for (int i = 0; i < c.lr_n_stepvalue; ++i) std::printf("%s%d", i ? "," : " ", c.lr_stepvalue[i]);
    std::printf(" weight_decay %.9g regularization %s\n", (double)c.weight_decay, c.regularization_type == DQNHIP_REG_L1 ? "L1" : "L2");
    if (!FLAGS_dir.empty()) {
      const std::string d = FLAGS_dir + "/";
      for (int net = 0; net < 4; ++net) {
        const std::vector<float> w = slurp<float>(d + "w" + std::to_string(net) + ".bin");
        CK(dqnhip_set_params(h, net, DQNHIP_KIND_W, w.data(), w.size()));
      }
      const std::vector<float> s = slurp<float>(d + "s.bin"), a = slurp<float>(d + "a.bin"), r = slurp<float>(d + "r.bin"), mc = slurp<float>(d + "mc.bin"),
                               nx = slurp<float>(d + "nx.bin");
      const std::vector<uint8_t> term = slurp<uint8_t>(d + "term.bin");
      CK(dqnhip_add_transitions(h, s.data(), a.data(), r.data(), mc.data(), nx.data(), term.data(), (int32_t)r.size()));
      const std::vector<int32_t> idx = slurp<int32_t>(d + "idx.bin");
      const int B = dqn.minibatch_size();
      if ((int)idx.size() < FLAGS_updates * B) { std::printf("idx.bin holds %zu indices, %d needed\n", idx.size(), FLAGS_updates * B); return 1; }
      for (int u = 0; u < FLAGS_updates; ++u) {
        float rate[2], loss = 0, q = 0;
        CK(dqnhip_get_learning_rate(h, DQNHIP_ACTOR, &rate[0])); CK(dqnhip_get_learning_rate(h, DQNHIP_CRITIC, &rate[1]));
        CK(dqnhip_update(h, idx.data() + (size_t)u * B, &loss, &q));
        std::printf("update %d: rates %.9g %.9g loss %.9g avg_q %.9g\n", u, (double)rate[0], (double)rate[1], (double)loss, (double)q);
      }
      for (int net = 0; net < 4; ++net) {
        size_t n = 0;
        CK(dqnhip_param_count(h, net, &n));
        std::vector<float> w(n);
        CK(dqnhip_get_params(h, net, DQNHIP_KIND_W, w.data(), n));
        std::ofstream(d + "out" + std::to_string(net) + ".bin", std::ios::binary).write((const char*)w.data(), (std::streamsize)(n * sizeof(float)));
      }
    }
  }
  std::printf("lr policy smoke OK\n");
  return 0;
}
