// snapshot_codec.h — the Caffe snapshot's builders on host pointers (snapshot.cpp): what dqnhip_solver_snapshot assembles from
// dqnhip_get_params and the asynchronous snapshot's writer thread (learner_save_async.hip) from its staged copies, so both write the same
// bytes.  Nothing here touches a learner or the GPU.  Host code only; not installed, not part of the C-ABI.
#pragma once
#include <string>

#include "../../include/dqnhip.h"

namespace dqnhip_snap {

// net: DQNHIP_ACTOR or DQNHIP_CRITIC; the arrays are dense, in Caffe order (dqnhip_get_params)
size_t dense_count(const dqnhip_config& c, int net);
std::string caffemodel_bytes(const dqnhip_config& c, int net, const float* w);
// h2 is read only where the solver keeps two history blobs per parameter (Adam, AdaDelta)
std::string solverstate_bytes(const dqnhip_config& c, int net, int iter, const std::string& learned_net, const float* h1, const float* h2);
// Caffe's solvers that keep two history blobs per parameter (AdamSolver::AdamPreSolve, AdaDeltaSolver::AdaDeltaPreSolve)
bool two_histories(int solver_type);
// A snapshot's files.  [actor, critic], without the extension (.caffemodel / .solverstate): where the solvers write them
// (Solver::SnapshotFilename on save_path) and where DQN::Snapshot moves them (the prefix); the replay memory's file
struct Names { std::string from[2], to[2], memory; };
Names names_of(const std::string& save_path, const std::string& prefix, int actor_iter, int critic_iter);
// path + ".tmp", fsync, rename: a killed process leaves no partial file under `path`
int publish_file(const std::string& path, const std::string& data, std::string* err);
int move_file(const std::string& from, const std::string& to, std::string* err);
// DQN::Snapshot's removal of the older files of a prefix (src/dqn.cpp:612-618)
void remove_old_snapshots(const std::string& prefix, int actor_iter, int critic_iter);

}  // namespace dqnhip_snap
