// solver_kernels.hip.h — the optimiser launches of a learner whose solver is not Adam: k_solver_soft<SOLVER> and
// k_solver_soft_gather<SOLVER> (the twins of k_adam_soft / k_adam_soft_gather, small_kernels.hip.h; bodies: solver_bodies.hip.h) and
// the switch that launches them.  Five solvers x two kernels; learner.hip includes this and no other unit does (kernels are
// static: a unit that includes this embeds all ten).  No first-layer riders: plan_of gives these learners the schedule without them.
// Below them k_sched_soft<SOLVER> / k_sched_soft_gather<SOLVER>, six solvers x two kernels: the pass of a learner with an lr policy on
// another solver than Adam, or with a weight decay on any (sched_soft_body); the same schedule.
#pragma once
#include "../../include/dqnhip.h"
#include "solver_bodies.hip.h"

namespace dqnhip {

static_assert(kSolverAdam == DQNHIP_SOLVER_ADAM && kSolverSGD == DQNHIP_SOLVER_SGD && kSolverNesterov == DQNHIP_SOLVER_NESTEROV &&
              kSolverAdaGrad == DQNHIP_SOLVER_ADAGRAD && kSolverRMSProp == DQNHIP_SOLVER_RMSPROP && kSolverAdaDelta == DQNHIP_SOLVER_ADADELTA,
              "Solver mirrors dqnhip_solver");

// the pass in a launch of its own; block 0 runs the update's bookkeeping when it is the update's last launch (as k_adam_soft)
template <int SOLVER>
static __global__ __launch_bounds__(256) void k_solver_soft(AdamArgs a) {
  __shared__ float s[8];
  __shared__ double sq[4];
  solver_soft_body<SOLVER>(a, blockIdx.x, gridDim.x, s);
  if (a.tick_on && blockIdx.x == 0) {
    const bool skipped = s[7] == 1.0f;      // (2: dynamic loss scaling backed off — skipped, not reported)
    __syncthreads();
    tick_body(a.tick, s, sq, skipped);
  }
}

// the update's last launch inside a multi-update graph: the first g.blocks workgroups are the NEXT update's gather (as
// k_adam_soft_gather routes them; gather_block unchanged — the bias corrections it leaves in DevState are read by nobody here)
template <int SOLVER>
static __global__ __launch_bounds__(256) void k_solver_soft_gather(AdamArgs a, GatherArgs g) {
  const int b0 = adam_routed_block(a, (int)blockIdx.x, g.blocks);
  __shared__ float s[8];
  __shared__ double sq[4];
  if (b0 < g.blocks) { gather_block(g, b0); return; }
  const int blk = b0 - g.blocks;
  solver_soft_body<SOLVER>(a, blk, (int)gridDim.x - g.blocks, s);
  if (a.tick_on && blk == 0) {
    const bool skipped = s[7] == 1.0f;
    __syncthreads();
    tick_body(a.tick, s, sq, skipped);
  }
}

// blocks: the strided pass's workgroups; g: the next update's gather riding in front of them, or null
template <int SOLVER>
inline hipError_t solver_launch_as(const LaunchOn& on, int blocks, const AdamArgs& a, const GatherArgs* g) {
  if (g != nullptr) return launch(on, k_solver_soft_gather<SOLVER>, dim3(g->blocks + blocks), dim3(256), 0, a, *g);
  return launch(on, k_solver_soft<SOLVER>, dim3(blocks), dim3(256), 0, a);
}
inline hipError_t solver_launch(int solver, const LaunchOn& on, int blocks, const AdamArgs& a, const GatherArgs* g) {
  switch (solver) {
    case kSolverSGD: return solver_launch_as<kSolverSGD>(on, blocks, a, g);
    case kSolverNesterov: return solver_launch_as<kSolverNesterov>(on, blocks, a, g);
    case kSolverAdaGrad: return solver_launch_as<kSolverAdaGrad>(on, blocks, a, g);
    case kSolverRMSProp: return solver_launch_as<kSolverRMSProp>(on, blocks, a, g);
    case kSolverAdaDelta: return solver_launch_as<kSolverAdaDelta>(on, blocks, a, g);
    default: return hipErrorInvalidValue;
  }
}

// ---- k_sched_soft<SOLVER> / k_sched_soft_gather<SOLVER>: the pass of a learner with an lr policy or a weight decay (sched_soft_body) ----
// The twins of the two kernels above, for all six solvers; the decay and its kind are arguments of their own (AdamArgs keeps its layout).
template <int SOLVER>
static __global__ __launch_bounds__(256) void k_sched_soft(AdamArgs a, DecayArgs d) {
  __shared__ float s[8];
  __shared__ double sq[4];
  sched_soft_body<SOLVER>(a, d, blockIdx.x, gridDim.x, s);
  if (a.tick_on && blockIdx.x == 0) {
    const bool skipped = s[7] == 1.0f;
    __syncthreads();
    tick_body(a.tick, s, sq, skipped);
  }
}
template <int SOLVER>
static __global__ __launch_bounds__(256) void k_sched_soft_gather(AdamArgs a, DecayArgs d, GatherArgs g) {
  const int b0 = adam_routed_block(a, (int)blockIdx.x, g.blocks);
  __shared__ float s[8];
  __shared__ double sq[4];
  if (b0 < g.blocks) { gather_block(g, b0); return; }
  const int blk = b0 - g.blocks;
  sched_soft_body<SOLVER>(a, d, blk, (int)gridDim.x - g.blocks, s);
  if (a.tick_on && blk == 0) {
    const bool skipped = s[7] == 1.0f;
    __syncthreads();
    tick_body(a.tick, s, sq, skipped);
  }
}
template <int SOLVER>
inline hipError_t sched_launch_as(const LaunchOn& on, int blocks, const AdamArgs& a, const DecayArgs& d, const GatherArgs* g) {
  if (g != nullptr) return launch(on, k_sched_soft_gather<SOLVER>, dim3(g->blocks + blocks), dim3(256), 0, a, d, *g);
  return launch(on, k_sched_soft<SOLVER>, dim3(blocks), dim3(256), 0, a, d);
}
inline hipError_t sched_launch(int solver, const LaunchOn& on, int blocks, const AdamArgs& a, const DecayArgs& d, const GatherArgs* g) {
  switch (solver) {
    case kSolverAdam: return sched_launch_as<kSolverAdam>(on, blocks, a, d, g);
    case kSolverSGD: return sched_launch_as<kSolverSGD>(on, blocks, a, d, g);
    case kSolverNesterov: return sched_launch_as<kSolverNesterov>(on, blocks, a, d, g);
    case kSolverAdaGrad: return sched_launch_as<kSolverAdaGrad>(on, blocks, a, d, g);
    case kSolverRMSProp: return sched_launch_as<kSolverRMSProp>(on, blocks, a, d, g);
    case kSolverAdaDelta: return sched_launch_as<kSolverAdaDelta>(on, blocks, a, d, g);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dqnhip
