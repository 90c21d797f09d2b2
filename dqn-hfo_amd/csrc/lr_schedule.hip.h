// lr_schedule.hip.h — Caffe's learning-rate policies (SGDSolver::GetLearningRate @2ef5847) as ONE function that the host
// and the device both compile: the scalars block of gather_block (update_bodies.hip.h) evaluates it per update from the iteration
// counters in DevState — a rate cannot be a kernel argument of a captured graph — and dqnhip_get_learning_rate evaluates the same
// text on the host.  Argument layer: plain structs and inline functions, no kernel.  Also compiles as plain C++
// (tests/cpp/lr_schedule_host.cpp).
// Stated deviations from Caffe: evaluated in double from the float32 parameters and rounded ONCE (Caffe: float powf), as
// adam_correction is; multistep is stateless (equal to Caffe's current_step_ walk for strictly increasing stepvalues, which are
// required); poly clamps its base at 0, so the rate is 0 from max_iter on (Caffe: NaN for a fractional power).
#pragma once
#include <math.h>
#include <stdio.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DQNHIP_HD __host__ __device__
#else
#define DQNHIP_HD
#endif

namespace dqnhip {

// = DQNHIP_LR_* (include/dqnhip.h; static_assert in learner_plan.hip)
enum LrPolicy { kLrFixed = 0, kLrStep = 1, kLrExp = 2, kLrInv = 3, kLrMultistep = 4, kLrPoly = 5, kLrSigmoid = 6, kLrPolicies = 7 };
constexpr int kLrMaxStepvalues = 16;
// = DQNHIP_REG_*
enum Regularization { kRegL2 = 0, kRegL1 = 1 };

struct LrSchedule {
  int policy;
  float base_lr[2];          // [actor, critic]
  float gamma, power;
  int stepsize, max_iter, n_stepvalue;
  int stepvalue[kLrMaxStepvalues];
};

inline const char* lr_policy_name(int policy) {
  static const char* const kNames[kLrPolicies] = {"fixed", "step", "exp", "inv", "multistep", "poly", "sigmoid"};
  return policy >= 0 && policy < kLrPolicies ? kNames[policy] : nullptr;
}

// Caffe's current_step_ as GetLearningRate leaves it at `iter` (step, multistep; 0 for the other policies): an exact integer
DQNHIP_HD inline int lr_current_step(const LrSchedule& s, int iter) {
  if (s.policy == kLrStep) return iter / s.stepsize;
  if (s.policy == kLrMultistep) {
    int k = 0;
    for (int i = 0; i < s.n_stepvalue && i < kLrMaxStepvalues; ++i) k += s.stepvalue[i] <= iter ? 1 : 0;
    return k;
  }
  return 0;
}

// the rate of net's step at solver iteration `iter` (iter_ BEFORE the increment: GetLearningRate runs inside ApplyUpdate)
DQNHIP_HD inline float lr_rate(const LrSchedule& s, int net, int iter) {
  const double base = (double)s.base_lr[net], gamma = (double)s.gamma, power = (double)s.power, it = (double)iter;
  switch (s.policy) {
    case kLrStep:
    case kLrMultistep: return (float)(base * pow(gamma, (double)lr_current_step(s, iter)));
    case kLrExp: return (float)(base * pow(gamma, it));
    case kLrInv: return (float)(base * pow(1.0 + gamma * it, -power));
    case kLrPoly: {
      const double b = 1.0 - it / (double)s.max_iter;
      return (float)(base * pow(b > 0.0 ? b : 0.0, power));
    }
    case kLrSigmoid: return (float)(base / (1.0 + exp(-gamma * (it - (double)s.stepsize))));
    default: return s.base_lr[net];
  }
}

// The create-time refusals (Caffe's wording where it has one); 0: accepted, else the message is in msg.  policy is checked first,
// so a message can name it.
inline int lr_schedule_check(const LrSchedule& s, float weight_decay, int regularization_type, char* msg, size_t n) {
  const char* name = lr_policy_name(s.policy);
  if (!name) { snprintf(msg, n, "Unknown learning rate policy: %d", s.policy); return 1; }
  const double g = (double)s.gamma, p = (double)s.power;
  if (s.policy == kLrStep && !(s.stepsize > 0)) { snprintf(msg, n, "lr_policy step: stepsize > 0 required (got %d)", s.stepsize); return 1; }
  if ((s.policy == kLrStep || s.policy == kLrExp || s.policy == kLrMultistep) && !(g > 0.0 && isfinite(g))) {
    snprintf(msg, n, "lr_policy %s: gamma > 0 required (got %g)", name, g); return 1;
  }
  if (s.policy == kLrInv && !(g >= 0.0 && isfinite(g) && isfinite(p))) { snprintf(msg, n, "lr_policy inv: gamma >= 0 required (got gamma %g, power %g)", g, p); return 1; }
  if (s.policy == kLrMultistep) {
    if (s.n_stepvalue < 1 || s.n_stepvalue > kLrMaxStepvalues) {
      snprintf(msg, n, "lr_policy multistep: 1 to %d stepvalues required (got %d)", kLrMaxStepvalues, s.n_stepvalue); return 1;
    }
    for (int i = 0; i < s.n_stepvalue; ++i)
      if (s.stepvalue[i] <= (i ? s.stepvalue[i - 1] : 0)) {
        snprintf(msg, n, "lr_policy multistep: stepvalues must be positive and strictly increasing (stepvalue[%d] = %d)", i, s.stepvalue[i]); return 1;
      }
  }
  if (s.policy == kLrPoly) {
    if (!(s.max_iter > 0)) { snprintf(msg, n, "lr_policy poly: max_iter > 0 required (got %d)", s.max_iter); return 1; }
    if (!(p >= 0.0 && isfinite(p))) { snprintf(msg, n, "lr_policy poly: power >= 0 required (got %g)", p); return 1; }
  }
  if (s.policy == kLrSigmoid) {
    if (!(s.stepsize >= 0)) { snprintf(msg, n, "lr_policy sigmoid: stepsize >= 0 required (got %d)", s.stepsize); return 1; }
    if (!isfinite(g)) { snprintf(msg, n, "lr_policy sigmoid: gamma must be finite (got %g)", g); return 1; }
  }
  if (!((double)weight_decay >= 0.0 && isfinite((double)weight_decay))) { snprintf(msg, n, "weight_decay >= 0 required (got %g)", (double)weight_decay); return 1; }
  if (regularization_type != kRegL2 && regularization_type != kRegL1) { snprintf(msg, n, "Unknown regularization type: %d", regularization_type); return 1; }
  return 0;
}

}  // namespace dqnhip
