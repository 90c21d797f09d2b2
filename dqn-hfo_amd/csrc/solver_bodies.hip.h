// solver_bodies.hip.h — the optimiser pass of Caffe's other solvers (SGD, Nesterov, AdaGrad, RMSProp, AdaDelta): __device__ functions,
// no kernel.  The Adam pass (update_bodies.hip.h: adam_soft_body, adam_apply4) is tuned and stays as it is; these are its siblings with
// one rule each, on the same skeleton: SGDSolver::ClipGradients + <Solver>::ComputeUpdateValue + Net::Update + DQN::SoftUpdateNet in ONE
// pass over (w, g, h, [h2,] w_target).  28 B/param for the four single-history solvers, 36 B/param for AdaDelta.
// The rules are Caffe's CPU solvers @2ef5847 written from upstream knowledge (not re-verifiable offline) — each in ONE
// function, so that a correction touches one place.  The float32 expression order of each is part of the interface
// (include/dqnhip.h, tests/solver_ref.py derives the per-element bounds from it): contraction is off inside them.
#pragma once
#include "update_bodies.hip.h"

namespace dqnhip {

// = DQNHIP_SOLVER_* (include/dqnhip.h; static_assert in solver_kernels.hip.h)
enum Solver { kSolverAdam = 0, kSolverSGD = 1, kSolverNesterov = 2, kSolverAdaGrad = 3, kSolverRMSProp = 4, kSolverAdaDelta = 5 };

// What a rule reads of AdamArgs: lr, beta1 (cfg.momentum), eps (cfg.delta) — and beta2, which on a non-Adam learner carries
// cfg.rms_decay (adam_launch; no solver but Adam reads momentum2, and AdamArgs is an argument of the tuned kernels: it keeps its layout).
struct SolverHyper { float lr, mom, delta, rho; };
__device__ __forceinline__ SolverHyper solver_hyper(const AdamArgs& a) { return SolverHyper{a.lr, a.beta1, a.eps, a.beta2}; }

// S13 SGDSolver::ComputeUpdateValue: history = lr * diff + momentum * history; diff = history
__device__ __forceinline__ float sgd_step(const SolverHyper& p, float gs, float& h, float w) {
#pragma clang fp contract(off)
  const float h1 = fmaf(p.lr, gs, p.mom * h);
  h = h1;
  return w - h1;
}
// S14 NesterovSolver: update_saved = history; history = lr * diff + momentum * history; diff = (1 + momentum) * history - momentum * update_saved
__device__ __forceinline__ float nesterov_step(const SolverHyper& p, float gs, float& h, float w) {
#pragma clang fp contract(off)
  const float mh0 = p.mom * h;
  const float h1 = fmaf(p.lr, gs, mh0);
  const float u = fmaf(1.0f + p.mom, h1, -mh0);
  h = h1;
  return w - u;
}
// S15 AdaGradSolver: history += diff^2; diff = lr * diff / (sqrt(history) + delta)
__device__ __forceinline__ float adagrad_step(const SolverHyper& p, float gs, float& h, float w) {
#pragma clang fp contract(off)
  const float h1 = fmaf(gs, gs, h);
  h = h1;
  return w - p.lr * (gs / (sqrtf(h1) + p.delta));
}
// S16 RMSPropSolver: history = rms_decay * history + (1 - rms_decay) * diff^2; diff = lr * diff / (sqrt(history) + delta)
__device__ __forceinline__ float rmsprop_step(const SolverHyper& p, float gs, float& h, float w) {
#pragma clang fp contract(off)
  const float h1 = fmaf(1.0f - p.rho, gs * gs, p.rho * h);
  h = h1;
  return w - p.lr * (gs / (sqrtf(h1) + p.delta));
}
// S17 AdaDeltaSolver: history of squared gradients h, of squared updates h2 (read BEFORE it is advanced); delta inside both roots;
// the learning rate scales the update only after the update history has taken it
__device__ __forceinline__ float adadelta_step(const SolverHyper& p, float gs, float& h, float& h2, float w) {
#pragma clang fp contract(off)
  const float h1 = fmaf(1.0f - p.mom, gs * gs, p.mom * h);
  const float u = gs * sqrtf((h2 + p.delta) / (h1 + p.delta));
  h2 = fmaf(1.0f - p.mom, u * u, p.mom * h2);
  h = h1;
  return w - p.lr * u;
}

// one float4 of the step, in place: clip scale, the rule, the soft target update (adam_apply4's frame)
template <int SOLVER>
__device__ __forceinline__ void solver_apply4(const AdamArgs& a, const SolverHyper& p, float scale, bool soft, const f32x4& g, f32x4& h, f32x4& h2, f32x4& w, f32x4& wt) {
  static_assert(SOLVER >= kSolverSGD && SOLVER <= kSolverAdaDelta, "Adam has kernels of its own");
  const float tau = a.tau, omt = 1 - a.tau;
  const float* gp = reinterpret_cast<const float*>(&g); float* hp = reinterpret_cast<float*>(&h);
  float* h2p = reinterpret_cast<float*>(&h2); float* wp = reinterpret_cast<float*>(&w);
  float* tp = reinterpret_cast<float*>(&wt);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float gs = gp[e] * scale;
    float wi;
    if constexpr (SOLVER == kSolverSGD) wi = sgd_step(p, gs, hp[e], wp[e]);
    else if constexpr (SOLVER == kSolverNesterov) wi = nesterov_step(p, gs, hp[e], wp[e]);
    else if constexpr (SOLVER == kSolverAdaGrad) wi = adagrad_step(p, gs, hp[e], wp[e]);
    else if constexpr (SOLVER == kSolverRMSProp) wi = rmsprop_step(p, gs, hp[e], wp[e]);
    else wi = adadelta_step(p, gs, hp[e], h2p[e], wp[e]);
    wp[e] = wi;
    if (soft) tp[e] = fmaf(tau, wi, omt * tp[e]);
  }
}

// adam_soft_body<1, 0>'s skeleton: the first batch of loads goes out before the per-launch scalars (adam_scalars, unchanged: clip
// scale s[4], soft switch s[6], the skip decision s[7] with the sticky flag, skipped_steps and dynamic loss scaling; its s[5] — Adam's
// lr x bias correction — is not read), one strided pass over float4s, no first-layer riders (skip4 = 0), the shared-prefix pointer
// selection and the fp16 mirrors.  The second history arena (a.v) is loaded and stored by AdaDelta alone: the single-history
// solvers never touch it.
template <int SOLVER>
__device__ __forceinline__ void solver_soft_body(const AdamArgs& a, int blk, int nblk, float* s /*>= 8 floats*/) {
  constexpr bool H2 = SOLVER == kSolverAdaDelta;
  f32x4 g, h, h2 = f32x4{0.f, 0.f, 0.f, 0.f}, w, wt;
  f32x4* wq; f32x4* tq;
  auto load = [&](size_t i) {
    wq = reinterpret_cast<f32x4*>(i < a.n4_sh ? a.w_sh : a.w) + i;
    tq = reinterpret_cast<f32x4*>(i < a.n4_sh ? a.wt_sh : a.wt) + i;
    g = reinterpret_cast<const f32x4*>(a.g)[i];
    h = reinterpret_cast<const f32x4*>(a.m)[i];
    if constexpr (H2) h2 = reinterpret_cast<const f32x4*>(a.v)[i];
    w = *wq;
    wt = *tq;
  };
  size_t i = (size_t)blk * 256 + threadIdx.x;
  if (i < a.n4) load(i);
  adam_scalars<false>(a, blk, s);
  if (s[7] != 0.0f) return;
  const float scale = s[4];
  const bool soft = s[6] != 0.0f;
  const SolverHyper p = solver_hyper(a);
  for (bool first = true; i < a.n4; i += (size_t)nblk * 256, first = false) {
    if (!first) load(i);
    solver_apply4<SOLVER>(a, p, scale, soft, g, h, h2, w, wt);
    const float* wp = reinterpret_cast<const float*>(&w); const float* tp = reinterpret_cast<const float*>(&wt);
    reinterpret_cast<f32x4*>(a.m)[i] = h;
    if constexpr (H2) reinterpret_cast<f32x4*>(a.v)[i] = h2;
    *wq = w;
    if (soft) *tq = wt;
    if (a.w16 != nullptr) {
      typedef __attribute__((ext_vector_type(4))) _Float16 h16x4_t;
      reinterpret_cast<h16x4_t*>(a.w16)[i] = h16x4_t{(_Float16)wp[0], (_Float16)wp[1], (_Float16)wp[2], (_Float16)wp[3]};
      if (soft) reinterpret_cast<h16x4_t*>(a.wt16)[i] = h16x4_t{(_Float16)tp[0], (_Float16)tp[1], (_Float16)tp[2], (_Float16)tp[3]};
    }
  }
}

// ---- the scheduled / regularised pass (k_sched_soft<>, solver_kernels.hip.h) ---------------------------------------------------
// A learner with an lr policy whose solver is not Adam, or any learner with weight_decay != 0: all six solvers, Adam included, on
// solver_soft_body's skeleton.  Two differences.  The step size is s[5] = a.lr x *a.corr_pre, where a.lr is 1 and the slot holds the
// update's rate (x Adam's bias correction) as the scalars block of the gather left it (GatherArgs::sched) — or a.lr is the fixed
// rate and the slot the plain correction (1 for the five other solvers) when only a decay was asked for.  And SGDSolver::Regularize
//  sits between the clip and the rule: gd = fmaf(decay, r, g x clip_scale), r = w (L2) or sign(w) with sign(0) = 0
// (L1), read from the w the pass holds anyway — the owner's on a shared prefix — so the bytes per parameter are the unregularised
// pass's: 28 for the single-history rules, 36 for Adam and AdaDelta.  The clip norm and the partial sums are the unregularised
// gradient's.  Decay and its kind are runtime values: one kernel per solver.
struct DecayArgs { float decay; int l1; };

// Adam's rule as adam_apply4 states it, on the regularised gradient, contraction off like its siblings here
__device__ __forceinline__ float adam_step(const SolverHyper& p, float beta2, float gs, float& m, float& v, float w) {
#pragma clang fp contract(off)
  const float mi = fmaf(1.0f - p.mom, gs, p.mom * m);
  const float vi = fmaf(1.0f - beta2, gs * gs, beta2 * v);
  m = mi; v = vi;
  return w - p.lr * (mi / (sqrtf(vi) + p.delta));
}

template <int SOLVER>
__device__ __forceinline__ void sched_apply4(const AdamArgs& a, const SolverHyper& p, const DecayArgs& d, float scale, bool soft, const f32x4& g, f32x4& h, f32x4& h2, f32x4& w, f32x4& wt) {
  const float tau = a.tau, omt = 1 - a.tau;
  const float* gp = reinterpret_cast<const float*>(&g); float* hp = reinterpret_cast<float*>(&h);
  float* h2p = reinterpret_cast<float*>(&h2); float* wp = reinterpret_cast<float*>(&w);
  float* tp = reinterpret_cast<float*>(&wt);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float w0 = wp[e];
    const float r = d.l1 ? (float)((w0 > 0.0f) - (w0 < 0.0f)) : w0;
    const float gs = fmaf(d.decay, r, gp[e] * scale);
    float wi;
    if constexpr (SOLVER == kSolverAdam) wi = adam_step(p, a.beta2, gs, hp[e], h2p[e], w0);
    else if constexpr (SOLVER == kSolverSGD) wi = sgd_step(p, gs, hp[e], w0);
    else if constexpr (SOLVER == kSolverNesterov) wi = nesterov_step(p, gs, hp[e], w0);
    else if constexpr (SOLVER == kSolverAdaGrad) wi = adagrad_step(p, gs, hp[e], w0);
    else if constexpr (SOLVER == kSolverRMSProp) wi = rmsprop_step(p, gs, hp[e], w0);
    else wi = adadelta_step(p, gs, hp[e], h2p[e], w0);
    wp[e] = wi;
    if (soft) tp[e] = fmaf(tau, wi, omt * tp[e]);
  }
}

// PRE: these launches exist inside an update only (adam_launch refuses the others), so adam_scalars reads both slots
template <int SOLVER>
__device__ __forceinline__ void sched_soft_body(const AdamArgs& a, const DecayArgs& d, int blk, int nblk, float* s /*>= 8 floats*/) {
  constexpr bool H2 = SOLVER == kSolverAdaDelta || SOLVER == kSolverAdam;
  f32x4 g, h, h2 = f32x4{0.f, 0.f, 0.f, 0.f}, w, wt;
  f32x4* wq; f32x4* tq;
  auto load = [&](size_t i) {
    wq = reinterpret_cast<f32x4*>(i < a.n4_sh ? a.w_sh : a.w) + i;
    tq = reinterpret_cast<f32x4*>(i < a.n4_sh ? a.wt_sh : a.wt) + i;
    g = reinterpret_cast<const f32x4*>(a.g)[i];
    h = reinterpret_cast<const f32x4*>(a.m)[i];
    if constexpr (H2) h2 = reinterpret_cast<const f32x4*>(a.v)[i];
    w = *wq;
    wt = *tq;
  };
  size_t i = (size_t)blk * 256 + threadIdx.x;
  if (i < a.n4) load(i);
  adam_scalars<true>(a, blk, s);
  if (s[7] != 0.0f) return;
  const float scale = s[4];
  const bool soft = s[6] != 0.0f;
  SolverHyper p = solver_hyper(a);
  p.lr = s[5];
  for (bool first = true; i < a.n4; i += (size_t)nblk * 256, first = false) {
    if (!first) load(i);
    sched_apply4<SOLVER>(a, p, d, scale, soft, g, h, h2, w, wt);
    const float* wp = reinterpret_cast<const float*>(&w); const float* tp = reinterpret_cast<const float*>(&wt);
    reinterpret_cast<f32x4*>(a.m)[i] = h;
    if constexpr (H2) reinterpret_cast<f32x4*>(a.v)[i] = h2;
    *wq = w;
    if (soft) *tq = wt;
    if (a.w16 != nullptr) {
      typedef __attribute__((ext_vector_type(4))) _Float16 h16x4_t;
      reinterpret_cast<h16x4_t*>(a.w16)[i] = h16x4_t{(_Float16)wp[0], (_Float16)wp[1], (_Float16)wp[2], (_Float16)wp[3]};
      if (soft) reinterpret_cast<h16x4_t*>(a.wt16)[i] = h16x4_t{(_Float16)tp[0], (_Float16)tp[1], (_Float16)tp[2], (_Float16)tp[3]};
    }
  }
}

}  // namespace dqnhip
