// head_kernels.hip.h — the head layers' training kernels, launched by learner.hip: TD target + Euclidean loss (k_head_q_train, its restatements k_head_q_train_w / k_head_q_train_n, or
// inside the critic's top-layer dgrad launch: k_dgrad_qtrain), the heads' backward with the inverting gradients (k_head_bwd,
// k_head_bwd_big + k_head_wred, k_dqda_head_bwd).  The heads' forward: head_fwd_kernels.hip.h.
#pragma once
#include "gemm_direct.hip.h"
#include "update_bodies.hip.h"
#include "noise_bodies.hip.h"      // k_target_smooth: the normal draw, the clipped term, apply-and-clamp

namespace dqnhip {

// Both critic heads of the training step in one launch: q' = q_values(critic_target tower
// top), q = q_values(critic tower top), then the TD target (src/dqn.cpp:892-900, doubles where
// the reference has them) and the EuclideanLoss diff.  One wave per row.
static __global__ __launch_bounds__(256) void k_head_q_train(HeadTrainArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  __shared__ float s_part[4];
  float at = 0.0f, ao = 0.0f;
  // the row's scalars and the two biases: requested before the dot products, used after the reduction
  float bt0 = 0.0f, b0 = 0.0f, r = 0.0f, mcv = 0.0f, tm = 0.0f;
  if (row < a.rows && lane == 0) { bt0 = a.bt[0]; b0 = a.b[0]; r = a.reward[row]; mcv = a.mc[row]; tm = a.term[row]; }
  if (row < a.rows) {
    const size_t x0 = (size_t)row * a.H;
    auto dots = [&](auto tag) {
      for (int k = lane * 4; k < a.H; k += 256) {
        const f32x4 v0 = head_ld4t<decltype(tag)::value>(a.Xt, a.Xt16, x0 + k), w0 = *reinterpret_cast<const f32x4*>(a.Wt + k);
        const f32x4 v1 = head_ld4t<decltype(tag)::value>(a.X, a.X16, x0 + k), w1 = *reinterpret_cast<const f32x4*>(a.W + k);
        at = fmaf(v0.x, w0.x, at); at = fmaf(v0.y, w0.y, at); at = fmaf(v0.z, w0.z, at); at = fmaf(v0.w, w0.w, at);
        ao = fmaf(v1.x, w1.x, ao); ao = fmaf(v1.y, w1.y, ao); ao = fmaf(v1.z, w1.z, ao); ao = fmaf(v1.w, w1.w, ao);
      }
    };
    HEAD_DISPATCH(a.X16 != nullptr, dots);
  }
  at = wave_sum64(at); ao = wave_sum64(ao);
  float d2 = 0.0f, dq_row = 0.0f;
  if (row < a.rows && lane == 0) {
    const float qt = at + bt0, q = ao + b0;
    a.q_target[row] = qt; a.q[row] = q;
    const float off_policy = tm != 0.0f ? r : (float)((double)r + a.gamma * (double)qt);
    const float target = (float)(a.beta * (double)mcv + (1 - a.beta) * (double)off_policy);
    a.y[row] = target;
    if (!isfinite(target)) atomicOr(&a.st->flags, kFlagTarget);   // CHECK(std::isfinite(target)), src/dqn.cpp:898
    const float d = q - target;
    dq_row = a.inv_batch * d;
    a.dq[row] = dq_row;
    d2 = d * d;
  }
  if ((a.dZ != nullptr || a.dZ16 != nullptr) && row < a.rows) {     // (wave-uniform condition)
    const float dqv = __shfl(dq_row, 0, 64);
    const size_t x0 = (size_t)row * a.H;
    const float sc16 = a.dZ16 != nullptr ? ls_live(a.scale16, a.ls_mult) : 0.0f;      // (dynamic loss scaling: times the critic's live multiplier)
    auto seed = [&](auto tag) {
      for (int k = lane * 4; k < a.H; k += 256) {
        const f32x4 xv = head_ld4t<decltype(tag)::value>(a.X, a.X16, x0 + k), wv = *reinterpret_cast<const f32x4*>(a.W + k);
        // k_head_bwd<1>'s arithmetic: s0 = fma(d, w, 0) = d * w, then * lrelu'(x)
        f32x4 dz;
        dz.x = (dqv * wv.x) * lrelu_mask(xv.x); dz.y = (dqv * wv.y) * lrelu_mask(xv.y);
        dz.z = (dqv * wv.z) * lrelu_mask(xv.z); dz.w = (dqv * wv.w) * lrelu_mask(xv.w);
        if constexpr (decltype(tag)::value)
          *reinterpret_cast<head_h4*>(a.dZ16 + x0 + k) = head_h4{(_Float16)(dz.x * sc16), (_Float16)(dz.y * sc16), (_Float16)(dz.z * sc16), (_Float16)(dz.w * sc16)};
        else
          *reinterpret_cast<f32x4*>(a.dZ + x0 + k) = dz;
      }
    };
    HEAD_DISPATCH(a.X16 != nullptr, seed);
  }
  if (lane == 0) s_part[wave] = d2;
  __syncthreads();
  if (threadIdx.x == 0) a.loss_partial[blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// Prioritized replay: k_head_q_train restated with per-row importance weights (a copy, so that k_head_q_train keeps its instruction
// stream).  Every wave forms pmin = min_j prob[j] over the minibatch (the customary normalisation by the batch's largest weight
// (N pmin)^-beta; N cancels) and beta from the live critic iteration, so graph replays anneal without host traffic; the row's weight
// is w = (pmin / prob[row])^beta, 1.0f exactly when beta == 0.  dq_row = (inv_batch d) w, the loss partial (d d) w: with w = 1.0f both
// are k_head_q_train's bits.  Everything downstream reads dq from its buffer (the head's dW / db riders) or gets it here (dZ / dZ16).
// Also stores w[row] and td_abs[row] = |d| for the write-back (k_per_update).
__device__ __forceinline__ float per_beta_now(float beta0, int anneal, int critic_iter) {
  if (anneal <= 0) return beta0;
  return fminf(1.0f, beta0 + (1.0f - beta0) * ((float)critic_iter / (float)anneal));
}
static __global__ __launch_bounds__(256) void k_head_q_train_w(HeadTrainWArgs aw) {
  const HeadTrainArgs& a = aw.t;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  __shared__ float s_part[4];
  float at = 0.0f, ao = 0.0f;
  float bt0 = 0.0f, b0 = 0.0f, r = 0.0f, mcv = 0.0f, tm = 0.0f, pr = 1.0f;
  if (row < a.rows && lane == 0) { bt0 = a.bt[0]; b0 = a.b[0]; r = a.reward[row]; mcv = a.mc[row]; tm = a.term[row]; pr = aw.prob[row]; }
  float pmin = INFINITY;
  for (int j = lane; j < a.rows; j += 64) pmin = fminf(pmin, aw.prob[j]);
  if (row < a.rows) {
    const size_t x0 = (size_t)row * a.H;
    auto dots = [&](auto tag) {
      for (int k = lane * 4; k < a.H; k += 256) {
        const f32x4 v0 = head_ld4t<decltype(tag)::value>(a.Xt, a.Xt16, x0 + k), w0 = *reinterpret_cast<const f32x4*>(a.Wt + k);
        const f32x4 v1 = head_ld4t<decltype(tag)::value>(a.X, a.X16, x0 + k), w1 = *reinterpret_cast<const f32x4*>(a.W + k);
        at = fmaf(v0.x, w0.x, at); at = fmaf(v0.y, w0.y, at); at = fmaf(v0.z, w0.z, at); at = fmaf(v0.w, w0.w, at);
        ao = fmaf(v1.x, w1.x, ao); ao = fmaf(v1.y, w1.y, ao); ao = fmaf(v1.z, w1.z, ao); ao = fmaf(v1.w, w1.w, ao);
      }
    };
    HEAD_DISPATCH(a.X16 != nullptr, dots);
  }
  at = wave_sum64(at); ao = wave_sum64(ao);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) pmin = fminf(pmin, __shfl_xor(pmin, off, 64));
  float d2 = 0.0f, dq_row = 0.0f;
  if (row < a.rows && lane == 0) {
    const float qt = at + bt0, q = ao + b0;
    a.q_target[row] = qt; a.q[row] = q;
    const float off_policy = tm != 0.0f ? r : (float)((double)r + a.gamma * (double)qt);
    const float target = (float)(a.beta * (double)mcv + (1 - a.beta) * (double)off_policy);
    a.y[row] = target;
    if (!isfinite(target)) atomicOr(&a.st->flags, kFlagTarget);   // CHECK(std::isfinite(target)), src/dqn.cpp:898
    const float beta = per_beta_now(aw.beta0, aw.beta_anneal_iters, a.st->critic_iter);
    const float w = beta == 0.0f ? 1.0f : powf(__fdiv_rn(pmin, pr), beta);
    const float d = q - target;
    dq_row = (a.inv_batch * d) * w;
    a.dq[row] = dq_row;
    d2 = (d * d) * w;
    aw.w[row] = w; aw.td_abs[row] = fabsf(d);
  }
  if ((a.dZ != nullptr || a.dZ16 != nullptr) && row < a.rows) {     // (wave-uniform condition)
    const float dqv = __shfl(dq_row, 0, 64);
    const size_t x0 = (size_t)row * a.H;
    const float sc16 = a.dZ16 != nullptr ? ls_live(a.scale16, a.ls_mult) : 0.0f;
    auto seed = [&](auto tag) {
      for (int k = lane * 4; k < a.H; k += 256) {
        const f32x4 xv = head_ld4t<decltype(tag)::value>(a.X, a.X16, x0 + k), wv = *reinterpret_cast<const f32x4*>(a.W + k);
        f32x4 dz;
        dz.x = (dqv * wv.x) * lrelu_mask(xv.x); dz.y = (dqv * wv.y) * lrelu_mask(xv.y);
        dz.z = (dqv * wv.z) * lrelu_mask(xv.z); dz.w = (dqv * wv.w) * lrelu_mask(xv.w);
        if constexpr (decltype(tag)::value)
          *reinterpret_cast<head_h4*>(a.dZ16 + x0 + k) = head_h4{(_Float16)(dz.x * sc16), (_Float16)(dz.y * sc16), (_Float16)(dz.z * sc16), (_Float16)(dz.w * sc16)};
        else
          *reinterpret_cast<f32x4*>(a.dZ + x0 + k) = dz;
      }
    };
    HEAD_DISPATCH(a.X16 != nullptr, seed);
  }
  if (lane == 0) s_part[wave] = d2;
  __syncthreads();
  if (threadIdx.x == 0) a.loss_partial[blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// n-step returns: k_head_q_train (WEIGHTED: k_head_q_train_w) restated with a per-row discount — again a copy, so that the two keep
// their instruction streams.  a.reward[row] is the window's discounted reward sum R and disc[row] = gamma^m (k_gather_n); the
// target is k_head_q_train's expression with disc[row] in a.gamma's place and R in r's: off = term ? R : (float)((double)R +
// disc (double)q').  At m = 1 (every row of an n = 1 learner) disc is gamma and R is r: the 1-step kernels' bits.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_head_q_train_n(HeadTrainNArgs an) {
  const HeadTrainWArgs& aw = an.w;
  const HeadTrainArgs& a = aw.t;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  __shared__ float s_part[4];
  float at = 0.0f, ao = 0.0f;
  float bt0 = 0.0f, b0 = 0.0f, r = 0.0f, mcv = 0.0f, tm = 0.0f, pr = 1.0f;
  double disc = 0.0;
  if (row < a.rows && lane == 0) {
    bt0 = a.bt[0]; b0 = a.b[0]; r = a.reward[row]; mcv = a.mc[row]; tm = a.term[row]; disc = an.disc[row];
    if constexpr (WEIGHTED) pr = aw.prob[row];
  }
  float pmin = INFINITY;
  if constexpr (WEIGHTED)
    for (int j = lane; j < a.rows; j += 64) pmin = fminf(pmin, aw.prob[j]);
  if (row < a.rows) {
    const size_t x0 = (size_t)row * a.H;
    auto dots = [&](auto tag) {
      for (int k = lane * 4; k < a.H; k += 256) {
        const f32x4 v0 = head_ld4t<decltype(tag)::value>(a.Xt, a.Xt16, x0 + k), w0 = *reinterpret_cast<const f32x4*>(a.Wt + k);
        const f32x4 v1 = head_ld4t<decltype(tag)::value>(a.X, a.X16, x0 + k), w1 = *reinterpret_cast<const f32x4*>(a.W + k);
        at = fmaf(v0.x, w0.x, at); at = fmaf(v0.y, w0.y, at); at = fmaf(v0.z, w0.z, at); at = fmaf(v0.w, w0.w, at);
        ao = fmaf(v1.x, w1.x, ao); ao = fmaf(v1.y, w1.y, ao); ao = fmaf(v1.z, w1.z, ao); ao = fmaf(v1.w, w1.w, ao);
      }
    };
    HEAD_DISPATCH(a.X16 != nullptr, dots);
  }
  at = wave_sum64(at); ao = wave_sum64(ao);
  if constexpr (WEIGHTED) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) pmin = fminf(pmin, __shfl_xor(pmin, off, 64));
  }
  float d2 = 0.0f, dq_row = 0.0f;
  if (row < a.rows && lane == 0) {
    const float qt = at + bt0, q = ao + b0;
    a.q_target[row] = qt; a.q[row] = q;
    const float off_policy = tm != 0.0f ? r : (float)((double)r + disc * (double)qt);
    const float target = (float)(a.beta * (double)mcv + (1 - a.beta) * (double)off_policy);
    a.y[row] = target;
    if (!isfinite(target)) atomicOr(&a.st->flags, kFlagTarget);   // CHECK(std::isfinite(target)), src/dqn.cpp:898
    const float d = q - target;
    if constexpr (WEIGHTED) {
      const float beta = per_beta_now(aw.beta0, aw.beta_anneal_iters, a.st->critic_iter);
      const float w = beta == 0.0f ? 1.0f : powf(__fdiv_rn(pmin, pr), beta);
      dq_row = (a.inv_batch * d) * w;
      d2 = (d * d) * w;
      aw.w[row] = w; aw.td_abs[row] = fabsf(d);
    } else {
      dq_row = a.inv_batch * d;
      d2 = d * d;
    }
    a.dq[row] = dq_row;
  }
  if ((a.dZ != nullptr || a.dZ16 != nullptr) && row < a.rows) {     // (wave-uniform condition)
    const float dqv = __shfl(dq_row, 0, 64);
    const size_t x0 = (size_t)row * a.H;
    const float sc16 = a.dZ16 != nullptr ? ls_live(a.scale16, a.ls_mult) : 0.0f;
    auto seed = [&](auto tag) {
      for (int k = lane * 4; k < a.H; k += 256) {
        const f32x4 xv = head_ld4t<decltype(tag)::value>(a.X, a.X16, x0 + k), wv = *reinterpret_cast<const f32x4*>(a.W + k);
        f32x4 dz;
        dz.x = (dqv * wv.x) * lrelu_mask(xv.x); dz.y = (dqv * wv.y) * lrelu_mask(xv.y);
        dz.z = (dqv * wv.z) * lrelu_mask(xv.z); dz.w = (dqv * wv.w) * lrelu_mask(xv.w);
        if constexpr (decltype(tag)::value)
          *reinterpret_cast<head_h4*>(a.dZ16 + x0 + k) = head_h4{(_Float16)(dz.x * sc16), (_Float16)(dz.y * sc16), (_Float16)(dz.z * sc16), (_Float16)(dz.w * sc16)};
        else
          *reinterpret_cast<f32x4*>(a.dZ + x0 + k) = dz;
      }
    };
    HEAD_DISPATCH(a.X16 != nullptr, seed);
  }
  if (lane == 0) s_part[wave] = d2;
  __syncthreads();
  if (threadIdx.x == 0) a.loss_partial[blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// ---- Step(1)'s head arithmetic inside the critic's first backward launch (round 5) -------------------------------------------
// k_head_q_train sits between the critics' last forward launch and the critic's top-layer dgrad: a 4.9-us launch-floor link
// whose output the dgrad needs only as a PER-ROW SCALAR.  dZ_L[r][n] = (dq_r w_n) lrelu'(x_rn) = (-dq_r) U[r][n] with
// U = (-w) lrelu'(x), which does not depend on q: the online critic's top forward layer leaves U in its epilogue
// (GemmProblem::seed_w, as the dq = -1 pass already does), the dgrad runs on U, and
//     dZ_{L-1}[r][j] = ((sum_n U[r][n] W[n][j]) * (-dq_r)) * lrelu'(x_{L-1}[r][j])
// takes the scalar in its epilogue.  The two head dot products arrive in 16-column pieces from the critics' top forward layers
// (GemmProblem::dot_w: the finished activations are in that epilogue's registers anyway).  Each of the workgroup's four waves
// requests the pieces of four of the tile's 16 rows once its operand pipeline is primed (2 KB per workgroup), and after its last
// MFMA sums them, forms q', q, the TD target and dq (k_head_q_train's arithmetic from there on), publishes -dq_r in LDS before
// the body's barrier; afterwards the workgroup writes its 64-column slices of dZ_L (the next launch's wgrad reads them).  The
// workgroups of tile column 0 write the per-row outputs.  q', q and dZ_{L-1} differ from the two-launch form by fp32 round-off
// only (the dot product is summed in another fixed order; the scalar is applied after the reduction instead of before):
// DQNHIP_TUNE_SEPARATE_Q_TRAIN restores the two launches.
// Measured on the way (profiles/r05_dgrad_qtrain.txt): a FIFTH wave per workgroup reading the tower tops itself — 17.4 us against
// 8.3 + 4.8 for the two launches (it shares a SIMD and the CU's load path with an MFMA wave); the four MFMA waves reading their
// rows of the tower tops — 12.1 us (the 16 workgroups of a tile row each re-read the same 128 KB: +50% on an L2-bound kernel).
struct QTrainHook {
  const HeadTrainArgs& a; float* s_scale; float* s_dq; int q0; bool owner;
  float v0[4], v1[4];        // rows 4 wave + j: piece `lane` of the target / online head dot product (H / 16 <= 64 pieces)
  float rw[4], mcv[4], tm[4], bt0, b0;
  f32x4 xv, wv;              // this thread's piece of the workgroup's first dZ_L slice (row threadIdx.x / 16, 4 columns)
  int c_first;
  __device__ __forceinline__ QTrainHook(const HeadTrainArgs& a_, float* sc, float* sd, int q0_, int tile_p) : a(a_), s_scale(sc), s_dq(sd), q0(q0_), owner(tile_p == 0), c_first(tile_p * 64) {}
  __device__ __forceinline__ void after_prologue() {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int np = a.H >> 4;
    const int pc = lane < np ? lane : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t x0 = (size_t)(q0 + wave * 4 + j) * np + pc;
      v0[j] = a.pdt[x0]; v1[j] = a.pd[x0];
      const int row = q0 + wave * 4 + j;
      rw[j] = a.reward[row]; mcv[j] = a.mc[row]; tm[j] = a.term[row];
    }
    bt0 = a.bt[0]; b0 = a.b[0];
    if (c_first < a.H) {
      const int rr = threadIdx.x >> 4, c = c_first + ((threadIdx.x & 15) << 2);
      xv = *reinterpret_cast<const f32x4*>(a.X + (size_t)(q0 + rr) * a.H + c); wv = *reinterpret_cast<const f32x4*>(a.W + c);
    }
  }
  __device__ __forceinline__ void before_park() {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool in = lane < (a.H >> 4);
    float d2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rr = wave * 4 + j, row = q0 + rr;
      const float at = wave_sum64(in ? v0[j] : 0.0f), ao = wave_sum64(in ? v1[j] : 0.0f);
      const float r = rw[j];
      const float qt = at + bt0, q = ao + b0;
      const float off_policy = tm[j] != 0.0f ? r : (float)((double)r + a.gamma * (double)qt);      // src/dqn.cpp:893-900
      const float target = (float)(a.beta * (double)mcv[j] + (1 - a.beta) * (double)off_policy);
      const float d = q - target;
      const float dq_row = a.inv_batch * d;
      d2[j] = d * d;
      if (lane == 0) {
        s_scale[rr] = -dq_row; s_dq[rr] = dq_row;
        if (owner) {
          a.q_target[row] = qt; a.q[row] = q; a.y[row] = target; a.dq[row] = dq_row;
          if (!isfinite(target)) atomicOr(&a.st->flags, kFlagTarget);   // CHECK(std::isfinite(target)), src/dqn.cpp:898
        }
      }
    }
    // k_head_q_train's partial of its block of four rows (one row per wave there: ((w0 + w1) + w2) + w3)
    if (owner && lane == 0) a.loss_partial[(q0 >> 2) + wave] = ((d2[0] + d2[1]) + d2[2]) + d2[3];
  }
};
// the workgroup of tile (tile_p, tile_q): the dgrad tile with the head arithmetic hooked in, then its slices of dZ_L
__device__ __forceinline__ void dgrad_qtrain_block(const GemmProblem& pr, const int tile_p, const int tile_q, const HeadTrainArgs& a, float* smem, float* s_scale, float* s_dq) {
  const int q0 = tile_q * 16;
  QTrainHook hook(a, s_scale, s_dq, q0, tile_p);
  dgrad_lds_body<1, 1, true, QTrainHook>(pr, tile_p, tile_q, smem, s_scale, hook);
  // this workgroup's slices of dZ_L: columns [64 tile_p, +64) and every tiles_p-th slice after it, 16 rows (one float4 per thread);
  // s_dq was published before the body's barrier
  for (int c0 = tile_p * 64; c0 < a.H; c0 += pr.tiles_p * 64) {
    const int rr = threadIdx.x >> 4, c = c0 + ((threadIdx.x & 15) << 2);
    const size_t x0 = (size_t)(q0 + rr) * a.H + c;
    f32x4 xv = hook.xv, wv = hook.wv;       // (the first slice's operands were requested under the main loop)
    if (c0 != tile_p * 64) { xv = *reinterpret_cast<const f32x4*>(a.X + x0); wv = *reinterpret_cast<const f32x4*>(a.W + c); }
    const float dqv = s_dq[rr];
    f32x4 dz;
    dz.x = (dqv * wv.x) * lrelu_mask(xv.x); dz.y = (dqv * wv.y) * lrelu_mask(xv.y);
    dz.z = (dqv * wv.z) * lrelu_mask(xv.z); dz.w = (dqv * wv.w) * lrelu_mask(xv.w);
    *reinterpret_cast<f32x4*>(a.dZ + x0) = dz;
  }
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_dgrad_qtrain(DQN_PRELOAD_PARAMS, const GemmArgs<1> args, const HeadTrainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float s_scale[16], s_dq[16];
  int tile_p, tile_q;
  if (!(pre_flags & kPreValid)) {          // (switched off, or a value its field cannot hold: the GemmArgs path as it was)
    HotArgs<1> r;
    const int b = request_args(args, r, (int)blockIdx.x);
    const GemmProblem pr = problem_at<0>(args, r);
    tile_of_record<0>(r, b, tile_p, tile_q);
    dgrad_qtrain_block(pr, tile_p, tile_q, a, smem, s_scale, s_dq);
    return;
  }
  // the dgrad's operands from the preloaded words (GemmPreload, gemm_common.hip.h)
  const PreRecordTile t = preload_record_decode(DQN_PRELOAD_BLOCK, (int)blockIdx.x);      // (every block of this grid is a tile of the record)
  const GemmProblem pr = record_of_preload<0>(DQN_PRELOAD_BLOCK, args, t);
  dgrad_qtrain_block(pr, t.tile_p, t.tile_q, a, smem, s_scale, s_dq);
}
inline hipError_t dgrad_qtrain_launch(GemmBatch& batch, const HeadTrainArgs& a, const LaunchOn& on) {
  batch.n = 1;
  tile_batch(batch, 64, 16);
  GemmArgs<1> args;
  if (!pack_args(batch, args)) return hipErrorInvalidValue;
  const GemmPreload pre = make_preload_record(args, 0, on.no_preload);
  return launch(on, k_dgrad_qtrain<0>, dim3(batch.total_tiles), dim3(256), dgrad_lds_bytes<1, 1>(), DQN_PRELOAD_WORDS(pre), args, a);
}

// Fused head backward: in one pass over the tower top X4[rows][H]
//   (actor only) inverting gradients (src/dqn.cpp:924-957) on the critic's input-gradient
//                columns -> dYh[m][0..9]
//   dZ4[m][k]  = (sum_j dYh[m][j] Wh[j][k]) * lrelu'(X4[m][k])       (head dgrad + ReLU bwd)
//   dWh[j][k]  = sum_m dYh[m][j] X4[m][k] ;  dbh[j] = sum_m dYh[m][j]  (head wgrad)
//   + one sum-of-squares partial per block.
// Block = 64 columns x 16 row groups (1024 threads); row groups are added in fixed order.
// Replaces three launches (invert, head dgrad, head wgrad) and 16x the parallelism of the
// old column-strip wgrad.
// Grid = (H/64 column blocks) x (RC row chunks); block = 64 columns x 16 row groups.  Each block
// writes its dZ rows directly and a partial dW slab; the LAST block to arrive for a column block
// (agent-scope release -> ticket -> acquire, guide G16) adds the RC slabs in fixed order, so the
// result does not depend on which block that is.
// cross-block hand-off words: coherent at agent scope without a fence on either side
__device__ __forceinline__ void slab_st(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float slab_ld(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <int NH>
__global__ __launch_bounds__(1024) void k_head_bwd(HeadBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int RC = a.rc_blocks > 0 ? a.rc_blocks : gridDim.y, rc = blockIdx.y, nkb = gridDim.x;
  if (a.q_out != nullptr && rc >= RC) {                // rider blocks: one wave per row, k-strips of float4
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = (((int)blockIdx.y - RC) * (int)gridDim.x + (int)blockIdx.x) * 16 + wave;
    if (row >= a.rows) return;
    const float* rW = a.qr_W ? a.qr_W : a.W; const float* rX = a.qr_W ? a.qr_X4 : a.X4;
    const _Float16* rX16 = a.qr_W ? a.qr_X416 : a.X416; const int rH = a.qr_W ? a.qr_H : a.H;
    const size_t x0 = (size_t)row * rH;
    float acc = 0.0f;
    auto dots = [&](auto tag) {
      for (int k = lane * 4; k < rH; k += 256) {
        const f32x4 xv = head_ld4t<decltype(tag)::value>(rX, rX16, x0 + k), wv = *reinterpret_cast<const f32x4*>(rW + k);
        acc = fmaf(xv.x, wv.x, acc); acc = fmaf(xv.y, wv.y, acc); acc = fmaf(xv.z, wv.z, acc); acc = fmaf(xv.w, wv.w, acc);
      }
    };
    HEAD_DISPATCH(rX16 != nullptr, dots);
    acc = wave_sum64(acc);
    if (lane == 0) { const float v = acc + a.q_bias[0]; a.q_out[row] = v; a.qsum_partial[row] = (double)v; }
    return;
  }
  const int rows_c = (a.rows + RC - 1) / RC;           // rows of this chunk
  const int r0 = rc * rows_c, r1 = min(a.rows, r0 + rows_c);
  float* s_dy = sm;                                    // [rows_c][NH]
  float* s_acc = sm + rows_c * NH;                     // [16][NH][64]
  __shared__ int s_last;
  const int tid = threadIdx.x;
  const bool want_w = a.dW != nullptr;
  const int kc = tid & 63, rg = tid >> 6;              // 16 row groups
  const int k = blockIdx.x * 64 + kc;
  const int per = (r1 - r0 + 15) / 16;
  const int m0 = r0 + rg * per, m1 = min(r1, m0 + per);
  // this thread's head weights and its first four tower-top values go out BEFORE the head diffs are staged: neither
  // depends on them, and the staging (two dependent loads + the inverting-gradients arithmetic + a barrier) is a chain
  // of its own.  Rows are then taken four at a time, four independent loads in flight, instead of one load per iteration.
  constexpr int RB = 4;
  float w[NH];
#pragma unroll
  for (int j = 0; j < NH; ++j) w[j] = a.W[(size_t)j * a.H + k];
  float xpre[RB];
  auto ldx = [&](int m) -> float { return a.X416 != nullptr ? (float)a.X416[(size_t)m * a.H + k] : a.X4[(size_t)m * a.H + k]; };
#pragma unroll
  for (int u = 0; u < RB; ++u) xpre[u] = (m0 + u < m1) ? ldx(m0 + u) : 0.0f;
  // ---- head diffs of this chunk's rows into LDS
  for (int i = tid; i < (r1 - r0) * NH; i += 1024) {
    const int m = r0 + i / NH, j = i % NH;
    float d;
    if constexpr (NH == kNO) {
      d = a.dXc[(size_t)m * a.ldx + a.S + j];
      const float out = a.aout16[(size_t)m * kAP + j];
      float mn, mx;
      inverting_bounds(j, mn, mx);
      if (d < 0) d *= (mx - out) / (mx - mn);
      else if (d > 0) d *= (out - mn) / (mx - mn);
      if (blockIdx.x == 0) a.dA16[(size_t)m * kAP + j] = d;
    } else {
      d = a.dyh ? a.dyh[(size_t)m * a.lddy + j] : -1.0f;
    }
    s_dy[i] = d;
  }
  __syncthreads();
  float acc[NH];
#pragma unroll
  for (int j = 0; j < NH; ++j) acc[j] = 0.0f;
  const float sc16 = a.dZ16 != nullptr ? ls_live(a.scale16, a.ls_mult) : 0.0f;      // (dynamic loss scaling: times the net's live multiplier)
  auto rows_loop = [&](auto tag) {
  for (int mb = m0; mb < m1; mb += RB) {
    float xb[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u)
      xb[u] = (mb == m0) ? xpre[u] : ((mb + u < m1) ? head_ld1t<decltype(tag)::value>(a.X4, a.X416, (size_t)(mb + u) * a.H + k) : 0.0f);
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const int m = mb + u;
      if (m >= m1) break;
      const float xv = xb[u];
      float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
      for (int j = 0; j < NH; ++j) {
        const float d = s_dy[(m - r0) * NH + j];
        // Split layer: action_layer's and actionpara_layer's bottom diffs are
        // formed separately and added
        if (NH == kNO && j >= kNA) s1 = fmaf(d, w[j], s1); else s0 = fmaf(d, w[j], s0);
        acc[j] = fmaf(d, xv, acc[j]);
      }
      if (NH == kNO) s0 += s1;
      const float dz = s0 * lrelu_mask(xv);
      if (a.dZ != nullptr) a.dZ[(size_t)m * a.H + k] = dz;
      if (a.dZ16 != nullptr) a.dZ16[(size_t)m * a.H + k] = (_Float16)(dz * sc16);
    }
  }
  };
  HEAD_DISPATCH(a.X416 != nullptr, rows_loop);
  if (!want_w) return;
#pragma unroll
  for (int j = 0; j < NH; ++j) s_acc[(rg * NH + j) * 64 + kc] = acc[j];
  __syncthreads();
  // this chunk's partial: row groups added in fixed order
  float* my_slab = a.slab + ((size_t)rc * nkb + blockIdx.x) * NH * 64;
  if (rg < NH) {                                      // wave j folds head j (NH <= 16 waves)
    const int j = rg;
    float v = 0.0f;
#pragma unroll
    for (int g = 0; g < 16; ++g) v += s_acc[(g * NH + j) * 64 + kc];
    slab_st(&my_slab[j * 64 + kc], v);
  }
  if (rg == NH && blockIdx.x == 0 && kc < NH) {       // partial bias gradient of this chunk (a spare wave)
    float v = 0.0f;
    for (int m = 0; m < r1 - r0; ++m) v += s_dy[m * NH + kc];
    slab_st(&a.slab[(size_t)RC * nkb * NH * 64 + rc * 16 + kc], v);
  }
  // publish the slab, take a ticket; the last arriver reduces (placement independent).  The slab travels as
  // agent-scope (sc1: write-through / L2-bypassing) stores and loads, drained before the ticket — not plain stores +
  // a release fence (the fence writes back the whole L2, this launch's dZ rows included, once per block, and the
  // last arriver's acquire invalidates it again).  Measured alternatives at 256 rows, same-box A/B: one row chunk on
  // 32-column blocks (no counter): no gain; the gradients from an extra grid row of blocks that walk all rows: -0.8 %.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    // The hand-off is MI355X_MICROARCH.md's "handoff-flag" form for gfx950: write-through (sc1) payload stores, the storing
    // waves' `s_waitcnt vmcnt(0)` above, a barrier, then a relaxed agent-scope counter; the last arriver reads the slabs with
    // sc1 (L1-bypassing) loads.  No release / acquire fence: an agent-scope release writes the whole L2 back — this launch's
    // dZ rows included — once per block (measured round 4 with ACQ_REL here: k_head_bwd<10> 9.6 -> 10.7 us, <1> 6.2 -> 6.8
    // at 512 fp16 rows).  That is an ISA-level guarantee, not one of the HIP memory model, so it is pinned by
    // a stress test that checks every word of the reduced gradient under uneven load from a second stream
    // (tests/test_gpu_head_handoff.py); shapes whose head gradients ride in a carrier launch never come here.
    const int t = __hip_atomic_fetch_add(a.ticket + blockIdx.x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (t == RC - 1);
  }
  __syncthreads();
  if (!s_last) return;
  float ssq = 0.0f;
  if (rg < NH) {
    const int j = rg;
    float v = 0.0f;
    for (int c = 0; c < RC; ++c) v += slab_ld(&a.slab[((size_t)c * nkb + blockIdx.x) * NH * 64 + j * 64 + kc]);
    a.dW[(size_t)j * a.H + k] = v;
    ssq = v * v;
  } else if (rg == NH && blockIdx.x == 0 && kc < NH) {
    float v = 0.0f;
    for (int c = 0; c < RC; ++c) v += slab_ld(&a.slab[(size_t)RC * nkb * NH * 64 + c * 16 + kc]);
    a.db[kc] = v;
    ssq = v * v;
  }
  ssq = wave_sum64(ssq);
  if (kc == 0) s_acc[rg] = ssq;                        // s_acc is free again
  __syncthreads();
  if (tid == 0) {
    float t = 0.0f;
#pragma unroll
    for (int g = 0; g <= NH; ++g) t += s_acc[g];        // heads in order, then the bias wave
    if (a.partial != nullptr) a.partial[blockIdx.x] = t;
    a.ticket[blockIdx.x] = 0;                          // re-arm for the next launch
  }
}

// ---- critic dQ/da + inverting gradients + actor heads' backward in ONE launch (round 5) ----------------------------------------
// The critic's BackwardFrom(q_values) chain (src/dqn.cpp:918-923) ends in the first layer's input gradient, of which only the ten
// action columns are consumed; the inverting-gradients pass (:924-957) and the actor heads' backward (BackwardFrom(actionpara_layer),
// :960-963: head dgrad + the tower top's ReLU') follow.  They used to be two launch-floor launches (gemm_dgrad_narrow_qrider:
// 32 tiles of 16 x 16 + the q riders, 6.2 us; k_head_bwd<10>: 4.8 us).  Here workgroup (row tile t, column chunk c) recomputes
// the 16 x 16 tile of dQ/da for its 16 rows — a 1024-deep reduction on four waves, 0.1 us of MFMA: recomputing it in each of the
// H / 256 column chunks costs less than handing it across a kernel boundary — inverts it, and writes its 16 x 256 piece of the
// actor's tower-top gradient.  Same arithmetic in the same order as the two kernels it replaces (bit-identical: the narrow
// tile's values do not depend on which columns a workgroup owns, the head part is k_head_bwd's loop).  The q(s, mu(s)) riders
// come last in the grid, as before.  The head's own dW / db are the wgrad-tail launch's riders (HeadWgradRider).
// The kernarg preload block of k_dqda_head_bwd<false> (the idea of GemmPreload, gemm_common.hip.h, with this kernel's own words): what
// routes a workgroup and what its first loads are addressed from — the head part's (ten head weights, the tower-top column, mu(s))
// and the narrow tile's operands — as 14 leading scalar parameters, which gfx950 delivers in SGPRs at wave launch.  Everything
// else (dA16, dZ, the tile's mask, dxc, the rider) still comes from DqdaHeadArgs / QHeadRider, read in those loads' shadow.
// A value that does not fit its field, the fp16 form, or DQNHIP_TUNE_NO_KERNARG_PRELOAD: route = 0, the block is not valid and
// the workgroup gathers the same values in one round of scalar loads, as before.
struct DqdaPreload {
  const float* W; const float* X4; const float* aout16; const float* P; const float* Q;
  uint32_t ldp, ldq;
  uint32_t h_kred;             // H | Kred << 16
  uint32_t route;              // kPreValid | row_tiles << 1 | column chunks << 17 (dxc given: 1)
};
static_assert(sizeof(DqdaPreload) == 14 * 4, "16 user SGPRs less the kernarg pointer");
#define DQN_DQDA_PRELOAD_PARAMS const float* pre_W, const float* pre_X4, const float* pre_aout16, const float* pre_P, const float* pre_Q, \
    uint32_t pre_ldp, uint32_t pre_ldq, uint32_t pre_h_kred, uint32_t pre_route
#define DQN_DQDA_PRELOAD_WORDS(w) (w).W, (w).X4, (w).aout16, (w).P, (w).Q, (w).ldp, (w).ldq, (w).h_kred, (w).route
// what a workgroup's routing and first loads need, from either source
struct DqdaFirst { int H, row_tiles, tiles; const float* W; const float* X4; const float* aout16; };
__host__ __device__ __forceinline__ DqdaFirst dqda_preload_decode(const DqdaPreload& w) {
  DqdaFirst f;
  f.H = (int)(w.h_kred & 0xFFFFu);
  f.row_tiles = (int)((w.route >> 1) & 0xFFFFu);
  f.tiles = f.row_tiles * (int)(w.route >> 17);
  f.W = w.W; f.X4 = w.X4; f.aout16 = w.aout16;
  return f;
}
inline DqdaPreload make_dqda_preload(const DqdaHeadArgs& a, int row_tiles, bool off) {
  DqdaPreload w{};
  const int chunks = a.dxc != nullptr ? 1 : (a.H + 255) / 256;
  if (off || a.dZ16 != nullptr || a.X4 == nullptr) return w;
  if (a.H < 1 || a.H > 0xFFFF || a.pr.Kred < 0 || a.pr.Kred > 0xFFFF || row_tiles < 1 || row_tiles > 0xFFFF || chunks > 0x7FFF) return w;
  if (a.pr.ldp < 0 || a.pr.ldp > kMaxLeadingDim || a.pr.ldq < 0 || a.pr.ldq > kMaxLeadingDim) return w;
  w.W = a.W; w.X4 = a.X4; w.aout16 = a.aout16; w.P = a.pr.P; w.Q = a.pr.Q;
  w.ldp = (uint32_t)a.pr.ldp; w.ldq = (uint32_t)a.pr.ldq;
  w.h_kred = (uint32_t)a.H | (uint32_t)a.pr.Kred << 16;
  w.route = kPreValid | (uint32_t)row_tiles << 1 | (uint32_t)chunks << 17;
  return w;
}
// tile workgroup blk (f.tiles of them; the riders behind them are the kernel's business): pr = the narrow tile's problem (fp32 form)
template <bool F16>
__device__ __forceinline__ void dqda_head_block(const DqdaHeadArgs& a, const DqdaFirst& f, const GemmProblem& pr, const int blk,
                                                float* smem, float (*s_d)[17], float* s_dy) {
  const int rt = blk % f.row_tiles, cc = blk / f.row_tiles;
  const int tid = threadIdx.x, q0 = rt * 16;
  // (round 6: any tower-top width — the reference's own tower ends in 128 units; threads beyond it keep column H - 1's loads, take
  // part in the tile and the barriers, and store nothing)
  const bool live = (cc << 8) + tid < f.H;
  const int k = live ? (cc << 8) + tid : f.H - 1;
  // everything the head part needs that does not depend on dQ/da goes out first: this thread's ten head weights, its column of
  // the 16 tower-top rows, and (160 threads) one output of mu(s)
  float wh[kNO], xv[16];
#pragma unroll
  for (int j = 0; j < kNO; ++j) wh[j] = f.W[(size_t)j * f.H + k];
#pragma unroll
  for (int r = 0; r < 16; ++r) xv[r] = F16 ? (float)a.X416[(size_t)(q0 + r) * f.H + k] : f.X4[(size_t)(q0 + r) * f.H + k];
  float out = 0.0f;
  if (tid < 16 * kNO) out = f.aout16[(size_t)(q0 + tid / kNO) * kAP + tid % kNO];
  f32x4 v;
  float sc16 = 0.0f;
  if constexpr (F16) {
    v = dgrad_narrow_tile16<8>(a.t16, rt, smem);
    // (dynamic loss scaling: the incoming panel carries ls_q x mult, the outgoing one ls_a x mult — DqdaHeadArgs::ls_mult, whose
    // pointer came with the launch's one round of scalar loads; the pair itself is read behind the tile)
    float inv_ls = a.inv_ls;
    sc16 = a.scale16;
    if (a.ls_mult != nullptr) { inv_ls *= a.ls_mult[1]; sc16 *= a.ls_mult[0]; }
    v.x *= inv_ls; v.y *= inv_ls; v.z *= inv_ls; v.w *= inv_ls;
  }
  else v = dgrad_narrow_tile<8>(pr, 0, rt, smem);
  if (tid < 64) {                          // wave 0 holds the tile: lane (li, lg), register r = dX[row q0 + li][column 4 lg + r]
    const int li = tid & 15, lg = tid >> 4;
    s_d[li][(lg << 2) + 0] = v.x; s_d[li][(lg << 2) + 1] = v.y; s_d[li][(lg << 2) + 2] = v.z; s_d[li][(lg << 2) + 3] = v.w;
  }
  __syncthreads();
  if (a.dxc != nullptr) {                  // (uniform) the separate form: dQ/da itself, for k_head_bwd<10>
    if (tid < 16 * kNO) a.dxc[(size_t)(q0 + tid / kNO) * a.lddxc + tid % kNO] = s_d[tid / kNO][tid % kNO];
    return;
  }
  if (tid < 16 * kNO) {                    // inverting gradients (k_head_bwd<10>'s staging loop)
    const int r = tid / kNO, j = tid % kNO;
    float d = s_d[r][j];
    float mn, mx;
    inverting_bounds(j, mn, mx);
    if (d < 0) d *= (mx - out) / (mx - mn);
    else if (d > 0) d *= (out - mn) / (mx - mn);
    if (cc == 0) a.dA16[(size_t)(q0 + r) * kAP + j] = d;
    s_dy[tid] = d;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int j = 0; j < kNO; ++j) {
      const float d = s_dy[r * kNO + j];
      // Split layer: action_layer's and actionpara_layer's bottom diffs are formed separately and added
      if (j >= kNA) s1 = fmaf(d, wh[j], s1); else s0 = fmaf(d, wh[j], s0);
    }
    s0 += s1;
    const float dz = s0 * lrelu_mask(xv[r]);
    if (!live) continue;
    if constexpr (F16) a.dZ16[(size_t)(q0 + r) * f.H + k] = (_Float16)(dz * sc16);
    else a.dZ[(size_t)(q0 + r) * f.H + k] = dz;
  }
}
template <bool F16 = false>
__global__ __launch_bounds__(256) void k_dqda_head_bwd(DQN_DQDA_PRELOAD_PARAMS, const DqdaHeadArgs a, const QHeadRider rider) {
  extern __shared__ __attribute__((aligned(16))) float smem[];     // the narrow dgrad's parking area (4 waves x 64 lanes x 16 B)
  __shared__ float s_d[16][17];
  __shared__ float s_dy[16 * kNO];
  if constexpr (!F16) {
    if (pre_route & kPreValid) {
      // routing, the head part's first loads and the narrow tile's operands from the preloaded words: no scalar wait in front of them
      const DqdaPreload w{pre_W, pre_X4, pre_aout16, pre_P, pre_Q, pre_ldp, pre_ldq, pre_h_kred, pre_route};
      const DqdaFirst f = dqda_preload_decode(w);
      const int blk = (int)blockIdx.x;
      if (blk >= f.tiles) { q_head_rider(rider, blk - f.tiles); return; }
      GemmProblem pr = a.pr;
      pr.P = w.P; pr.Q = w.Q; pr.ldp = (int)w.ldp; pr.ldq = (int)w.ldq; pr.Kred = (int)(w.h_kred >> 16);
      dqda_head_block<false>(a, f, pr, blk, smem, s_d, s_dy);
      return;
    }
  }
  // what routes the workgroup, what the head part's first loads need and the narrow tile's operands: ONE round of scalar loads
  // (request_args, gemm_bodies.hip.h, has the reasoning; left alone: the tile count, then the head's pointers, then the tile's)
  int blk = (int)blockIdx.x;
  if constexpr (F16) asm volatile("" : "+s"(blk) : "s"(a.H), "s"(a.row_tiles), "s"(a.W), "s"(a.X416), "s"(a.aout16), "s"(a.t16.P), "s"(a.t16.Q), "s"(a.t16.ldp), "s"(a.t16.Kred), "s"(a.ls_mult));
  else asm volatile("" : "+s"(blk) : "s"(a.H), "s"(a.row_tiles), "s"(a.W), "s"(a.X4), "s"(a.aout16), "s"(a.pr.P), "s"(a.pr.Q), "s"(a.pr.ldp), "s"(a.pr.Kred));
  DqdaFirst f;
  f.H = a.H; f.row_tiles = a.row_tiles; f.tiles = a.row_tiles * (a.dxc != nullptr ? 1 : (a.H + 255) >> 8);
  f.W = a.W; f.X4 = a.X4; f.aout16 = a.aout16;
  if (blk >= f.tiles) { q_head_rider(rider, blk - f.tiles); return; }
  dqda_head_block<F16>(a, f, a.pr, blk, smem, s_d, s_dy);
}
inline hipError_t dqda_head_bwd_launch(DqdaHeadArgs& a, const QHeadRider& rider, const LaunchOn& on) {
  a.row_tiles = a.rows / 16;
  a.pr.tiles_p = 1; a.pr.tiles_q = a.row_tiles; a.pr.tile_base = 0;
  // (dxc given: the tile alone, column chunk 0 of every row tile)
  const dim3 grid(a.row_tiles * (a.dxc != nullptr ? 1 : (a.H + 255) / 256) + rider.blocks);
  const DqdaPreload w = make_dqda_preload(a, a.row_tiles, on.no_preload);
  if (a.dZ16 != nullptr) return launch(on, k_dqda_head_bwd<true>, grid, dim3(256), kNarrowDgradLds, DQN_DQDA_PRELOAD_WORDS(w), a, rider);
  return launch(on, k_dqda_head_bwd<false>, grid, dim3(256), kNarrowDgradLds, DQN_DQDA_PRELOAD_WORDS(w), a, rider);
}

// ---- head backward for large minibatches (rows >= 1024) -------------------------------------
// Same arithmetic as k_head_bwd, re-tiled for bandwidth: block = 64 rows x 256 columns, wave = 16
// rows, lane = 4 consecutive columns (16-B loads / stores of X4 and dZ).  Per-chunk partial head
// gradients go to a slab [rows/64][NH][H]; k_head_wred adds the chunks in index order.  In fp16
// mode the tower-top gradient is written directly as the scaled fp16 panel, replacing the fp32 panel +
// conversion pass.
template <int NH>
__global__ __launch_bounds__(256) void k_head_bwd_big(HeadBwdBigArgs b) {
  typedef __attribute__((ext_vector_type(4))) _Float16 h4;
  const HeadBwdArgs& a = b.a;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* s_dy = sm;                                    // [64][NH]
  float* s_red = sm + 64 * NH;                         // [4][NH][256]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  if (b.chunks > 0 && (int)blockIdx.x >= b.chunks) {
    // (rider: the q head of HeadBwdArgs::qr_* when given — the fp16 learner's critic(s, mu(s)) head in the ACTOR heads' launch —
    // else this launch's own head, the dq = -1 launch)
    const float* rW = a.qr_W ? a.qr_W : a.W; const float* rX4 = a.qr_W ? a.qr_X4 : a.X4;
    const _Float16* rX416 = a.qr_W ? a.qr_X416 : a.X416; const int rH = a.qr_W ? a.qr_H : a.H;
    // one wave per row, four rows of the wave in flight at once (16 x 16-B loads per lane before the first use:
    // with one row at a time the rider was a chain of exposed memory latencies, 9 us at 4096 rows)
    const int nwave = ((int)gridDim.x - b.chunks) * (int)gridDim.y * 4;
    const int wv = (((int)blockIdx.x - b.chunks) * (int)gridDim.y + (int)blockIdx.y) * 4 + w;
    const bool hoist = rH <= 1024;
    f32x4 wreg[4];
    if (hoist) {
#pragma unroll
      for (int t = 0; t < 4; ++t) { const int k = lane * 4 + 256 * t; wreg[t] = k < rH ? *reinterpret_cast<const f32x4*>(rW + k) : f32x4{0.f, 0.f, 0.f, 0.f}; }
    }
    for (int r0 = wv * 4; r0 < a.rows; r0 += nwave * 4) {
      if (hoist) {
        f32x4 xr[4][4];
        if (rX416 != nullptr) {
          head_h4 hr[4][4];
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const int k = lane * 4 + 256 * t;
              hr[j][t] = (r0 + j < a.rows && k < rH) ? *reinterpret_cast<const head_h4*>(rX416 + (size_t)(r0 + j) * rH + k) : head_h4{(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
            }
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) xr[j][t] = f32x4{(float)hr[j][t].x, (float)hr[j][t].y, (float)hr[j][t].z, (float)hr[j][t].w};
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const int k = lane * 4 + 256 * t;
              xr[j][t] = (r0 + j < a.rows && k < rH) ? *reinterpret_cast<const f32x4*>(rX4 + (size_t)(r0 + j) * rH + k) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float acc = 0.0f;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            acc = fmaf(xr[j][t].x, wreg[t].x, acc); acc = fmaf(xr[j][t].y, wreg[t].y, acc);
            acc = fmaf(xr[j][t].z, wreg[t].z, acc); acc = fmaf(xr[j][t].w, wreg[t].w, acc);
          }
          acc = wave_sum64(acc);
          if (lane == 0 && r0 + j < a.rows) { const float v = acc + a.q_bias[0]; a.q_out[r0 + j] = v; a.qsum_partial[r0 + j] = (double)v; }
        }
      } else {
        for (int j = 0; j < 4 && r0 + j < a.rows; ++j) {
          const size_t x0 = (size_t)(r0 + j) * rH;
          float acc = 0.0f;
          for (int k = lane * 4; k < rH; k += 256) {
            const f32x4 xv = head_ld4(rX4, rX416, x0 + k), wv4 = *reinterpret_cast<const f32x4*>(rW + k);
            acc = fmaf(xv.x, wv4.x, acc); acc = fmaf(xv.y, wv4.y, acc); acc = fmaf(xv.z, wv4.z, acc); acc = fmaf(xv.w, wv4.w, acc);
          }
          acc = wave_sum64(acc);
          if (lane == 0) { const float v = acc + a.q_bias[0]; a.q_out[r0 + j] = v; a.qsum_partial[r0 + j] = (double)v; }
        }
      }
    }
    return;
  }
  const int m0 = blockIdx.x * 64, kb = blockIdx.y * 256, k0 = kb + lane * 4;
  const bool want_w = a.dW != nullptr;
  // the head weights and all 16 rows of this wave's strip of the tower top go out BEFORE the head diffs are staged: neither
  // depends on them, and the staging (two dependent loads, the inverting-gradients arithmetic, a barrier) is a memory round
  // trip of its own that used to sit in front of these loads (round 4: one exposed latency less per launch)
  f32x4 wv[NH], acc[NH];
#pragma unroll
  for (int j = 0; j < NH; ++j) { wv[j] = *reinterpret_cast<const f32x4*>(a.W + (size_t)j * a.H + k0); acc[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  f32x4 xr[16];
  head_h4 hr[16];
  if (a.X416 != nullptr) {
#pragma unroll
    for (int r = 0; r < 16; ++r) hr[r] = *reinterpret_cast<const head_h4*>(a.X416 + (size_t)(m0 + w * 16 + r) * a.H + k0);
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) xr[r] = *reinterpret_cast<const f32x4*>(a.X4 + (size_t)(m0 + w * 16 + r) * a.H + k0);
  }
  for (int i = tid; i < 64 * NH; i += 256) {
    const int m = m0 + i / NH, j = i % NH;
    float d;
    if constexpr (NH == kNO) {
      d = a.dXc[(size_t)m * a.ldx + a.S + j];
      const float out = a.aout16[(size_t)m * kAP + j];
      float mn, mx;
      inverting_bounds(j, mn, mx);
      if (d < 0) d *= (mx - out) / (mx - mn);
      else if (d > 0) d *= (out - mn) / (mx - mn);
      if (blockIdx.y == 0) a.dA16[(size_t)m * kAP + j] = d;
    } else {
      d = a.dyh ? a.dyh[(size_t)m * a.lddy + j] : -1.0f;
    }
    s_dy[i] = d;
  }
  const float sc16 = b.dZ16 != nullptr ? ls_live(b.scale16, a.ls_mult) : 0.0f;      // (dynamic loss scaling: times the net's live multiplier)
  __syncthreads();
  if (a.X416 != nullptr) {
#pragma unroll
    for (int r = 0; r < 16; ++r) xr[r] = f32x4{(float)hr[r].x, (float)hr[r].y, (float)hr[r].z, (float)hr[r].w};
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int ml = w * 16 + r, m = m0 + ml;
    const f32x4 x = xr[r];
    f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NH; ++j) {
      const float d = s_dy[ml * NH + j];
      if (NH == kNO && j >= kNA) { s1.x = fmaf(d, wv[j].x, s1.x); s1.y = fmaf(d, wv[j].y, s1.y); s1.z = fmaf(d, wv[j].z, s1.z); s1.w = fmaf(d, wv[j].w, s1.w); }
      else { s0.x = fmaf(d, wv[j].x, s0.x); s0.y = fmaf(d, wv[j].y, s0.y); s0.z = fmaf(d, wv[j].z, s0.z); s0.w = fmaf(d, wv[j].w, s0.w); }
      acc[j].x = fmaf(d, x.x, acc[j].x); acc[j].y = fmaf(d, x.y, acc[j].y); acc[j].z = fmaf(d, x.z, acc[j].z); acc[j].w = fmaf(d, x.w, acc[j].w);
    }
    if (NH == kNO) { s0.x += s1.x; s0.y += s1.y; s0.z += s1.z; s0.w += s1.w; }
    const f32x4 dz = f32x4{s0.x * lrelu_mask(x.x), s0.y * lrelu_mask(x.y), s0.z * lrelu_mask(x.z), s0.w * lrelu_mask(x.w)};
    if (a.dZ != nullptr) *reinterpret_cast<f32x4*>(a.dZ + (size_t)m * a.H + k0) = dz;
    if (b.dZ16 != nullptr) {
      const h4 hz = h4{(_Float16)(dz.x * sc16), (_Float16)(dz.y * sc16), (_Float16)(dz.z * sc16), (_Float16)(dz.w * sc16)};
      *reinterpret_cast<h4*>(b.dZ16 + (size_t)m * a.H + k0) = hz;
    }
  }
  if (want_w) {
#pragma unroll
    for (int j = 0; j < NH; ++j) *reinterpret_cast<f32x4*>(s_red + ((w * NH + j) * 256 + lane * 4)) = acc[j];
  }
  if (!want_w) return;
  __syncthreads();
  float* slab = b.slab2 + (size_t)blockIdx.x * NH * a.H;
  for (int i = tid; i < NH * 256; i += 256) {
    const int j = i >> 8, c = i & 255;
    slab[(size_t)j * a.H + kb + c] = (s_red[(0 * NH + j) * 256 + c] + s_red[(1 * NH + j) * 256 + c]) +
                                     (s_red[(2 * NH + j) * 256 + c] + s_red[(3 * NH + j) * 256 + c]);
  }
  if (blockIdx.y == 0 && tid < NH) {
    float v = 0.0f;
    for (int m = 0; m < 64; ++m) v += s_dy[m * NH + tid];
    const size_t n_chunks = b.chunks > 0 ? (size_t)b.chunks : (size_t)gridDim.x;      // (rider blocks extend the grid beyond the row chunks)
    b.slab2[n_chunks * NH * a.H + blockIdx.x * 16 + tid] = v;
  }
}
// adds the row-chunk slabs of k_head_bwd_big: block = (64 columns, head j); the 4 waves take every
// 4th chunk and are combined in fixed order.  Writes dW, db and one sum-of-squares partial per
// (head, 64 columns) into partial[j * H/64 + column block].
template <int NH>
__global__ __launch_bounds__(256) void k_head_wred(HeadBwdBigArgs b, int chunks) {
  const HeadBwdArgs& a = b.a;
  __shared__ float s[4][64];
  __shared__ float s_bias;
  const int j = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blockIdx.x * 64 + lane;
  float v = 0.0f;
#pragma unroll 4
  for (int c = w; c < chunks; c += 4) v += b.slab2[((size_t)c * NH + j) * a.H + k];
  s[w][lane] = v;
  if (w == 1) {
    float t = 0.0f;
    if (blockIdx.x == 0) {
      for (int c = lane; c < chunks; c += 64) t += b.slab2[(size_t)chunks * NH * a.H + c * 16 + j];
      t = wave_sum64(t);
      if (lane == 0) a.db[j] = t;
    }
    if (lane == 0) s_bias = t * t;
  }
  __syncthreads();
  if (w != 0) return;
  v = (s[0][lane] + s[1][lane]) + (s[2][lane] + s[3][lane]);
  a.dW[(size_t)j * a.H + k] = v;
  float ssq = v * v;
  ssq = wave_sum64(ssq);
  if (lane == 0 && a.partial != nullptr) a.partial[j * gridDim.x + blockIdx.x] = ssq + s_bias;
}

// ---- target policy smoothing (dqnhip_target_noise_enable) ----------------------------------------------------------------------
// One launch between the actors' head launch and the critics' first layers: a~ = clamp(mu'(s') + range clip(sigma z, -clip, clip)) over
// the mu'(s') columns the head left in aout_t16 (which keep the clean values), written into the critic-target's action columns of Xc_nx
// and, with the z used, into the debug rows.  z is keyed by (noise seed, c, row 32 + 2 j) with c = DevState::update_counter as it
// stands when the launch runs: every earlier update's tick has advanced it, this update's has not, so c is the counter gather_block
// samples this update with (update_counter, or gbase_counter + ahead inside a multi-update graph).  Thread = one (row, padded column).
struct TargetSmoothArgs {
  NoiseCfg cfg;
  const DevState* st;
  const float* mu16;               // [rows][kAP] the target actor's head outputs
  float* xc; int ldxc, xc_col;     // the critic-target's input panel: a~ goes to columns [xc_col, xc_col + kNO)
  float* smoothed16; float* z16;   // [rows][kAP] a~ and the z used
  unsigned long long* counter;     // [1] c
  int rows;
};
static __global__ __launch_bounds__(256) void k_target_smooth(const TargetSmoothArgs a) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int r = gid >> 4, j = gid & 15;
  const unsigned long long c = a.st->update_counter;
  if (gid == 0) *a.counter = c;
  if (r >= a.rows || j >= kNO) return;
  const float z = noise_normal(a.cfg.seed, c, noise_lane0(r, j));
  const float t = noise_clipped(noise_sigma(a.cfg, j), z, a.cfg.clip);
  const float v = noise_apply(a.mu16[(size_t)r * kAP + j], j, t, a.cfg.clamp);
  a.xc[(size_t)r * a.ldxc + a.xc_col + j] = v;
  a.smoothed16[(size_t)r * kAP + j] = v;
  a.z16[(size_t)r * kAP + j] = z;
}

}  // namespace dqnhip
