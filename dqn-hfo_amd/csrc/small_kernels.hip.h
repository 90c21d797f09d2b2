// small_kernels.hip.h — the small kernels learner.hip launches around the GEMMs and heads: the update's first launch (k_gather; k_gather_n with n-step returns), the
// clip norm's passes (k_sumsq*, k_to_bf16), the fused clip + Adam + soft-update pass with its riders (k_adam_soft*), the data-parallel
// tails and shards (k_tails, k_shard_*), k_advance_iter.  (Kernels are static: a unit that includes this embeds all of them.)
// What else once lived under this name is in learner_args.hip.h (structs), update_bodies.hip.h (device functions), head_kernels.hip.h,
// head_fwd_kernels.hip.h and io_kernels.hip.h.
#pragma once
#include "update_bodies.hip.h"

namespace dqnhip {

// the minibatch gather in a launch of its own (gather_block, update_bodies.hip.h)
static __global__ void k_gather(GatherArgs g) { gather_block(g, (int)blockIdx.x); }
// ... of a learner with n-step returns (gather_n_block): the update's first launch there, always a launch of its own
static __global__ void k_gather_n(GatherNArgs a) { gather_n_block(a, (int)blockIdx.x); }

// ---- optimiser -----------------------------------------------------------------
// Sum of squares of a gradient arena -> per-block partials (used after an
// all-reduce, where the GEMM-epilogue partials no longer describe the reduced
// gradient).
static __global__ __launch_bounds__(256) void k_sumsq(const float* __restrict__ g, size_t n4,
                                               float* __restrict__ partial) {
  __shared__ float s[4];
  float acc = 0.0f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
    acc = fmaf(v.x, v.x, acc); acc = fmaf(v.y, v.y, acc); acc = fmaf(v.z, v.z, acc); acc = fmaf(v.w, v.w, acc);
  }
  acc = wave_sum64(acc);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
}

// Data-parallel exchange in half the bytes (dqnhip_dp_init flag DQNHIP_DP_HALF_GRADS): the gradient arena crosses
// the links as bf16 (fp32's exponent range: no loss scale, no overflow; 8 significant bits, round-to-nearest-even)
// and is widened again by the pass that takes the clip norm of the reduced gradient.
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);   // NaN stays NaN
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static __global__ __launch_bounds__(256) void k_to_bf16(const float* __restrict__ g, size_t n4, uint16_t* __restrict__ out) {
  typedef __attribute__((ext_vector_type(4))) uint16_t u16x4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
    reinterpret_cast<u16x4*>(out)[i] = u16x4{f32_to_bf16(v.x), f32_to_bf16(v.y), f32_to_bf16(v.z), f32_to_bf16(v.w)};
  }
}
// bf16 image (after the all-reduce) -> fp32 arena + sum-of-squares partials (k_sumsq's layout and order)
static __global__ __launch_bounds__(256) void k_sumsq_bf16(const uint16_t* __restrict__ in, float* __restrict__ g, size_t n4,
                                                    float* __restrict__ partial) {
  typedef __attribute__((ext_vector_type(4))) uint16_t u16x4;
  __shared__ float s[4];
  float acc = 0.0f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const u16x4 h = reinterpret_cast<const u16x4*>(in)[i];
    const f32x4 v = f32x4{__builtin_bit_cast(float, (uint32_t)h.x << 16), __builtin_bit_cast(float, (uint32_t)h.y << 16),
                          __builtin_bit_cast(float, (uint32_t)h.z << 16), __builtin_bit_cast(float, (uint32_t)h.w << 16)};
    reinterpret_cast<f32x4*>(g)[i] = v;
    acc = fmaf(v.x, v.x, acc); acc = fmaf(v.y, v.y, acc); acc = fmaf(v.z, v.z, acc); acc = fmaf(v.w, v.w, acc);
  }
  acc = wave_sum64(acc);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
}

// the optimiser pass (adam_soft_body, update_bodies.hip.h) in a launch of its own, any unroll / load flavour (tuning probes)
template <int U, int NT>
__global__ __launch_bounds__(256) void k_adam_soft_t(AdamArgs a) {
  __shared__ float s[8];
  adam_soft_body<U, NT>(a, blockIdx.x, gridDim.x, s);
}

static __global__ __launch_bounds__(256) void k_adam_soft(AdamArgs a) {
  __shared__ float s[8];
  __shared__ double sq[4];
  adam_soft_body<1, 0>(a, blockIdx.x, gridDim.x, s);
  // The update's bookkeeping (statistics, ++iter of both solvers, the sampling counter) rides in block 0 of the update's
  // last launch.  It used to wait for the LAST block to arrive (two levels of arrival counters: every block read the
  // iteration counters in its prologue) — a tail of 2.5-5 us behind the last stores (same-box A/B: 3 108-3 132 against
  // 3 138-3 157 updates/s without it).  With the bias correction and the soft-update switch left in DevState by the
  // update's first launch, no block of this launch reads anything tick_body writes, so block 0 runs it as soon as its
  // own slice is done, beside the other 2047 blocks.
  if (a.tick_on && blockIdx.x == 0) {
    const bool skipped = s[7] == 1.0f;      // (2: dynamic loss scaling backed off — skipped, not reported)
    __syncthreads();
    tick_body(a.tick, s, sq, skipped);
  }
}

// The update's last launch inside a multi-update graph: the first g.blocks workgroups are the NEXT update's gather
// (nothing it reads or writes is touched by this optimiser pass: the minibatch panels are dead until that update's first
// forward, its scalars go to the other DevState slot, its counters come from DevState::gbase), the rest is k_adam_soft.
// Takes the gather (a ~5-us launch of two dependent HBM round trips) off the chain of all but the first update of such a graph.
static __global__ __launch_bounds__(256) void k_adam_soft_gather(AdamArgs a, GatherArgs g) {
  const int b0 = adam_routed_block(a, (int)blockIdx.x, g.blocks);
  __shared__ float s[8];
  __shared__ double sq[4];
  if (b0 < g.blocks) { gather_block(g, b0); return; }
  const int blk = b0 - g.blocks;
  adam_soft_body<1, 0>(a, blk, (int)gridDim.x - g.blocks, s);
  if (a.tick_on && blk == 0) {
    const bool skipped = s[7] == 1.0f;      // (2: dynamic loss scaling backed off — skipped, not reported)
    __syncthreads();
    tick_body(a.tick, s, sq, skipped);
  }
}

// ---- the first tower layer of the pass that follows, inside the optimiser launch (round 5) -------------------------------------
// The launch after the critic's optimiser pass is the first layer of critic(s, mu(s)): K = S + 10 padded to 64 / 128, a 5-us
// launch-floor link whose only late operand is the layer's own, just-updated weights.  Here the launch's first r.blocks
// workgroups each OWN 16 output rows of W1 (and their 16 biases): they take the step on that slice (adam_apply4: the strided pass's
// arithmetic), keep the new weights in LDS and run the layer for those 16 outputs over every minibatch row — the split of the
// reduction over the four waves, the step order and the (w0 + w1) + (w2 + w3) reduction of fwd_direct_body, so the activations
// are bit-identical to that launch's.  The strided pass belongs to the other workgroups and starts behind the slice
// (AdamArgs::skip4).  The riders are issued first and done after ~10 us of a 20-us pass.
// (First form, measured: the riders also took their share of the strided pass and walked the rows one 16-row tile at a time,
// every step behind its own load round trip: 26.8 us per launch against 19.7 + 5.0.)
template <int G>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void k_adam_soft_fwd1(AdamArgs a, FirstLayerRider r) {   // (six workgroups per CU, as k_adam_soft: 1536 resident at once)
  __shared__ float s[8];
  __shared__ __attribute__((aligned(16))) float sW[16 * 64 * G];
  __shared__ __attribute__((aligned(16))) float sB[16];
  __shared__ __attribute__((aligned(16))) float park[4096];
  const int b = adam_routed_block(a, (int)blockIdx.x, r.blocks);
  if (b < r.blocks) {
    FirstLayerWork<G> work(a, r, b, sW, sB, park);
    work.request();
    adam_scalars<true>(a, -1, s);          // (-1: the strided pass's first workgroup reports a skipped step)
    // (a skipped step — non-finite gradient norm — still runs the layer, on the weights as they are)
    work.run(s[4], s[5], s[6] != 0.0f, s[7] == 0.0f);
    return;
  }
  adam_soft_body<1, 0, true>(a, b - r.blocks, (int)gridDim.x - r.blocks, s);
}

// ... with the NEXT update's gather in the same launch (multi-update graphs, round 5: the gather moves from the update's last launch
// to this one, so that the next update's first-layer inputs are complete BEFORE the actor's optimiser launch — k_adam_soft_l0)
template <int G>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void k_adam_soft_fwd1_gather(AdamArgs a, FirstLayerRider r, GatherArgs g) {
  __shared__ float s[8];
  __shared__ __attribute__((aligned(16))) float sW[16 * 64 * G];
  __shared__ __attribute__((aligned(16))) float sB[16];
  __shared__ __attribute__((aligned(16))) float park[4096];
  const int b = adam_routed_block(a, (int)blockIdx.x, r.blocks, g.blocks);
  if (b < r.blocks) {
    FirstLayerWork<G> work(a, r, b, sW, sB, park);
    work.request();
    adam_scalars<true>(a, -1, s);
    work.run(s[4], s[5], s[6] != 0.0f, s[7] == 0.0f);
    return;
  }
  if (b < r.blocks + g.blocks) { gather_block(g, b - r.blocks); return; }
  adam_soft_body<1, 0, true>(a, b - r.blocks - g.blocks, (int)gridDim.x - r.blocks - g.blocks, s);
}

// ---- the NEXT update's four first tower layers inside the actor's optimiser launch (round 5) -------------------------------------
// With the next update's minibatch panels gathered one launch group earlier (above; the two panels this update still reads exist
// twice), nothing but the actor's own step stands between this launch and the next update's first GEMM launch
// (first_layers_launch).  The workgroups that own 16 rows of the ACTOR's W1 take the step in registers — which also gives them
// the target actor's soft-updated rows — and run actor(s) and actor_target(s') for those outputs (ActorL0); critic(s, a)'s first
// layer and the state half of critic_target's read weights that have been final since the critic's step: plain riders (PlainL0).
// Every element as fwd_direct_body computes it.  The next update then starts at its second layer.
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void k_adam_soft_l0(AdamArgs a, ActorL0 ra, PlainL0 p0, PlainL0 p1) {
  __shared__ float s[8];
  __shared__ double sq[4];
  __shared__ __attribute__((aligned(16))) float sW[2 * 16 * 64];
  __shared__ __attribute__((aligned(16))) float sB[32];
  __shared__ __attribute__((aligned(16))) float park[4096];
  int b = adam_routed_block(a, (int)blockIdx.x, ra.blocks, p0.blocks, p1.blocks);
  if (b < ra.blocks) {
    ActorL0Work work(a, ra, b, sW, sB, park);
    work.request();
    adam_scalars<true>(a, -1, s);
    work.run(s[4], s[5], s[6] != 0.0f, s[7] == 0.0f);
    return;
  }
  b -= ra.blocks;
  if (b < p0.blocks) { if (p0.Kred == 64) plain_l0_run<1>(p0, b, park); else plain_l0_run<2>(p0, b, park); return; }
  b -= p0.blocks;
  if (b < p1.blocks) { if (p1.Kred == 64) plain_l0_run<1>(p1, b, park); else plain_l0_run<2>(p1, b, park); return; }
  b -= p1.blocks;
  adam_soft_body<1, 0, true>(a, b, (int)gridDim.x - ra.blocks - p0.blocks - p1.blocks, s);
  if (a.tick_on && b == 0) {
    const bool skipped = s[7] == 1.0f;      // (2: dynamic loss scaling backed off — skipped, not reported)
    __syncthreads();
    tick_body(a.tick, s, sq, skipped);
  }
}

// Sharded optimiser (DQNHIP_DP_SHARD_OPT): the sum of squares of THIS rank's slice of the reduced gradient, folded from
// k_sumsq's partials with the tree adam_scalars uses (strided sums, butterfly, fixed cross-wave order: a one-rank group
// then derives the same bits as the replicated form) into tail[3]; the 4-float tail is what the ranks all-reduce.
static __global__ __launch_bounds__(256) void k_shard_scal(const float* __restrict__ partial, int n_partial, float* tail) {
  __shared__ float s[4];
  float acc = 0.0f;
  for (int i = threadIdx.x; i < n_partial; i += 256) acc += partial[i];
  acc = wave_sum64(acc);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) tail[3] = (s[0] + s[1]) + (s[2] + s[3]);
}
// dqnhip_apply_update_sharded (one process standing in for every rank of a group in turn): total += the slice's sum
static __global__ void k_shard_accumulate(float* total, const float* tail, int first) {
  total[0] = first ? tail[3] : total[0] + tail[3];
}

// Reduce the per-block loss / q partials into the gradient-arena tails (tails_block, gemm_common.hip.h) in a launch of its own: the
// form for schedules without a carrier launch; otherwise the block rides in the net's last backward launch (TailsArgs::on).
static __global__ __launch_bounds__(256) void k_tails(TailsArgs a) {
  __shared__ float sdot[4];
  __shared__ double sq[4];
  tails_block(a, sdot, sq);
}

// ++iter of one solver (dqnhip_apply_update: set_iter(iter() + 1), src/dqn.cpp:965)
// It is also this path's "tick": an optimiser pass outside an update may have raised kFlagGradNorm (skipped step), and
// dqnhip_read_stats only reads the host-mapped words — mirror the sticky flags there (loss / avg_q stay the last update's).
static __global__ void k_advance_iter(DevState* st, int which, float* host_stats) {
  if (which == 0) st->actor_iter += 1; else st->critic_iter += 1;
  if (host_stats != nullptr) {
    const int fl = __hip_atomic_load(&st->flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    host_stats[2] = __builtin_bit_cast(float, fl);
  }
}

}  // namespace dqnhip
