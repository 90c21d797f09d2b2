// gemm_experiments.hip.h — fp32 GEMM bodies that were built, measured against the learner's and NOT adopted.
// TEST-ONLY: variants of dqnhip_test_gemm (libdqnhip_test.so) on top of the product's gemm_direct.hip.h (DQN_MFMA, GemmBatch,
// direct_launch); the learner launches none of them and this header is not part of libdqnhip.so.
#pragma once
#include "gemm_direct.hip.h"

namespace dqnhip {

// ---- DGRAD, half-width tiles: 32 input columns x 16 rows (round 6 experiment) ---------------------------
// Twice the workgroups of dgrad_direct_body<1, 1> (512 for a 256 x 1024 x 1024 layer), each with half the MFMA chain and a quarter
// of the LDS: two (or more) co-resident per CU.  P = W read as 8-byte pieces (two columns per lane), Q = dY as in dgrad_direct_body.
// Harness variant 8 of dqnhip_test_gemm mode 1; measured against variants 1 (64 x 16 direct) and 5 (64 x 16, dY through the LDS
// transpose — the learner's): profiles/r06_dgrad_half_tiles.txt.
__device__ __forceinline__ void dgrad_direct32_body(const GemmProblem& pr, int tile_p, int tile_q, float* smem) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  constexpr int NACC = 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int p0 = tile_p * 32, q0 = tile_q * 16;
  const int Kw = pr.Kred >> 2;
  const int nkb = Kw >> 4;
  const float* pp = pr.P + (size_t)(wave * Kw + lg * 4) * pr.ldp + p0 + li * 2;
  const float* qp = pr.Q + (size_t)(q0 + li) * pr.ldq + wave * Kw + lg * 4;
  const size_t ldp = pr.ldp;
  f32x4 acc[NACC];
  acc[0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
  f32x2 rp[4][4]; f32x4 rq[4];
#define D32_LOAD(slot, kb)                                                              \
  {                                                                                     \
    rq[slot] = *reinterpret_cast<const f32x4*>(qp + ((kb) << 4));                      \
    _Pragma("unroll") for (int s = 0; s < 4; ++s)                                       \
        rp[slot][s] = *reinterpret_cast<const f32x2*>(pp + (size_t)(((kb) << 4) + s) * ldp); \
  }
#define D32_COMPUTE(slot)                                                               \
  {                                                                                     \
    _Pragma("unroll") for (int s = 0; s < 4; ++s)                                       \
    _Pragma("unroll") for (int pc = 0; pc < 2; ++pc)                                    \
        acc[pc] = DQN_MFMA(rp[slot][s][pc], rq[slot][s], acc[pc]);                      \
  }
  const int nkb4 = nkb & ~3;
  if (nkb4 > 0) {
    D32_LOAD(0, 0) D32_LOAD(1, 1) D32_LOAD(2, 2) D32_LOAD(3, 3)
    int kb = 0;
    for (; kb + 4 < nkb4; kb += 4) {
      D32_COMPUTE(0) DQN_PIN(); D32_LOAD(0, kb + 4) DQN_PIN();
      D32_COMPUTE(1) DQN_PIN(); D32_LOAD(1, kb + 5) DQN_PIN();
      D32_COMPUTE(2) DQN_PIN(); D32_LOAD(2, kb + 6) DQN_PIN();
      D32_COMPUTE(3) DQN_PIN(); D32_LOAD(3, kb + 7) DQN_PIN();
    }
    D32_COMPUTE(0) D32_COMPUTE(1) D32_COMPUTE(2) D32_COMPUTE(3)
  }
  for (int kb = nkb4; kb < nkb; ++kb) { D32_LOAD(0, kb) D32_COMPUTE(0) }
#undef D32_LOAD
#undef D32_COMPUTE
  // C/D map of acc[pc]: lane (li, lg), register r = dX[row q0 + li][column p0 + 2 (4 lg + r) + pc]: 8 consecutive columns per lane
  f32x4 m0 = f32x4{1.f, 1.f, 1.f, 1.f}, m1 = m0;
  if (wave == 0 && pr.mask != nullptr) {
    const float* mp = pr.mask + (size_t)(q0 + li) * pr.ldm + p0 + (lg << 3);
    m0 = *reinterpret_cast<const f32x4*>(mp); m1 = *reinterpret_cast<const f32x4*>(mp + 4);
  }
  park_accumulators<NACC>(smem, acc, wave, lane);
  __syncthreads();
  if (wave == 0) {
    const f32x4 a0 = reduce_accumulator<NACC>(smem, 0, lane), a1 = reduce_accumulator<NACC>(smem, 1, lane);
    f32x4 v0 = f32x4{a0.x, a1.x, a0.y, a1.y}, v1 = f32x4{a0.z, a1.z, a0.w, a1.w};
    if (pr.mask != nullptr) {
      v0.x *= lrelu_mask(m0.x); v0.y *= lrelu_mask(m0.y); v0.z *= lrelu_mask(m0.z); v0.w *= lrelu_mask(m0.w);
      v1.x *= lrelu_mask(m1.x); v1.y *= lrelu_mask(m1.y); v1.z *= lrelu_mask(m1.z); v1.w *= lrelu_mask(m1.w);
    }
    float* c = pr.C + (size_t)(q0 + li) * pr.ldc + p0 + (lg << 3);
    *reinterpret_cast<f32x4*>(c) = v0; *reinterpret_cast<f32x4*>(c + 4) = v1;
  }
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void gemm_dgrad_direct32(const GemmBatch batch) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int pi, tile_p, tile_q;
  tile_of_block(batch, pi, tile_p, tile_q);
  dgrad_direct32_body(batch.prob[pi], tile_p, tile_q, smem);
}
inline hipError_t dgrad_direct32_launch(GemmBatch& b, hipStream_t s) { return direct_launch(gemm_dgrad_direct32<0>, b, 32, 16, 4 * 2 * 64 * 16, s); }

// ---- WGRAD, quadrants: no split-K (round 6 experiment) ---------------------------------------------------
// At minibatches <= 512 the reduction (the rows) is only 256-512 deep; wgrad_direct_body still splits it four ways over the waves
// and pays one LDS pass (64 KB parked, 256 KB read back per workgroup) to add the partial tiles.  Here each wave OWNS a 32 x 32
// quadrant of the 64 x 64 tile over the WHOLE reduction: four accumulators, 8-byte operand loads (two columns per lane), no
// parking, no barrier before the stores.  Same tile map, same db / sum-of-squares outputs (the partial is summed in another
// fixed order); every dW element is ONE chain over the rows instead of four quarter chains.
// Measured against wgrad_direct_body in the test harness (dqnhip_test_gemm mode 2, variant 3): profiles/r06_wgrad_quadrants.txt.
template <int NS = 8>
__device__ __forceinline__ void wgrad_quad_body(const GemmProblem& pr, int tile_p, int tile_q, float* smem) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int wp = wave & 1, wq = wave >> 1;
  const int p0 = tile_p * 64 + wp * 32, q0 = tile_q * 64 + wq * 32;
  const int nst = pr.Kred >> 2;              // steps of 4 rows (lane group lg owns row 4 st + lg)
  const float* pp = pr.P + (size_t)lg * pr.ldp + p0 + li * 2;
  const float* qp = pr.Q + (size_t)lg * pr.ldq + q0 + li * 2;
  const size_t ldp4 = (size_t)4 * pr.ldp, ldq4 = (size_t)4 * pr.ldq;
  const bool want_db = (pr.db != nullptr) && (tile_p == 0) && (wp == 0);
  f32x4 acc[4];     // index qc * 2 + pc
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x2 dbacc = f32x2{0.f, 0.f};
  f32x2 rp[NS], rq[NS];
#define WQ_LOAD(slot, st) { rp[slot] = *reinterpret_cast<const f32x2*>(pp + (size_t)(st) * ldp4); rq[slot] = *reinterpret_cast<const f32x2*>(qp + (size_t)(st) * ldq4); }
#define WQ_COMPUTE(slot)                                                                \
  {                                                                                     \
    dbacc.x += rq[slot].x; dbacc.y += rq[slot].y;                                       \
    _Pragma("unroll") for (int qc = 0; qc < 2; ++qc)                                    \
    _Pragma("unroll") for (int pc = 0; pc < 2; ++pc)                                    \
        acc[qc * 2 + pc] = DQN_MFMA(rp[slot][pc], rq[slot][qc], acc[qc * 2 + pc]);      \
  }
  const int nstN = nst - nst % NS;
  if (nstN > 0) {
#pragma unroll
    for (int i = 0; i < NS; ++i) { WQ_LOAD(i, i) DQN_PIN(); }
    int st = 0;
    for (; st + NS < nstN; st += NS) {
#pragma unroll
      for (int i = 0; i < NS; ++i) { WQ_COMPUTE(i) DQN_PIN(); WQ_LOAD(i, st + NS + i) DQN_PIN(); }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) { WQ_COMPUTE(i) }
  }
  for (int st = nstN; st < nst; ++st) { WQ_LOAD(0, st) WQ_COMPUTE(0) }
#undef WQ_LOAD
#undef WQ_COMPUTE
  // C/D map of acc[qc * 2 + pc]: lane (li, lg), register r = D[i = 4 lg + r][j = li] = dW[n = q0 + 2 li + qc][p = p0 + 2 (4 lg + r) + pc]
  float ssq = 0.0f;
#pragma unroll
  for (int qc = 0; qc < 2; ++qc) {
    const int n = q0 + li * 2 + qc;
    const f32x4 a0 = acc[qc * 2 + 0], a1 = acc[qc * 2 + 1];
    const f32x4 v0 = f32x4{a0.x, a1.x, a0.y, a1.y}, v1 = f32x4{a0.z, a1.z, a0.w, a1.w};     // p = p0 + 8 lg + 0..3, + 4..7
    ssq = fmaf(v0.x, v0.x, ssq); ssq = fmaf(v0.y, v0.y, ssq); ssq = fmaf(v0.z, v0.z, ssq); ssq = fmaf(v0.w, v0.w, ssq);
    ssq = fmaf(v1.x, v1.x, ssq); ssq = fmaf(v1.y, v1.y, ssq); ssq = fmaf(v1.z, v1.z, ssq); ssq = fmaf(v1.w, v1.w, ssq);
    float* c = pr.C + (size_t)n * pr.ldc + p0 + (lg << 3);
    *reinterpret_cast<f32x4*>(c) = v0; *reinterpret_cast<f32x4*>(c + 4) = v1;
  }
  if (want_db) {
    f32x2 v = dbacc;      // add the 4 lane groups (rows m + 0..3)
    v.x += __shfl_xor(v.x, 16, 64); v.y += __shfl_xor(v.y, 16, 64);
    v.x += __shfl_xor(v.x, 32, 64); v.y += __shfl_xor(v.y, 32, 64);
    if (lg == 0) {
      *reinterpret_cast<f32x2*>(pr.db + q0 + li * 2) = v;
      ssq = fmaf(v.x, v.x, ssq); ssq = fmaf(v.y, v.y, ssq);
    }
  }
  if (pr.partial != nullptr) {
    ssq = wave_sum64(ssq);
    if (lane == 0) smem[wave] = ssq;
    __syncthreads();
    if (threadIdx.x == 0) pr.partial[tile_q * pr.tiles_p + tile_p] = (smem[0] + smem[1]) + (smem[2] + smem[3]);
  }
}
template <int NS>
__global__ __launch_bounds__(256) void gemm_wgrad_quad(const GemmBatch batch) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int pi, tile_p, tile_q;
  tile_of_block(batch, pi, tile_p, tile_q);
  wgrad_quad_body<NS>(batch.prob[pi], tile_p, tile_q, smem);
}
template <int NS>
inline hipError_t wgrad_quad_launch(GemmBatch& b, hipStream_t s) { return direct_launch(gemm_wgrad_quad<NS>, b, 64, 64, 64, s); }

}  // namespace dqnhip
