// head_fwd_kernels.hip.h — the head layers' forward kernels and their launcher head_forward<>: the one kernel group that all
// three launching units use (the update, acting, the env front-end).  Templates: a unit embeds the instantiations it names.
#pragma once
#include "learner_internal.hip.h"
#include "update_bodies.hip.h"

namespace dqnhip {

// L1: compiled with the target actor's first-layer epilogue (HeadArgs::l1_*; Step(1) only — the acting path and the critic heads
// instantiate L1 = false and carry neither its 44 registers nor its LDS row)
// The kernel's leading scalar parameters (the idea of GemmPreload, gemm_common.hip.h): head weights, biases and widths of its (up to)
// two heads — what a block's FIRST vector loads, its bias and its NH weight strips, are addressed from — delivered in SGPRs at wave
// launch where the unit is compiled with the kernarg preload option; the panel, the row count and the epilogue's fields still
// come from HeadArgs2, read in those loads' shadow.  flags = 0 (DQNHIP_TUNE_NO_KERNARG_PRELOAD, a width its field cannot hold):
// everything from HeadArgs2 as before, behind one uniform branch.
struct HeadFwdPreload { const float* W0; const float* W1; const float* b0; const float* b1; uint32_t H0, H1, flags; };
#define DQN_HEAD_PRELOAD_PARAMS const float* pre_W0, const float* pre_W1, const float* pre_b0, const float* pre_b1, \
    uint32_t pre_H0, uint32_t pre_H1, uint32_t pre_flags
#define DQN_HEAD_PRELOAD_WORDS(w) (w).W0, (w).W1, (w).b0, (w).b1, (w).H0, (w).H1, (w).flags
inline HeadFwdPreload make_head_preload(const HeadArgs2& a2, bool two, bool off) {
  HeadFwdPreload w{};
  if (off || a2.p[0].H < 1 || (two && a2.p[1].H < 1)) return w;
  w.W0 = a2.p[0].W; w.b0 = a2.p[0].b; w.H0 = (uint32_t)a2.p[0].H;
  if (two) { w.W1 = a2.p[1].W; w.b1 = a2.p[1].b; w.H1 = (uint32_t)a2.p[1].H; }
  w.flags = kPreValid;
  return w;
}
// one head's blocks: W / b / H from either source, the rest from a
template <int NH, int MODE, bool L1>
__device__ __forceinline__ void head_fwd_block(const HeadArgs& a, const float* W, const float* b, const int H) {
  // one block per row (grid-strided when there are more rows than blocks): the 4 waves split K
  // (each lane one float4 strip per 1024 columns), butterfly within the wave, then the 4 wave
  // sums are added in fixed order.  For H <= 1024 the head weights stay in registers across rows.
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __shared__ float s_acc[4][NH];
  const bool hoist = H <= 1024;
  const float bias_j = threadIdx.x < NH ? b[threadIdx.x] : 0.0f;      // requested now, used after the reduction
  f32x4 wreg[NH];
  if (hoist) {
#pragma unroll
    for (int j = 0; j < NH; ++j)
      wreg[j] = (threadIdx.x * 4 < H) ? *reinterpret_cast<const f32x4*>(W + (size_t)j * H + threadIdx.x * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // (l1: this thread's four outputs' action-column weights and biases do not depend on the row)
  constexpr bool kL1 = (L1 && MODE == HEAD_ACTOR && NH == kNO);
  __shared__ float s_mu[kAP];
  float l1w[kL1 ? 4 : 1][kL1 ? kNO : 1];
  f32x4 l1b = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool l1_on = kL1 && a.l1_y != nullptr && (int)threadIdx.x * 4 < a.l1_n;
  if constexpr (kL1) {
    if (l1_on) {
#pragma unroll
      for (int j = 0; j < kNO; ++j) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(a.l1_wt + (size_t)j * a.l1_n + threadIdx.x * 4);
        l1w[0][j] = w4.x; l1w[1][j] = w4.y; l1w[2][j] = w4.z; l1w[3][j] = w4.w;
      }
      l1b = *reinterpret_cast<const f32x4*>(a.l1_b + threadIdx.x * 4);
    }
  }
  for (int row = blockIdx.x; row < a.rows; row += gridDim.x) {
    float acc[NH];
#pragma unroll
    for (int j = 0; j < NH; ++j) acc[j] = 0.0f;
    const size_t x0 = (size_t)row * a.ldx;
    f32x4 zs = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (kL1) { if (l1_on) zs = *reinterpret_cast<const f32x4*>(a.l1_zs + (size_t)row * a.l1_ld + threadIdx.x * 4); }
    auto dots = [&](auto tag) {
      for (int k = threadIdx.x * 4; k < H; k += 1024) {
        const f32x4 xv = head_ld4t<decltype(tag)::value>(a.X, a.X16, x0 + k);
#pragma unroll
        for (int j = 0; j < NH; ++j) {
          const f32x4 wv = hoist ? wreg[j] : *reinterpret_cast<const f32x4*>(W + (size_t)j * H + k);
          acc[j] = fmaf(xv.x, wv.x, acc[j]); acc[j] = fmaf(xv.y, wv.y, acc[j]);
          acc[j] = fmaf(xv.z, wv.z, acc[j]); acc[j] = fmaf(xv.w, wv.w, acc[j]);
        }
      }
    };
    HEAD_DISPATCH(a.X16 != nullptr, dots);
#pragma unroll
    for (int j = 0; j < NH; ++j) {
      acc[j] = wave_sum64(acc[j]);
      if (lane == 0) s_acc[wave][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < kAP) {
      const int j = threadIdx.x;
      float v = 0.0f;
      if (j < NH) v = ((s_acc[0][j] + s_acc[1][j]) + (s_acc[2][j] + s_acc[3][j])) + bias_j;
      if constexpr (MODE == HEAD_ACTOR) {
        a.out16[(size_t)row * kAP + j] = v;
        if (a.xc != nullptr && j < NH) a.xc[(size_t)row * a.ldxc + a.xc_col + j] = v;
        if (a.xc16 != nullptr && j < NH) a.xc16[(size_t)row * a.ldxc16 + a.xc_col + j] = (_Float16)v;
        if constexpr (kL1) s_mu[j] = v;
      } else {
        if (j == 0) {
          a.q[row] = v;
          if constexpr (MODE == HEAD_Q_POLICY) a.qsum_partial[row] = (double)v;   // summed in row order by k_tick / k_tails
        }
      }
    }
    __syncthreads();                       // s_acc is rewritten by the next row
    if constexpr (kL1) {
      if (a.l1_y != nullptr) {             // (uniform)
        if (l1_on) {
          float o[4] = {zs.x, zs.y, zs.z, zs.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int j = 0; j < kNO; ++j) o[e] = fmaf(l1w[e][j], s_mu[j], o[e]);
          }
          f32x4 y;
          y.x = lrelu_fwd(o[0] + l1b.x); y.y = lrelu_fwd(o[1] + l1b.y); y.z = lrelu_fwd(o[2] + l1b.z); y.w = lrelu_fwd(o[3] + l1b.w);
          *reinterpret_cast<f32x4*>(a.l1_y + (size_t)row * a.l1_ld + threadIdx.x * 4) = y;
        }
        __syncthreads();                   // s_mu is rewritten by the next row
      }
    }
  }
}
template <int NH, int MODE, bool L1 = false>
__global__ __launch_bounds__(256) void k_head_fwd(DQN_HEAD_PRELOAD_PARAMS, HeadArgs2 a2) {
  const HeadArgs& a = a2.p[blockIdx.y];
  if (!(pre_flags & kPreValid)) { head_fwd_block<NH, MODE, L1>(a, a.W, a.b, a.H); return; }
  const bool second = blockIdx.y != 0;
  head_fwd_block<NH, MODE, L1>(a, second ? pre_W1 : pre_W0, second ? pre_b1 : pre_b0, (int)(second ? pre_H1 : pre_H0));
}

// (Round 4: a form with the head weights staged once per block in LDS, 16 rows per block, all of a wave's rows in flight
// at once was built and measured — 13.4 us against 12.5 for two 4096-row fp16 passes, no change at 2048 fp32 rows: the
// per-wave weight reload is not what this kernel waits for; it streams its panel at ~2.7 TB/s either way.  Not kept.)
// Large minibatches (rows >= 1024): one WAVE per row, no block-level synchronisation; the head weights
// stay in registers across the rows of a wave (H <= 1024: NH x 4 float4 per lane).
template <int NH, int MODE>
__global__ __launch_bounds__(256) void k_head_fwd_rows(HeadArgs2 a2) {
  const HeadArgs& a = a2.p[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // a lane's four float4 strips of a row: fp32 panel k = 4 lane + 256 t (16-B loads); fp16 panel k = 8 lane + 512 (t / 2)
  // + 4 (t % 2), i.e. two 16-B loads of eight halves each (8-B loads run at about half the rate per byte)
  const bool in16 = a.X16 != nullptr;
  auto kof = [&](int t) { return in16 ? lane * 8 + 512 * (t >> 1) + 4 * (t & 1) : lane * 4 + 256 * t; };
  f32x4 wreg[NH][4];
#pragma unroll
  for (int j = 0; j < NH; ++j)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = kof(t);
      wreg[j][t] = k < a.H ? *reinterpret_cast<const f32x4*>(a.W + (size_t)j * a.H + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  // the next row of this wave is fetched while the current one is reduced (the loop was one exposed memory latency
  // per row: 4 rows per wave at 4096 rows)
  auto load_row = [&](int row, f32x4 (&v)[4]) {
    const size_t x0 = (size_t)row * a.ldx;
    if (in16) {
      typedef __attribute__((ext_vector_type(8))) _Float16 h8;
      h8 u[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int k = lane * 8 + 512 * q;
        if (k < a.H) u[q] = *reinterpret_cast<const h8*>(a.X16 + x0 + k);
        else { for (int e = 0; e < 8; ++e) u[q][e] = (_Float16)0.f; }
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        v[2 * q] = f32x4{(float)u[q][0], (float)u[q][1], (float)u[q][2], (float)u[q][3]};
        v[2 * q + 1] = f32x4{(float)u[q][4], (float)u[q][5], (float)u[q][6], (float)u[q][7]};
      }
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = lane * 4 + 256 * t;
        v[t] = k < a.H ? *reinterpret_cast<const f32x4*>(a.X + x0 + k) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  };
  const int row_step = gridDim.x * 4;
  const float bias_l = lane < NH ? a.b[lane] : 0.0f;   // once: inside the row loop the stores keep it from being hoisted
  f32x4 xn[4];
  if ((int)(blockIdx.x * 4 + wave) < a.rows) load_row(blockIdx.x * 4 + wave, xn);
  for (int row = blockIdx.x * 4 + wave; row < a.rows; row += row_step) {
    f32x4 xv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) xv[t] = xn[t];
    if (row + row_step < a.rows) load_row(row + row_step, xn);
    float acc[NH];
#pragma unroll
    for (int j = 0; j < NH; ++j) {
      float s = 0.0f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        s = fmaf(xv[t].x, wreg[j][t].x, s); s = fmaf(xv[t].y, wreg[j][t].y, s);
        s = fmaf(xv[t].z, wreg[j][t].z, s); s = fmaf(xv[t].w, wreg[j][t].w, s);
      }
      acc[j] = wave_sum64(s);
    }
    if (lane < kAP) {
      float v = 0.0f;
#pragma unroll
      for (int j = 0; j < NH; ++j) if (lane == j) v = acc[j] + bias_l;
      if constexpr (MODE == HEAD_ACTOR) {
        a.out16[(size_t)row * kAP + lane] = v;
        if (a.xc != nullptr && lane < NH) a.xc[(size_t)row * a.ldxc + a.xc_col + lane] = v;
        if (a.xc16 != nullptr && lane < NH) a.xc16[(size_t)row * a.ldxc16 + a.xc_col + lane] = (_Float16)v;
      } else {
        if (lane == 0) {
          a.q[row] = v;
          if constexpr (MODE == HEAD_Q_POLICY) a.qsum_partial[row] = (double)v;
        }
      }
    }
  }
}

}  // namespace dqnhip

namespace dqnhip_host {

template <int NH, int MODE>
int head_forward(H* h, hipStream_t st, const HeadArgs& a, const HeadArgs* b = nullptr) {
  HeadArgs2 a2{}; a2.p[0] = a; if (b) a2.p[1] = *b;
  // (single-head: the block-per-row form measured faster, 6.6 vs 8.8 us.  Chosen at compile time, so that no unit embeds a
  // k_head_fwd_rows<1, .> that nothing launches)
  if constexpr (NH > 1) {
    if (a.rows >= 1024 && a.H <= 1024 && a.H % 4 == 0) {
      HIPCHK(launch(st, k_head_fwd_rows<NH, MODE>, dim3(256, b ? 2 : 1), dim3(256), 0, a2));
      return 0;
    }
  }
  const HeadFwdPreload w = make_head_preload(a2, b != nullptr, (h->cfg.tuning_flags & DQNHIP_TUNE_NO_KERNARG_PRELOAD) != 0);
  if (a.l1_y != nullptr || (b && b->l1_y != nullptr))      // Step(1): the target actor's head also finishes critic_target's first layer
    HIPCHK(launch(st, k_head_fwd<NH, MODE, true>, dim3(std::min(a.rows, 1024), b ? 2 : 1), dim3(256), 0, DQN_HEAD_PRELOAD_WORDS(w), a2));
  else
    HIPCHK(launch(st, k_head_fwd<NH, MODE, false>, dim3(std::min(a.rows, 1024), b ? 2 : 1), dim3(256), 0, DQN_HEAD_PRELOAD_WORDS(w), a2));
  return 0;
}

}  // namespace dqnhip_host
