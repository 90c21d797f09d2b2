// gemm_common.hip.h — the bottom of the argument layer (learner_args.hip.h has the map of the kernel headers): the GEMM problem
// descriptions, where a launch goes (LaunchOn / launch), and the few device helpers every kernel group uses (leaky ReLU, the wave
// sum, the tails block).  Shared by the fp32 MFMA GEMM family (gemm_bodies.hip.h, gemm_direct.hip.h), the fp16 family (hgemm.hip.h)
// and the head / optimiser / replay kernels.
//
// Every tower GEMM computes C[q][p] = sum_k Pop(p,k) * Qop(q,k) with `p` the contiguous
// output dimension; the three modes replace the Caffe InnerProduct forward/backward GEMMs
// the reference reaches from src/dqn.cpp:751, 904, 923, 963, 1013:
//
//   FWD   Y[m][n]  = lrelu(sum_k X[m][k] W[n][k] + b[n])         P=W  Q=X
//   DGRAD dX[m][j] = (sum_n dY[m][n] W[n][j]) * lrelu'(Xp[m][j])  P=W  Q=dY
//   WGRAD dW[n][j] = sum_m dY[m][n] X[m][j] ; db[n] = sum_m dY[m][n]   P=X  Q=dY
//
// with the ReLU(negative_slope=0.01) forward/backward (src/dqn.cpp:292-301) fused into the
// epilogues.  A launch may carry up to 4 independent problems (grouped GEMM).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

namespace dqnhip {

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum GemmMode { GEMM_FWD = 0, GEMM_DGRAD = 1, GEMM_WGRAD = 2 };

constexpr float kLeakySlope = 0.01f;  // src/dqn.cpp:300

struct GemmProblem {
  const float* P; int ldp;   // operand that indexes the contiguous output dim
  const float* Q; int ldq;   // operand that indexes the output rows
  float* C; int ldc;         // C[q*ldc + p]
  int Pdim, Qdim, Kred;      // Pdim % BP == 0, Qdim % BQ == 0
  const float* bias;         // FWD: bias[p] (may be null)
  const float* mask; int ldm;// DGRAD: previous activation [q][p] for lrelu' (null: none)
  float* db;                 // WGRAD: bias gradient [q] (null: skip)
  float* partial;            // WGRAD: one sum-of-squares partial per tile (null: skip)
  int relu;                  // FWD: apply leaky ReLU
  // FWD, top tower layer of the critic(s, mu(s)) pass: the epilogue also writes the seed of BackwardFrom(q_values_layer)
  // (src/dqn.cpp:918-923: q diff = -1 per row) taken through the head and this layer's ReLU,
  // C2[q][p] = (-seed_w[p]) * lrelu'(C[q][p]) — what a head-backward launch of its own used to compute from C (null: none)
  const float* seed_w; float* C2;
  // FWD, top tower layer of a critic pass of Step(1): the epilogue also leaves the head's dot product in pieces,
  // dot_out[q][p / 16] = sum over the 16 finished activations C[q][p .. p+15] of C * dot_w (fixed order: a lane's four columns
  // as an fma chain from 0, then (g0 + g1) + (g2 + g3) over the four lane groups) — k_dgrad_qtrain sums the Pdim / 16 pieces of a row
  const float* dot_w; float* dot_out;
  // FWD (first_layers_launch, the state half of critic_target's first layer): the workgroups also leave (column j: row tile j mod tiles_q) columns
  // [xcopy_col, +xcopy_n) of their 16 TP rows of P transposed, xcopy_dst[j][p] = P[p][xcopy_col + j] (the action-column weights the
  // target actor's head kernel applies: there one coalesced float4 per action instead of 40 strided dwords per thread); null: none
  float* xcopy_dst; int xcopy_col, xcopy_n;
  int mode;                  // mixed-mode launches (gemm_bwd_pair_direct): GEMM_DGRAD / GEMM_WGRAD
  int tiles_p, tiles_q, tile_base;
};

// The bodies address an operand as a wave-uniform 64-bit base plus ONE 32-bit byte offset per lane: at most 15 rows and 60 floats
// into the operand, (15 ld + 60) * 4 + 16 <= 2^32.  gemm_form_accepts and pack_args refuse a larger leading dimension (the
// product's are the tower widths, at most a few thousand); tests/cpp/tile_decode_host.cpp checks both sides of the bound.
constexpr int kMaxLeadingDim = 1 << 26;
constexpr int kMaxGroup = 4;
struct GemmBatch {
  GemmProblem prob[kMaxGroup];
  int n;
  int total_tiles;
};

// ---- what the fp32 GEMM kernels receive ----------------------------------------------------------------------------------------
// GemmBatch stays the host-side description; its launcher packs it (pack_args, gemm_direct.hip.h) into a GemmArgs laid out by when
// a wave needs each field.  A wave's first operand load used to wait for five dependent scalar loads of the 640-byte GemmBatch
// (tile_base, then tiles_p / tiles_q of prob[pi], ... then P / Q of prob[pi]); with this layout everything the first load needs is
// requested at constant kernarg offsets in ONE round: the header (first 64 bytes) and the hot record of every problem; a uniform
// branch on the block index then takes the record of the workgroup's problem (problem_of_tile).  The cold record (epilogue fields)
// is indexed by pi, so its request goes out after that round and nothing waits for it before the operand loads are in flight.
struct alignas(64) GemmHeader {
  int tile_base[kMaxGroup];    // entries >= n: INT_MAX (so the problem search needs no `n`)
  int tiles_p[kMaxGroup], tiles_q[kMaxGroup];
  int n, total_tiles, pad[2];
};
struct alignas(64) GemmHot {   // one 64-byte line; what every body's first loads need comes first, in whole 16-byte pieces
  const float* P; const float* Q;
  int ldp, ldq, Kred, ldc;
  float* C;
  int mode;                    // (mixed-mode launches choose their body by it)
  int Pdim, Qdim;
  uint32_t tq_magic;           // ceil(2^31 / tiles_q): the tile decode's division as one multiply (tile_decode, gemm_bodies.hip.h); with
                               // the record, not in the header: four problems need four and the header has two spare words
  int pad[2];
};
struct GemmCold {
  const float* bias; const float* mask; float* db; float* partial;
  const float* seed_w; float* C2; const float* dot_w; float* dot_out; float* xcopy_dst;
  int ldm, relu, xcopy_col, xcopy_n;
};
// N: the records the kernel carries (kMaxGroup for the grouped kernels; the kernels with a fixed number of problems carry — and
// index — exactly theirs)
template <int N>
struct GemmArgs {
  GemmHeader head;
  GemmHot hot[N];
  GemmCold cold[N];
};
static_assert(sizeof(GemmHeader) == 64 && sizeof(GemmHot) == 64, "one 16-dword scalar load each");

// ---- the kernarg preload block -------------------------------------------------------------------------------------------------
// gfx950 delivers a kernel's first (up to) 14 kernarg dwords in SGPRs at wave launch — leading SCALAR parameters only, a struct is
// never preloaded.  The chain kernels therefore take these 14 dwords as leading scalar parameters in front of their GemmArgs:
// what a workgroup needs to form the addresses of its first operand loads and nothing else, so that those loads issue without a
// scalar wait in front of them; everything else still comes from the GemmArgs behind them, requested in the loads' shadow.
// The host derives the block from a packed GemmArgs (make_preload_*, gemm_direct.hip.h); GemmArgs itself is unchanged.
//   one problem            P0 / Q0, one set of ldp / ldq / Kred / tile counts / magic; no split
//   two of equal shape     P0 / Q0 / P1 / Q1, ONE set of the rest; tiles b >= split are problem 1's
//   one record             P0 / Q0 and the rest of ONE record of a two-tile kernel; in place of the split its first block
//   anything else          flags = 0: the kernel takes the GemmArgs path as it was, behind one uniform branch
struct GemmPreload {
  const float* P0; const float* Q0; const float* P1; const float* Q1;
  uint32_t ldp, ldq, Kred;
  uint32_t tiles;              // tiles_p | tiles_q << kPreTilesQShift
  uint32_t magic;              // tile_magic(tiles_q)
  uint32_t flags;              // kPreValid | (split or first block) << kPreSplitShift
};
static_assert(sizeof(GemmPreload) == 14 * 4, "16 user SGPRs less the kernarg pointer");
constexpr uint32_t kPreValid = 1;
constexpr int kPreSplitShift = 2, kPreTilesQShift = 20;
constexpr uint32_t kPreNoSplit = (1u << (32 - kPreSplitShift)) - 1;      // one problem: no block index reaches it
// the kernels' leading parameters / the words of a GemmPreload in a launch's argument list, in the struct's order
#define DQN_PRELOAD_PARAMS const float* pre_P0, const float* pre_Q0, const float* pre_P1, const float* pre_Q1, \
    uint32_t pre_ldp, uint32_t pre_ldq, uint32_t pre_Kred, uint32_t pre_tiles, uint32_t pre_magic, uint32_t pre_flags
#define DQN_PRELOAD_WORDS(pre) (pre).P0, (pre).Q0, (pre).P1, (pre).Q1, (pre).ldp, (pre).ldq, (pre).Kred, (pre).tiles, (pre).magic, (pre).flags
#define DQN_PRELOAD_BLOCK GemmPreload{pre_P0, pre_Q0, pre_P1, pre_Q1, pre_ldp, pre_ldq, pre_Kred, pre_tiles, pre_magic, pre_flags}

// Where ONE kernel launch goes: a stream and, in the learner's timing mode, the event pair that brackets it.  Every launcher takes a
// LaunchOn where it would take a stream (a bare hipStream_t converts: untimed) and hands it to exactly one launch().
struct LaunchOn {
  hipStream_t stream;
  hipEvent_t start = nullptr, stop = nullptr;
  bool no_preload = false;         // DQNHIP_TUNE_NO_KERNARG_PRELOAD: the launch's GemmPreload is marked "not valid" (A/B in one binary)
  LaunchOn(hipStream_t s) : stream(s) {}
  LaunchOn(hipStream_t s, hipEvent_t t0, hipEvent_t t1) : stream(s), start(t0), stop(t1) {}
};
// The one place a kernel is launched from.  With events: hipExtLaunchKernelGGL, which stamps them with the dispatch packet's own
// start / stop timestamps — the kernel duration rocprofv3 reports, without the cost of separate event records.
template <typename K, typename... A>
inline hipError_t launch(const LaunchOn& on, K kernel, dim3 grid, dim3 block, size_t lds, const A&... args) {
  if (on.start) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, on.stream, on.start, on.stop, 0, args...);
  else hipLaunchKernelGGL(kernel, grid, block, lds, on.stream, args...);
  return hipGetLastError();
}

__device__ __forceinline__ float lrelu_fwd(float x) {
  // Caffe ReLULayer::Forward: max(x,0) + slope*min(x,0)
  return fmaxf(x, 0.0f) + kLeakySlope * fminf(x, 0.0f);
}
__device__ __forceinline__ float lrelu_mask(float y) {
  // Caffe ReLULayer::Backward (in-place: bottom_data is the output y)
  return (y > 0.0f ? 1.0f : 0.0f) + kLeakySlope * (y <= 0.0f ? 1.0f : 0.0f);
}

// Sum over the 64 lanes of a wave with DPP moves (VALU speed) instead of six ds_bpermute butterfly steps: quad
// xor 1, xor 2, half-row mirror, row mirror give every lane its 16-lane row total; row_bcast15 / row_bcast31 chain
// the four row totals into lane 63, which is broadcast.  (Ten heads x six dependent LDS-crossbar shuffles were
// ~2.5 us per row in the one-wave-per-row head kernels.)  Order: fixed, the same in every wave.
__device__ __forceinline__ float wave_sum64(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xC, 0xF, false));
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// sticky device flags (DevState::flags, learner_args.hip.h)
constexpr int kFlagTarget = 1;     // a TD target of the last update(s) was not finite
constexpr int kFlagGradNorm = 2;   // a gradient L2 norm was not finite: that clip+Adam step was skipped

// Dynamic loss scaling (DevState::ls_mult, learner_args.hip.h): a static loss scale times the live multiplier, or the reciprocal of
// one times the reciprocal of the other.  Null: static mode, the immediate as it is and no load.
__device__ __forceinline__ float ls_live(float base, const float* mult) { return mult != nullptr ? base * *mult : base; }

// Data-parallel learners: the per-block loss / q partials reduced into the 4-float tails that ride in the gradient exchange
// ([loss_sum, q_sum, target flag, 0]; tail[2] carries this rank's non-finite-target flag: it is raised from the rank's OWN replay
// shard, so without it one rank would stop with "Target not finite!" while the others walk into the next collective).
// One block of 256 threads, the reduction tree of tick_body (strided partials, butterfly, fixed cross-wave order).  A launch of its
// own (k_tails) or — round 6 — ONE extra block of the net's last backward launch (everything it reads is complete launches earlier).
struct TailsArgs {
  const float* loss_partial; int n_loss; const double* q_partial; int n_q;
  float inv_batch; float* critic_tail; float* actor_tail; const int* flags;
  int on;                          // rider form: not 0 = the launch's last block runs tails_block (gemm_wgrad_tail: that block's index + 1)
};
__device__ __forceinline__ void tails_block(const TailsArgs& a, float* sdot /*[4]*/, double* sq /*[4]*/) {
  const int t = threadIdx.x;
  float dot = 0.0f; double qs = 0.0;
  if (a.critic_tail != nullptr) for (int i = t; i < a.n_loss; i += 256) dot += a.loss_partial[i];
  if (a.actor_tail != nullptr) for (int i = t; i < a.n_q; i += 256) qs += a.q_partial[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { dot += __shfl_xor(dot, off, 64); qs += __shfl_xor(qs, off, 64); }
  if ((t & 63) == 0) { sdot[t >> 6] = dot; sq[t >> 6] = qs; }
  __syncthreads();
  if (t != 0) return;
  if (a.critic_tail != nullptr) {
    dot = (sdot[0] + sdot[1]) + (sdot[2] + sdot[3]);
    a.critic_tail[0] = dot * a.inv_batch / 2.0f;   // EuclideanLoss: dot / num / 2
    a.critic_tail[1] = 0.f; a.critic_tail[2] = (*a.flags & kFlagTarget) ? 1.0f : 0.f; a.critic_tail[3] = 0.f;
  }
  if (a.actor_tail != nullptr) {
    qs = (sq[0] + sq[1]) + (sq[2] + sq[3]);
    a.actor_tail[0] = 0.f; a.actor_tail[1] = (float)qs; a.actor_tail[2] = 0.f; a.actor_tail[3] = 0.f;
  }
}

}  // namespace dqnhip
