// gemm_direct.hip.h — "direct-to-register, split-K-across-waves" fp32 MFMA GEMMs
// for the small-M (minibatch 32..4096) layers of the actor/critic towers.
//
// Why a second family: at M = 256 a 1024x1024 layer is only 0.54 GFLOP.  An
// LDS-staged tile kernel (gemm_mfma.hip.h) needs one workgroup barrier per K
// tile and can only offer 128-256 workgroups; measured 16-25 us per layer
// (profiles/r01_v1_*).  Here instead:
//   * every output tile is computed by ONE workgroup of 4 waves, each wave
//     accumulating the WHOLE tile over its own quarter of the reduction
//     range (in-workgroup split-K).  The waves never synchronise in the main
//     loop — four independent load->MFMA pipelines per CU, one per SIMD;
//   * operands go global/L2 -> VGPR directly in MFMA fragment layout with
//     16-byte loads, no LDS round trip: a "k-contiguous" operand (KC) is read
//     as float4 along k (4 consecutive k-steps of one row per lane); a
//     "k-strided" operand (KS) is read as float4 along the free dimension
//     (whole 256-B rows per 16 lanes) and its four components feed four
//     interleaved MFMAs (output columns 4i+c);
//   * a 4-deep register ring keeps >= 2048 MFMA-cycles of loads in flight;
//   * one LDS pass at the end adds the four waves' partial tiles in fixed order
//     (w0+w1)+(w2+w3) -> deterministic, no atomics; the epilogue (bias +
//     leaky ReLU / ReLU' mask / bias-gradient + sum-of-squares partial) is
//     applied by the wave that reduces the accumulator.
// The smallest tiles (32x32 fwd, 64x16 dgrad, 64x64 wgrad) give 256
// workgroups for ONE 256x1024x1024 layer, i.e. a single layer fills the chip.
//
// Same GemmProblem/GemmBatch interface and the same three modes as
// gemm_mfma.hip.h (C[q][p] = sum_k P(p,k) Q(q,k), p contiguous).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "gemm_bodies.hip.h"
#include "gemm_plan.hip.h"         // GemmForm, gemm_form_accepts

namespace dqnhip {

// ---- kernels: thin wrappers over the bodies --------------------------------------------
template <int TP, int TQ>
__global__ __launch_bounds__(256) void gemm_fwd_direct(const GemmArgs<kMaxGroup> args) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int tile_p, tile_q;
  const GemmProblem pr = problem_of_block(args, tile_p, tile_q);
  fwd_direct_body<TP, TQ>(pr, tile_p, tile_q, smem);
}
template <int TP, int TQ, bool PIN, int NSLOT = 2>
__global__ __launch_bounds__(256) void gemm_fwd_lds(DQN_PRELOAD_PARAMS, const GemmArgs<kMaxGroup> args) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int tile_p, tile_q;
  if (!(pre_flags & kPreValid)) {          // not a form the preload block expresses (or switched off): the GemmArgs path as it was
    const GemmProblem pr = problem_of_block(args, tile_p, tile_q);
    fwd_lds_body<TP, TQ, PIN, NSLOT>(pr, tile_p, tile_q, smem);
    return;
  }
  const GemmProblem pr = problem_of_preload(DQN_PRELOAD_BLOCK, args, (int)blockIdx.x, tile_p, tile_q);
  fwd_lds_body<TP, TQ, PIN, NSLOT>(pr, tile_p, tile_q, smem);
}
template <int TPB, int TQ>
__global__ __launch_bounds__(256) void gemm_dgrad_direct(const GemmArgs<kMaxGroup> args) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int tile_p, tile_q;
  const GemmProblem pr = problem_of_block(args, tile_p, tile_q);
  dgrad_direct_body<TPB, TQ>(pr, tile_p, tile_q, smem);
}
template <int TPB, int TQ, bool SCH = true>
__device__ __forceinline__ void dgrad_lds_body(const GemmProblem& pr, int tile_p, int tile_q, float* smem) {
  DgradNoHook none;
  dgrad_lds_body<TPB, TQ, SCH, DgradNoHook>(pr, tile_p, tile_q, smem, nullptr, none);
}
template <int TPB, int TQ>
__global__ __launch_bounds__(256) void gemm_dgrad_lds(DQN_PRELOAD_PARAMS, const GemmArgs<kMaxGroup> args) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int tile_p, tile_q;
  if (!(pre_flags & kPreValid)) {
    const GemmProblem pr = problem_of_block(args, tile_p, tile_q);
    dgrad_lds_body<TPB, TQ>(pr, tile_p, tile_q, smem);
    return;
  }
  const GemmProblem pr = problem_of_preload(DQN_PRELOAD_BLOCK, args, (int)blockIdx.x, tile_p, tile_q);
  dgrad_lds_body<TPB, TQ>(pr, tile_p, tile_q, smem);
}
template <int TPB, int TQB>
__global__ __launch_bounds__(256) void gemm_wgrad_direct(const GemmArgs<kMaxGroup> args) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int tile_p, tile_q;
  const GemmProblem pr = problem_of_block(args, tile_p, tile_q);
  wgrad_direct_body<TPB, TQB>(pr, tile_p, tile_q, smem);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void gemm_dgrad_narrow(const GemmArgs<kMaxGroup> args) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int tile_p, tile_q;
  const GemmProblem pr = problem_of_block(args, tile_p, tile_q);
  dgrad_narrow_body(pr, tile_p, tile_q, smem);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void gemm_dgrad_narrow_qrider(const GemmArgs<kMaxGroup> args, const QHeadRider rider) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  HotArgs<kMaxGroup> r;
  const int b = request_args(args, r, (int)blockIdx.x, args.head.total_tiles);
  if (b >= r.hd.total_tiles) { q_head_rider(rider, b - r.hd.total_tiles); return; }
  int tile_p, tile_q;
  const GemmProblem pr = problem_of_tile(args, r, b, tile_p, tile_q);
  dgrad_narrow_body(pr, tile_p, tile_q, smem);
}
template <int TPB>
__global__ __launch_bounds__(256) void gemm_wgrad_narrow(const GemmArgs<kMaxGroup> args) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int tile_p, tile_q;
  const GemmProblem pr = problem_of_block(args, tile_p, tile_q);
  wgrad_narrow_body<TPB>(pr, tile_p, tile_q, smem);
}
// One layer's backward in ONE launch: problems with mode GEMM_DGRAD (64x16 tiles) and
// GEMM_WGRAD (64x64 tiles) side by side.  dX_{l-1} = dZ_l W_l and dW_l = dZ_l^T X_{l-1} only
// share their input dZ_l, so a 256x1024x1024 layer offers 256 + 256 workgroups = 2 per CU.
template <int TQD = 1, bool DLDS = false>
__global__ __launch_bounds__(256) void gemm_bwd_pair_direct(const GemmArgs<kMaxGroup> args) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int tile_p, tile_q;
  const GemmProblem pr = problem_of_block(args, tile_p, tile_q);
  if (pr.mode == GEMM_WGRAD) wgrad_direct_body<1, 1>(pr, tile_p, tile_q, smem);
  else if constexpr (DLDS) dgrad_lds_body<1, TQD, false>(pr, tile_p, tile_q, smem);   // (scheduled form measured 0.5 us slower beside the co-resident wgrad wave)
  else dgrad_direct_body<1, TQD>(pr, tile_p, tile_q, smem);
}

// The same layer backward with ONE workgroup type: workgroup b computes wgrad tile b and then dgrad
// tile b in one instruction stream (prob[0] = dgrad, prob[1] = wgrad).  Two co-resident workgroups
// per CU measured ~ the SUM of their stand-alone times (the pair kernel above: 15.5 us for 2 x 4.2 us
// of MFMA); one workgroup doing both pays the per-launch fixed cost once and keeps one wave per SIMD.
template <bool DLDS>
__device__ __forceinline__ void bwd_seq_block(const GemmArgs<2>& args, const int block, float* smem) {
  int tile_p, tile_q;
  HotArgs<2> r;
  const int b = request_args(args, r, block);
  // wgrad first (measured 14.9 us; dgrad first 15.3, also with the wgrad ring pre-issued under the
  // dgrad epilogue; round 5: wgrad first with the dgrad tile's first operand requests issued BEFORE the wgrad tile parks /
  // reduces / stores — 15.0-15.1 against 14.7 us; the same requests issued before the WHOLE wgrad tile — 14.9: three cold loads
  // in flight do not pay for the registers and wait counts they hold through the other tile)
  const GemmProblem pw = problem_at<1>(args, r);
  if (b < pw.tiles_p * pw.tiles_q) {
    tile_of_record<1>(r, b, tile_p, tile_q);
    wgrad_direct_body<1, 1>(pw, tile_p, tile_q, smem);
  }
  __syncthreads();
  const GemmProblem pd = problem_at<0>(args, r);
  if (b < pd.tiles_p * pd.tiles_q) {
    tile_of_record<0>(r, b, tile_p, tile_q);
    if constexpr (DLDS) dgrad_lds_body<1, 1, true>(pd, tile_p, tile_q, smem);
    else dgrad_direct_body<1, 1>(pd, tile_p, tile_q, smem);
  }
}
template <bool DLDS>
__global__ __launch_bounds__(256) void gemm_bwd_seq(const GemmArgs<2> args) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  bwd_seq_block<DLDS>(args, (int)blockIdx.x, smem);
}

// The carrier is the FIRST tower layer's narrow wgrad launch (the last launch before the optimiser pass): 64-128 tiles, so the rider
// blocks land on CUs of their own instead of beside a GEMM wave (as riders of the top layer's gemm_bwd_seq: +0.9 us on that launch)
template <int NH>
__global__ __launch_bounds__(256) void gemm_wgrad_narrow_rider(const GemmArgs<kMaxGroup> args, const HeadWgradRider rider) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  HotArgs<kMaxGroup> r;
  const int b = request_args(args, r, (int)blockIdx.x, rider.blocks);
  if (b < rider.blocks) { head_wgrad_rider<NH>(rider, b, smem); return; }
  int tile_p, tile_q;
  const GemmProblem pr = problem_of_tile(args, r, b - rider.blocks, tile_p, tile_q);
  wgrad_narrow_body<1>(pr, tile_p, tile_q, smem);
}

// The LAST launch of a net's backward under the shifted schedule (learner.hip tower_backward): layer 1's wgrad (prob[0]:
// 64 x 64 tiles), the first layer's narrow wgrad (prob[1]: 16-output tiles) and the head's dW / db rider blocks.  The
// first layer's wgrad alone is 64-128 short workgroups — a 6-us launch of launch floor; beside a full wgrad it costs ~1.
// Grid order: the rider blocks, the narrow tiles, the 64 x 64 tiles, the tails block (the long workgroups first measured the same,
// profiles/r06_wgrad_tail_order.txt); the preloaded path below depends on it through the first-block word.
template <int NH>
__global__ __launch_bounds__(256) void gemm_wgrad_tail(DQN_PRELOAD_PARAMS, const GemmArgs<2> args, const HeadWgradRider rider, const TailsArgs tails) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (pre_flags & kPreValid) {
    // The preloaded words are the 64 x 64 wgrad's record: its workgroups are the long ones.  They come behind the rider blocks and
    // the narrow tiles, from the block the words name on; every other block — the riders, the narrow tiles, the tails block behind
    // the last tile — takes the scalar path below.
    const PreRecordTile t = preload_record_decode(DQN_PRELOAD_BLOCK, (int)blockIdx.x);
    if (t.mine) {
      const GemmProblem p1 = record_of_preload<0>(DQN_PRELOAD_BLOCK, args, t);
      wgrad_direct_body<1, 1>(p1, t.tile_p, t.tile_q, smem);
      return;
    }
  }
  HotArgs<2> r;
  int blk = request_args(args, r, (int)blockIdx.x, tails.on, rider.blocks);
  int tile_p, tile_q;
  if (tails.on && blk == tails.on - 1) { tails_block(tails, smem, reinterpret_cast<double*>(smem + 8)); return; }   // data-parallel learners: one more block, last in the grid
  if (blk < rider.blocks) { head_wgrad_rider<NH>(rider, blk, smem); return; }
  blk -= rider.blocks;
  const int n0 = r.hd.tiles_p[1] * r.hd.tiles_q[1];
  if (blk < n0) { const GemmProblem p0 = problem_at<1>(args, r); tile_of_record<1>(r, blk, tile_p, tile_q); wgrad_narrow_body<1>(p0, tile_p, tile_q, smem); return; }
  blk -= n0;
  const GemmProblem p1 = problem_at<0>(args, r);
  tile_of_record<0>(r, blk, tile_p, tile_q); wgrad_direct_body<1, 1>(p1, tile_p, tile_q, smem);
}

// ---- launchers ------------------------------------------------------------------------
// Each fills the tile accounting of its problems and makes ONE launch() on the LaunchOn it is handed (gemm_common.hip.h).
// Dynamic-LDS sizes have a name next to their launcher; direct_prepare_all() raises the limit of those above 64 KB.

constexpr int kBwdTileLds = 4 * 16 * 64 * 16 + 4 * 16 * 16;   // the 64 x 64 backward tile: 64 KB of operand panels + 1 KB of bias-gradient partials
constexpr int kWgradTailLdsMax = 80 * 1024;                   // gemm_wgrad_tail with its head rider: still two workgroups per CU

// tiles of BP x BQ for every problem of the batch; returns (and stores) their number
inline int tile_batch(GemmBatch& batch, int BP, int BQ) {
  int base = 0;
  for (int i = 0; i < batch.n; ++i) {
    GemmProblem& p = batch.prob[i];
    p.tiles_p = p.Pdim / BP;
    p.tiles_q = p.Qdim / BQ;
    p.tile_base = base;
    base += p.tiles_p * p.tiles_q;
  }
  return batch.total_tiles = base;
}
template <typename K>
inline hipError_t direct_launch(K kernel, GemmBatch& batch, int BP, int BQ, int lds_bytes, const LaunchOn& on) {
  return launch(on, kernel, dim3(tile_batch(batch, BP, BQ)), dim3(256), lds_bytes, batch);
}
// What the product's kernels receive: the GemmArgs of a batch whose tile accounting is filled (gemm_common.hip.h).  false: the
// accounting does not hold together — the kernel carries no record for a problem, a problem has no tiles, or the tile_base values
// are not the running sum of the tile counts, so that a workgroup would be handed a tile of a problem it does not belong to, i.e. an
// operand pointer out of range.  (Inside a problem tile_of_counts is a bijection onto its tiles: tests/cpp/packed_args_host.cpp.)
// Also refused: tile counts beyond what the kernels' division-free decode is proven for (tile_decode, gemm_bodies.hip.h — the
// reciprocal goes into the hot record) and leading dimensions beyond the lanes' 32-bit offsets (kMaxLeadingDim).
// grouped: the problems' tiles follow each other in the grid (tile_base = running sum); else each problem's tiles count from 0.
template <int N>
inline bool pack_args(const GemmBatch& b, GemmArgs<N>& a, bool grouped = true) {
  a = GemmArgs<N>{};
  if (b.n < 1 || b.n > N) return false;
  a.head.n = b.n; a.head.total_tiles = b.total_tiles;
  int base = 0;
  for (int i = 0; i < kMaxGroup; ++i) {
    a.head.tile_base[i] = INT32_MAX; a.head.tiles_p[i] = 1; a.head.tiles_q[i] = 1;
    if (i >= b.n) continue;
    const GemmProblem& p = b.prob[i];
    if (p.tiles_p < 1 || p.tiles_q < 1 || p.tile_base != (grouped ? base : 0)) return false;
    if (p.ldp > kMaxLeadingDim || p.ldq > kMaxLeadingDim) return false;  // a lane's 32-bit operand offset would wrap (gemm_common.hip.h)
    if (!tile_magic_covers(p.tiles_p, p.tiles_q)) return false;       // more tiles than the kernels' division-free tile decode is exact for
    const int count = p.tiles_p * p.tiles_q;
    base += count;
    a.head.tile_base[i] = p.tile_base; a.head.tiles_p[i] = p.tiles_p; a.head.tiles_q[i] = p.tiles_q;
    GemmHot& h = a.hot[i];
    h.P = p.P; h.Q = p.Q; h.C = p.C; h.ldp = p.ldp; h.ldq = p.ldq; h.ldc = p.ldc; h.Pdim = p.Pdim; h.Qdim = p.Qdim; h.Kred = p.Kred; h.mode = p.mode;
    h.tq_magic = tile_magic(p.tiles_q);
    GemmCold& c = a.cold[i];
    c.bias = p.bias; c.mask = p.mask; c.db = p.db; c.partial = p.partial; c.seed_w = p.seed_w; c.C2 = p.C2; c.dot_w = p.dot_w; c.dot_out = p.dot_out;
    c.xcopy_dst = p.xcopy_dst; c.ldm = p.ldm; c.relu = p.relu; c.xcopy_col = p.xcopy_col; c.xcopy_n = p.xcopy_n;
  }
  return true;
}
// a grouped launch of `tiles` GEMM tiles and `extra` rider blocks; R: the rider structs the kernel takes after its GemmArgs
template <typename K, typename... R>
inline hipError_t packed_launch(K kernel, const GemmBatch& batch, int extra, int lds_bytes, const LaunchOn& on, const R&... riders) {
  GemmArgs<kMaxGroup> args;
  if (!pack_args(batch, args)) return hipErrorInvalidValue;
  return launch(on, kernel, dim3(batch.total_tiles + extra), dim3(256), lds_bytes, args, riders...);
}
template <typename K>
inline hipError_t packed_launch(K kernel, GemmBatch& batch, int BP, int BQ, int lds_bytes, const LaunchOn& on) {
  tile_batch(batch, BP, BQ);
  return packed_launch(kernel, batch, 0, lds_bytes, on);
}
// the same for a kernel that takes the preload block in front of its GemmArgs (GemmPreload, gemm_common.hip.h)
template <typename K>
inline hipError_t preload_launch(K kernel, GemmBatch& batch, int BP, int BQ, int lds_bytes, const LaunchOn& on) {
  tile_batch(batch, BP, BQ);
  GemmArgs<kMaxGroup> args;
  if (!pack_args(batch, args)) return hipErrorInvalidValue;
  const GemmPreload pre = make_preload_grouped(args, on.no_preload);
  return launch(on, kernel, dim3(batch.total_tiles), dim3(256), lds_bytes, DQN_PRELOAD_WORDS(pre), args);
}

template <int TP, int TQ>
constexpr int fwd_direct_lds_bytes() { return 4 * TP * TQ * 64 * 16; }
template <int TP, int TQ>
inline hipError_t fwd_direct_launch(GemmBatch& b, const LaunchOn& on) {
  return packed_launch(gemm_fwd_direct<TP, TQ>, b, 16 * TP, 16 * TQ, fwd_direct_lds_bytes<TP, TQ>(), on);
}
template <int TP, int TQ, bool PIN, int NSLOT = 2>
constexpr int fwd_lds_bytes() {
  return 4 * 4 * ((NSLOT * (TP + TQ) * 512 > TP * TQ * 256) ? NSLOT * (TP + TQ) * 512 : TP * TQ * 256);
}
template <int TP, int TQ, bool PIN, int NSLOT = 2>
inline hipError_t fwd_lds_launch(GemmBatch& b, const LaunchOn& on) {
  return preload_launch(gemm_fwd_lds<TP, TQ, PIN, NSLOT>, b, 16 * TP, 16 * TQ, (fwd_lds_bytes<TP, TQ, PIN, NSLOT>()), on);
}
template <int TPB, int TQ>
constexpr int dgrad_direct_lds_bytes() { return 4 * TPB * 4 * TQ * 64 * 16; }
template <int TPB, int TQ>
inline hipError_t dgrad_direct_launch(GemmBatch& b, const LaunchOn& on) {
  return packed_launch(gemm_dgrad_direct<TPB, TQ>, b, 64 * TPB, 16 * TQ, dgrad_direct_lds_bytes<TPB, TQ>(), on);
}
template <int TPB, int TQ>
constexpr int dgrad_lds_bytes() { return 4 * ((2 * TQ * 512 > TPB * 4 * TQ * 256) ? 2 * TQ * 512 : TPB * 4 * TQ * 256) * 4; }
template <int TPB, int TQ>
inline hipError_t dgrad_lds_launch(GemmBatch& b, const LaunchOn& on) {
  return preload_launch(gemm_dgrad_lds<TPB, TQ>, b, 64 * TPB, 16 * TQ, dgrad_lds_bytes<TPB, TQ>(), on);
}
template <int TPB, int TQB>
inline hipError_t wgrad_direct_launch(GemmBatch& b, const LaunchOn& on) {
  return packed_launch(gemm_wgrad_direct<TPB, TQB>, b, 64 * TPB, 64 * TQB,
                       4 * TPB * 4 * TQB * 4 * 64 * 16 + 4 * TQB * 16 * 16, on);
}
// mixed dgrad(64x16)/wgrad(64x64) launch; every problem carries its own mode
template <int TQD, bool DLDS = false>
inline hipError_t bwd_pair_direct_launch(GemmBatch& batch, const LaunchOn& on) {
  int base = 0;
  for (int i = 0; i < batch.n; ++i) {          // (not tile_batch: the tile height goes by the problem's mode)
    GemmProblem& p = batch.prob[i];
    p.tiles_p = p.Pdim / 64;
    p.tiles_q = p.Qdim / (p.mode == GEMM_WGRAD ? 64 : 16 * TQD);
    p.tile_base = base;
    base += p.tiles_p * p.tiles_q;
  }
  batch.total_tiles = base;
  return packed_launch(gemm_bwd_pair_direct<TQD, DLDS>, batch, 0, kBwdTileLds, on);
}
constexpr int kNarrowDgradLds = 4 * 64 * 16;
inline hipError_t dgrad_narrow_launch(GemmBatch& b, const LaunchOn& on) {
  return packed_launch(gemm_dgrad_narrow<0>, b, 16, 16, kNarrowDgradLds, on);
}
inline hipError_t dgrad_narrow_qrider_launch(GemmBatch& batch, const QHeadRider& rider, const LaunchOn& on) {
  tile_batch(batch, 16, 16);
  return packed_launch(gemm_dgrad_narrow_qrider<0>, batch, rider.blocks, kNarrowDgradLds, on, rider);
}
template <int TPB>
constexpr int wgrad_narrow_lds_bytes() { return 4 * TPB * 4 * 64 * 16 + 4 * 16 * 4; }
template <int TPB>
inline hipError_t wgrad_narrow_launch(GemmBatch& b, const LaunchOn& on) {
  return packed_launch(gemm_wgrad_narrow<TPB>, b, 64 * TPB, 16, wgrad_narrow_lds_bytes<TPB>(), on);
}
// what the head's dW / db rider blocks need
template <int NH>
inline size_t head_rider_lds_bytes(const HeadWgradRider& rider) { return (size_t)(rider.rows * NH + 16 * NH * 16) * sizeof(float); }
template <int NH>
inline hipError_t wgrad_narrow_rider_launch(GemmBatch& batch, const HeadWgradRider& rider, const LaunchOn& on) {
  const size_t lds = std::max(head_rider_lds_bytes<NH>(rider), (size_t)wgrad_narrow_lds_bytes<1>());
  if (lds > 64 * 1024) return hipErrorInvalidValue;
  tile_batch(batch, 64, 16);
  return packed_launch(gemm_wgrad_narrow_rider<NH>, batch, rider.blocks, (int)lds, on, rider);
}
// prob[0]: wgrad on 64 x 64 tiles, prob[1]: narrow wgrad on 64 x 16 tiles; rider.blocks may be 0
template <int NH>
inline hipError_t wgrad_tail_launch(GemmBatch& batch, const HeadWgradRider& rider, const LaunchOn& on, const TailsArgs* tails_in = nullptr) {
  TailsArgs tails{}; if (tails_in != nullptr) { tails = *tails_in; tails.on = 1; }
  GemmProblem& w1 = batch.prob[0]; GemmProblem& w0 = batch.prob[1];
  w1.tiles_p = w1.Pdim / 64; w1.tiles_q = w1.Qdim / 64; w1.tile_base = 0;
  w0.tiles_p = w0.Pdim / 64; w0.tiles_q = w0.Qdim / 16; w0.tile_base = w1.tiles_p * w1.tiles_q;
  const int grid = w0.tile_base + w0.tiles_p * w0.tiles_q + rider.blocks + (tails.on ? 1 : 0);
  batch.total_tiles = grid;
  if (tails.on) tails.on = grid;         // (the tails block's index + 1: the kernel needs no gridDim, which is a scalar load of its own)
  const size_t lds = std::max(rider.blocks ? head_rider_lds_bytes<NH>(rider) : (size_t)0, (size_t)kBwdTileLds);
  if (lds > (size_t)kWgradTailLdsMax) return hipErrorInvalidValue;
  GemmArgs<2> args;
  if (batch.n != 2 || !pack_args(batch, args)) return hipErrorInvalidValue;
  const GemmPreload pre = make_preload_record(args, 0, on.no_preload, rider.blocks + w0.tiles_p * w0.tiles_q);   // (riders, narrow tiles, then the 64 x 64 tiles)
  return launch(on, gemm_wgrad_tail<NH>, dim3(grid), dim3(256), lds, DQN_PRELOAD_WORDS(pre), args, rider, tails);
}
template <bool DLDS>
inline hipError_t bwd_seq_launch(GemmBatch& batch, const LaunchOn& on) {
  // prob[0] dgrad (64 x 16 tiles), prob[1] wgrad (64 x 64 tiles)
  GemmProblem& d = batch.prob[0]; GemmProblem& w = batch.prob[1];
  d.tiles_p = d.Pdim / 64; d.tiles_q = d.Qdim / 16; d.tile_base = 0;
  w.tiles_p = w.Pdim / 64; w.tiles_q = w.Qdim / 64; w.tile_base = 0;
  const int nd = d.tiles_p * d.tiles_q, nw = w.tiles_p * w.tiles_q;
  const int grid = nd > nw ? nd : nw;
  batch.total_tiles = grid;
  GemmArgs<2> args;
  if (batch.n != 2 || !pack_args(batch, args, false)) return hipErrorInvalidValue;
  return launch(on, gemm_bwd_seq<DLDS>, dim3(grid), dim3(256), kBwdTileLds, args);
}
// ONE launch of a form of gemm_plan.hip.h: the only place that names the launcher instances.  Refuses what the form does not accept
// before anything is launched.  rider / tails: the head's dW / db rider blocks and the tails block, which the tail forms alone carry.
// (A template, like direct_prepare_all below: only a unit that calls it instantiates — and embeds — the kernels it names.)
template <int UNUSED = 0>
inline hipError_t gemm_form_launch(int form, GemmBatch& b, const LaunchOn& on, const HeadWgradRider* rider = nullptr, const TailsArgs* tails = nullptr) {
  if (!gemm_form_accepts(form, b)) return hipErrorInvalidValue;
  const bool tail = form == GEMM_FORM_WGRAD_TAIL_1 || form == GEMM_FORM_WGRAD_TAIL_NO;
  if (!tail && (rider != nullptr || tails != nullptr)) return hipErrorInvalidValue;
  const HeadWgradRider no_rider{};     // blocks = 0
  switch (form) {
    case GEMM_FORM_FWD_DIRECT_2x2: return fwd_direct_launch<2, 2>(b, on);
    case GEMM_FORM_FWD_DIRECT_4x2: return fwd_direct_launch<4, 2>(b, on);
    case GEMM_FORM_FWD_LDS_1x1: return fwd_lds_launch<1, 1, true>(b, on);
    case GEMM_FORM_FWD_LDS_2x2: return fwd_lds_launch<2, 2, true>(b, on);
    case GEMM_FORM_FWD_LDS_4x2: return fwd_lds_launch<4, 2, true>(b, on);
    case GEMM_FORM_FWD_LDS_4x2_ONE_IMAGE: return fwd_lds_launch<4, 2, true, 1>(b, on);
    case GEMM_FORM_DGRAD_DIRECT: return dgrad_direct_launch<1, 1>(b, on);
    case GEMM_FORM_DGRAD_LDS: return dgrad_lds_launch<1, 1>(b, on);
    case GEMM_FORM_DGRAD_NARROW: return dgrad_narrow_launch(b, on);
    case GEMM_FORM_WGRAD_NARROW: return wgrad_narrow_launch<1>(b, on);
    case GEMM_FORM_BWD_SEQ: return bwd_seq_launch<false>(b, on);
    case GEMM_FORM_BWD_SEQ_LDS: return bwd_seq_launch<true>(b, on);
    case GEMM_FORM_BWD_PAIR: return bwd_pair_direct_launch<1, false>(b, on);
    case GEMM_FORM_BWD_PAIR_LDS: return bwd_pair_direct_launch<1, true>(b, on);
    case GEMM_FORM_WGRAD_TAIL_1: return wgrad_tail_launch<1>(b, rider ? *rider : no_rider, on, tails);
    case GEMM_FORM_WGRAD_TAIL_NO: return wgrad_tail_launch<kNO>(b, rider ? *rider : no_rider, on, tails);
  }
  return hipErrorInvalidValue;
}
template <typename K>
inline hipError_t direct_prepare(K kernel, int lds_bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
}
// The fp32 kernels the learner launches with more than 64 KB of dynamic LDS.  Kernels have internal linkage: this sets the
// attribute on the CALLING translation unit's copies, so the unit that launches them calls it (the fp16 family: hgemm_prepare_all).
// (A template, so that only a unit that calls it instantiates — and embeds — the kernels it names.)
template <int UNUSED = 0>
inline hipError_t direct_prepare_all() {
  hipError_t e = direct_prepare(gemm_bwd_seq<true>, kBwdTileLds);
  if (e == hipSuccess) e = direct_prepare(gemm_bwd_seq<false>, kBwdTileLds);
  if (e == hipSuccess) e = direct_prepare(gemm_wgrad_tail<1>, kWgradTailLdsMax);
  if (e == hipSuccess) e = direct_prepare(gemm_wgrad_tail<10>, kWgradTailLdsMax);      // (the actor's ten heads)
  if (e == hipSuccess) e = direct_prepare(gemm_bwd_pair_direct<1, true>, kBwdTileLds);
  if (e == hipSuccess) e = direct_prepare(gemm_bwd_pair_direct<1, false>, kBwdTileLds);
  if (e == hipSuccess) e = direct_prepare(gemm_fwd_lds<4, 2, true>, fwd_lds_bytes<4, 2, true>());
  return e;
}

}  // namespace dqnhip
