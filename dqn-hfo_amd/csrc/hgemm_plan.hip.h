// hgemm_plan.hip.h — the host side of the fp16 GEMM family (hgemm.hip.h): the problem description and the tile choice.  Part of the
// argument layer (learner_args.hip.h): no kernel, no launcher.
#pragma once
#include <hip/hip_runtime.h>

namespace dqnhip {

typedef _Float16 h16;

struct HGemm {
  const h16* A; int lda;
  const h16* B; int ldb;
  int M, N, K;                 // M % BM == 0, N % BN == 0, K % 64 == 0
  h16* C16; int ldc16;         // [M][ldc16]  m-major fp16 (may be null)
  h16* CT16; int ldct16;       // [N][ldct16] transposed fp16 (may be null)
  float* C32; int ldc32;       // [M][ldc32]  fp32 (may be null); columns >= n_valid32 are not written
  int n_valid32;
  const float* bias;           // [N] added before the activation (may be null)
  int relu;                    // leaky ReLU(0.01) on the result
  const h16* mask; int ldm;    // [M][ldm]: multiply by lrelu'(mask) = mask > 0 ? 1 : 0.01 (may be null)
  float scale32;               // the fp32 output is multiplied by this (loss-scale removal)
  float* sumsq_partial;        // one slot per workgroup of this problem: sum of squares of the fp32 values it wrote (may be null)
  // forward, top tower layer of the critic(s, mu(s)) pass (may be null): also write the seed of BackwardFrom(q_values_layer)
  // (src/dqn.cpp:918-923: q diff = -1 per row) taken through the head and this layer's ReLU, as the scaled fp16 panel the dgrad
  // chain reads: CS16[m][n] = fp16(((-seed_w[n]) * lrelu'(fp16(C[m][n]))) * seed_scale) — k_head_bwd(_big)<1>'s arithmetic
  // on the fp16-rounded activation, without its launch
  const float* seed_w; h16* CS16; int ldcs16; float seed_scale;
  // Operand orientation in memory.  0: k-major — [rows][ld] with the reduction index contiguous (a lane's MFMA fragment
  // is one 16-B piece).  1: REDUCTION-major — [K][ld] with the M (resp. N) index contiguous; fragments then come out of
  // LDS through the transposing read ds_read_b64_tr_b16.  With it the three layer GEMMs read the SAME batch-major panels
  // and the SAME weight mirror:  FWD  A = X[b][k] (0), B = W[n][k] (0);  DGRAD  A = dY[b][n] (0), B = W[n][k_in] (1: rows
  // are the reduction index n);  WGRAD  A = dY[b][n] (1), B = X[b][k] (1) — no transposed copy of anything.
  int ta, tb;
};

// Up to four independent problems of the same tile configuration in one launch (the two actors' /
// the two critics' same-depth layers; a layer's dgrad + wgrad at small minibatches; ALL wgrads of a net
// once its dgrad chain has produced every dZ panel): blocks [tile_end[i-1], tile_end[i]) work on g[i].
constexpr int kHGemmMax = 4;
struct HGemmBatch { HGemm g[kHGemmMax]; int n; int tile_end[kHGemmMax]; };

// Tile choice: 256x128 (8 waves) when THAT fills the chip (two 4096-row problems in one launch), 128x128 when that
// does, else 64x64 with in-workgroup split-K.  force: 0 auto, 1 128x128, 2 64x64, 3 256x128 on eight waves,
// 4 256x128 on four waves (128x64 per wave).
inline bool hgemm_big_ok(const HGemm& g) { return (g.M % 128 == 0) && (g.N % 128 == 0); }
inline bool hgemm_huge_ok(const HGemm& g) { return (g.M % 256 == 0) && (g.N % 128 == 0) && !g.ta && !g.tb; }
inline long hgemm_tiles(const HGemm& g, bool big) { return big ? (long)(g.M / 128) * (g.N / 128) : (long)(g.M / 64) * (g.N / 64); }
inline int hgemm_mode(const HGemm& g) { return (g.ta ? 1 : 0) | (g.tb ? 2 : 0); }

// fills b (problems, tile ranges) and returns the tile configuration in wm / wn; hipErrorInvalidValue if the
// problems do not fit one
inline hipError_t hgemm_plan(const HGemm* gs, int n, int force, HGemmBatch& b, int& wm, int& wn, long& blocks) {
  if (n < 1 || n > kHGemmMax) return hipErrorInvalidValue;
  bool big_ok = true, huge_ok = true; long tiles_big = 0, tiles_huge = 0;
  for (int i = 0; i < n; ++i) {
    big_ok = big_ok && hgemm_big_ok(gs[i]); huge_ok = huge_ok && hgemm_huge_ok(gs[i]);
    if (gs[i].K % 64 || gs[i].K < 64) return hipErrorInvalidValue;
  }
  if (big_ok) for (int i = 0; i < n; ++i) tiles_big += hgemm_tiles(gs[i], true);
  if (huge_ok) for (int i = 0; i < n; ++i) tiles_huge += (long)(gs[i].M / 256) * (gs[i].N / 128);
  const bool huge = force == 3 || force == 4 || (force == 0 && huge_ok && tiles_huge >= 192);
  const bool big = !huge && (force == 1 || (force == 0 && big_ok && tiles_big >= 192));
  if (huge && !huge_ok) return hipErrorInvalidValue;
  if (big && !big_ok) return hipErrorInvalidValue;
  b = HGemmBatch{};
  b.n = n;
  blocks = 0;
  for (int i = 0; i < n; ++i) {
    b.g[i] = gs[i];
    if (huge) blocks += (long)(gs[i].M / 256) * (gs[i].N / 128);
    else if (big) blocks += hgemm_tiles(gs[i], true);
    else { if (gs[i].M % 64 || gs[i].N % 64 || gs[i].K % 128) return hipErrorInvalidValue; blocks += hgemm_tiles(gs[i], false); }
    b.tile_end[i] = (int)blocks;
  }
  wm = huge ? 4 : (big ? 2 : 1); wn = huge ? 2 : (big ? 2 : 1);
  return hipSuccess;
}
// would a stand-alone launch of g use the 64x64 split-K tile?
inline bool hgemm_uses_small_tile(const HGemm& g) { return !(hgemm_big_ok(g) && hgemm_tiles(g, true) >= 192); }

}  // namespace dqnhip
