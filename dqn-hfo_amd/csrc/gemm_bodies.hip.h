// gemm_bodies.hip.h — the BODIES of the fp32 MFMA GEMM family: device functions, no kernel (the tile maps — tile_of_counts is also
// the host's —, the packed-argument readers, one body per GEMM form, the rider blocks that GEMM launches carry).  The kernels and
// launchers on top of them, and the family's description: gemm_direct.hip.h; kernels of other groups that carry a GEMM tile
// (k_dgrad_qtrain, k_dqda_head_bwd, k_env_l0_flush, the first-layer riders of the optimiser launches) call the same bodies.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "learner_args.hip.h"

namespace dqnhip {

// ---- shared pieces ----------------------------------------------------------------

__host__ __device__ __forceinline__ void tile_of_counts(int tiles_p, int tiles_q, int b, int& tile_p, int& tile_q) {
  // tiles_p % 8 == 0: same P panel (weight slice) -> same XCD L2 (b % 8): xcd = b & 7, j = b >> 3, tile (8 (j / tiles_q) + xcd,
  // j % tiles_q); else tile (b / tiles_q, b % tiles_q).  One division for both, no branch: the prologue stays one basic block,
  // so that the scalar loads in front of it are issued together.
  const bool xmap = (tiles_p & 7) == 0;
  const int j = xmap ? b >> 3 : b;
  const int d = j / tiles_q;
  tile_q = j - d * tiles_q;
  tile_p = xmap ? d * 8 + (b & 7) : d;
}
// The same map without the division, for the kernels that take packed arguments: the host knows tiles_q, pack_args stores
// magic = tile_magic(tiles_q) = ceil(2^31 / tiles_q) in the problem's hot record, and j / tiles_q = mulhi(2 j + 1, magic) — two
// scalar instructions where the division was a convert, a reciprocal, two lane reads and two correction steps in the vector unit,
// one dependent chain in front of every launch's first load.
// Why it is exact: magic = (2^31 + e) / tiles_q with 0 <= e < tiles_q, so (2 j + 1) magic / 2^32 = (j + 1/2) / tiles_q +
// (2 j + 1) e / (tiles_q 2^32).  floor((j + 1/2) / tiles_q) = j / tiles_q, and (j + 1/2) / tiles_q lies at least 1 / (2 tiles_q)
// below the next integer, so the floor is unchanged while (2 j + 1) e < 2^31, i.e. for every j < 2^30 / tiles_q.
// (tiles_q = 1: magic = 2^31, mulhi(2 j + 1, 2^31) = j.)  What pack_args lets through is far inside that, and is the range that
// tests/cpp/tile_decode_host.cpp sweeps whole against tile_of_counts: at most kTileDecodeMaxQ row tiles and kTileDecodeMaxTiles
// tiles per problem (the product's largest launch: 256 x 64 tiles, 4096 rows of a 1024-wide layer in 16 x 16 tiles).
constexpr int kTileDecodeMaxQ = 1024, kTileDecodeMaxTiles = 1 << 18;
__host__ __device__ __forceinline__ uint32_t tile_magic(int tiles_q) { return (uint32_t)((0x80000000ull + (uint32_t)tiles_q - 1) / (uint32_t)tiles_q); }
__host__ __device__ __forceinline__ bool tile_magic_covers(int tiles_p, int tiles_q) {
  return tiles_p >= 1 && tiles_q >= 1 && tiles_q <= kTileDecodeMaxQ && (int64_t)tiles_p * tiles_q <= kTileDecodeMaxTiles;
}
__host__ __device__ __forceinline__ void tile_decode(int tiles_p, int tiles_q, uint32_t magic, int b, int& tile_p, int& tile_q) {
  const bool xmap = (tiles_p & 7) == 0;
  const int j = xmap ? b >> 3 : b;
  const int d = (int)(((uint64_t)(2u * (uint32_t)j + 1u) * magic) >> 32);
  tile_q = j - d * tiles_q;
  tile_p = xmap ? d * 8 + (b & 7) : d;
}
__device__ __forceinline__ void tile_of_problem(const GemmProblem& pr, int b, int& tile_p, int& tile_q) {
  tile_of_counts(pr.tiles_p, pr.tiles_q, b, tile_p, tile_q);
}
__device__ __forceinline__ void tile_of_block(const GemmBatch& batch, int& pi, int& tile_p, int& tile_q) {
  int b = blockIdx.x;
  pi = 0;
#pragma unroll
  for (int i = 1; i < kMaxGroup; ++i)
    if (i < batch.n && b >= batch.prob[i].tile_base) pi = i;
  const GemmProblem& pr = batch.prob[pi];
  tile_of_problem(pr, b - pr.tile_base, tile_p, tile_q);
}

// ---- the packed form (GemmArgs, gemm_common.hip.h) ----
// The GemmProblem a body takes, assembled in registers.  `cold` may be indexed by pi: its loads are the epilogue's.
__device__ __forceinline__ GemmProblem make_problem(const float* P, const float* Q, float* C, int ldp, int ldq, int ldc, int Pdim, int Qdim, int Kred,
                                                    int mode, const GemmCold& c, int tiles_p, int tiles_q, int tile_base) {
  GemmProblem pr;
  pr.P = P; pr.ldp = ldp; pr.Q = Q; pr.ldq = ldq; pr.C = C; pr.ldc = ldc; pr.Pdim = Pdim; pr.Qdim = Qdim; pr.Kred = Kred;
  pr.bias = c.bias; pr.mask = c.mask; pr.ldm = c.ldm; pr.db = c.db; pr.partial = c.partial; pr.relu = c.relu;
  pr.seed_w = c.seed_w; pr.C2 = c.C2; pr.dot_w = c.dot_w; pr.dot_out = c.dot_out;
  pr.xcopy_dst = c.xcopy_dst; pr.xcopy_col = c.xcopy_col; pr.xcopy_n = c.xcopy_n;
  pr.mode = mode; pr.tiles_p = tiles_p; pr.tiles_q = tiles_q; pr.tile_base = tile_base;
  return pr;
}
// One wait for a launch's scalar arguments.  The (empty) statement reads one value of every 16-byte piece of the header and of the
// hot records, what the choice of a record and the tile decode read of them besides (Pdim, tq_magic), and up to two values of a
// rider struct (x0 / x1), and hands back the block index, from which everything else is
// computed: the compiler has to request all of them before it and cannot compute anything behind its back in between — left alone
// it requests the header, waits, does the tile arithmetic, requests the records, waits again.
template <int N>
struct HotArgs { GemmHeader hd; GemmHot hot[N]; };
template <int N>
__device__ __forceinline__ int request_args(const GemmArgs<N>& a, HotArgs<N>& r, int b, int x0 = 0, int x1 = 0) {
  r.hd = a.head;
#pragma unroll
  for (int i = 0; i < N; ++i) r.hot[i] = a.hot[i];
  const GemmHot &h0 = r.hot[0], &h1 = r.hot[N > 1 ? 1 : 0], &h2 = r.hot[N > 2 ? 2 : 0], &h3 = r.hot[N > 3 ? 3 : 0];
  asm volatile("" : "+s"(b) : "s"(r.hd.tile_base[1]), "s"(r.hd.tiles_p[0]), "s"(r.hd.tiles_q[0]), "s"(x0), "s"(x1),
               "s"(h0.P), "s"(h0.ldp), "s"(h0.C), "s"(h1.P), "s"(h1.ldp), "s"(h1.C), "s"(h2.P), "s"(h2.ldp), "s"(h2.C), "s"(h3.P), "s"(h3.ldp), "s"(h3.C),
               "s"(h0.Pdim), "s"(h1.Pdim), "s"(h2.Pdim), "s"(h3.Pdim), "s"(h0.tq_magic), "s"(h1.tq_magic), "s"(h2.tq_magic), "s"(h3.tq_magic));
  return b;
}
// problem I of a kernel whose problems are a compile-time fact (gemm_bwd_seq, gemm_wgrad_tail, k_dgrad_qtrain): no select at all
template <int I, int N>
__device__ __forceinline__ GemmProblem problem_at(const GemmArgs<N>& a, const HotArgs<N>& r) {
  static_assert(I < N, "record not carried");
  const GemmHot& h = r.hot[I];
  return make_problem(h.P, h.Q, h.C, h.ldp, h.ldq, h.ldc, h.Pdim, h.Qdim, h.Kred, h.mode, a.cold[I], r.hd.tiles_p[I], r.hd.tiles_q[I], r.hd.tile_base[I]);
}
// ... and tile b of that problem (b counts from the problem's first tile)
template <int I, int N>
__device__ __forceinline__ void tile_of_record(const HotArgs<N>& r, int b, int& tile_p, int& tile_q) {
  static_assert(I < N, "record not carried");
  tile_decode(r.hd.tiles_p[I], r.hd.tiles_q[I], r.hot[I].tq_magic, b, tile_p, tile_q);
}
// GEMM tile b (request_args' return value) of a grouped launch: its problem and tile coordinates from the header alone, the hot
// fields of that problem's record
template <int N>
__device__ __forceinline__ GemmProblem problem_of_tile(const GemmArgs<N>& a, const HotArgs<N>& r, const int b, int& tile_p, int& tile_q) {
  const GemmHeader& hd = r.hd;
  // A tile of problem 0 — every tile of a one-problem launch, which most launches of an update are (tile_base[1] = INT_MAX) —
  // takes record 0 as it is, a tile of problem 1 record 1 as it is, and only the tiles of problems 2 and 3 choose, with ONE select
  // per field.  The problem search and the three-deep selects over every field used to be some sixty scalar instructions between
  // the arguments' arrival and every workgroup's first operand load; now they are uniform branches that a workgroup of an early
  // problem does not enter.  (The empty statements keep the compiler from turning the branches back into selects.)
  int pi = 0;
  int tiles_p = hd.tiles_p[0], tiles_q = hd.tiles_q[0], tile_base = hd.tile_base[0];
  GemmHot h = r.hot[0];
  if (N > 1 && b >= hd.tile_base[N > 1 ? 1 : 0]) {
    pi = 1;
    tiles_p = hd.tiles_p[N > 1 ? 1 : 0]; tiles_q = hd.tiles_q[N > 1 ? 1 : 0]; tile_base = hd.tile_base[N > 1 ? 1 : 0];
    h = r.hot[N > 1 ? 1 : 0];
    if (N > 2 && b >= hd.tile_base[N > 2 ? 2 : 0]) {
      constexpr int I2 = N > 2 ? 2 : 0, I3 = N > 3 ? 3 : I2;
      const bool last = N > 3 && b >= hd.tile_base[I3];
      const GemmHot &h2 = r.hot[I2], &h3 = r.hot[I3];
      pi = last ? I3 : I2;
      tiles_p = last ? hd.tiles_p[I3] : hd.tiles_p[I2]; tiles_q = last ? hd.tiles_q[I3] : hd.tiles_q[I2];
      tile_base = last ? hd.tile_base[I3] : hd.tile_base[I2];
      h.P = last ? h3.P : h2.P; h.Q = last ? h3.Q : h2.Q; h.C = last ? h3.C : h2.C;
      h.ldp = last ? h3.ldp : h2.ldp; h.ldq = last ? h3.ldq : h2.ldq; h.ldc = last ? h3.ldc : h2.ldc;
      h.Pdim = last ? h3.Pdim : h2.Pdim; h.Qdim = last ? h3.Qdim : h2.Qdim; h.Kred = last ? h3.Kred : h2.Kred;
      h.mode = last ? h3.mode : h2.mode; h.tq_magic = last ? h3.tq_magic : h2.tq_magic;
      asm volatile("" : "+s"(pi));
    }
    asm volatile("" : "+s"(pi));
  }
  tile_decode(tiles_p, tiles_q, h.tq_magic, b - tile_base, tile_p, tile_q);
  return make_problem(h.P, h.Q, h.C, h.ldp, h.ldq, h.ldc, h.Pdim, h.Qdim, h.Kred, h.mode, a.cold[N == 1 ? 0 : pi], tiles_p, tiles_q, tile_base);
}
template <int N>
__device__ __forceinline__ GemmProblem problem_of_block(const GemmArgs<N>& a, int& tile_p, int& tile_q) {
  HotArgs<N> r;
  const int b = request_args(a, r, (int)blockIdx.x);
  return problem_of_tile(a, r, b, tile_p, tile_q);
}

// ---- the preloaded form (GemmPreload, gemm_common.hip.h) ----
// What a workgroup reads out of the 14 preloaded dwords: the tile of block b, its problem (0, or 1 from `split` on) and that problem's
// operand bases.  Host and device share it (tests/cpp/kernarg_preload_host.cpp holds it against the packed GemmArgs).
struct PreTile { int pi, tile_p, tile_q, tiles_p, tiles_q, tile_base; const float* P; const float* Q; };
__host__ __device__ __forceinline__ PreTile preload_decode(const GemmPreload& w, int b) {
  PreTile t;
  const int split = (int)(w.flags >> kPreSplitShift);
  t.pi = b >= split ? 1 : 0;
  t.tile_base = t.pi ? split : 0;
  t.tiles_p = (int)(w.tiles & ((1u << kPreTilesQShift) - 1)); t.tiles_q = (int)(w.tiles >> kPreTilesQShift);
  tile_decode(t.tiles_p, t.tiles_q, w.magic, b - t.tile_base, t.tile_p, t.tile_q);
  t.P = t.pi ? w.P1 : w.P0; t.Q = t.pi ? w.Q1 : w.Q0;
  return t;
}
// The record form: the block holds ONE record of a kernel whose workgroups know their records at compile time, and in place of the
// split the index `first` of the launch's first block that computes a tile of it (gemm_wgrad_tail's 64 x 64 tiles come behind its
// riders and narrow tiles; k_dgrad_qtrain: 0).  Block b computes tile b - first of the record, or — in front of `first`, behind the
// record's last tile — none of it (mine = false: that block takes the kernel's GemmArgs path).  Host and device share this too.
struct PreRecordTile { bool mine; int tile_p, tile_q, tiles_p, tiles_q; };
__host__ __device__ __forceinline__ PreRecordTile preload_record_decode(const GemmPreload& w, int b) {
  PreRecordTile t;
  const int bb = b - (int)(w.flags >> kPreSplitShift);
  t.tiles_p = (int)(w.tiles & ((1u << kPreTilesQShift) - 1)); t.tiles_q = (int)(w.tiles >> kPreTilesQShift);
  t.mine = bb >= 0 && bb < t.tiles_p * t.tiles_q;
  tile_decode(t.tiles_p, t.tiles_q, w.magic, t.mine ? bb : 0, t.tile_p, t.tile_q);
  return t;
}
// The host side.  A value that its field cannot hold makes the block "not valid" (all zero), never a truncated value.
inline bool preload_record_fits(const GemmHot& h, int tiles_p, int tiles_q) {
  return h.ldp >= 0 && h.ldp <= kMaxLeadingDim && h.ldq >= 0 && h.ldq <= kMaxLeadingDim && h.Kred >= 0 &&
         tile_magic_covers(tiles_p, tiles_q) && tiles_p < (1 << kPreTilesQShift) && tiles_q < (1 << (32 - kPreTilesQShift)) &&
         h.tq_magic == tile_magic(tiles_q);
}
// record i with the word that follows the flags: the split (grouped forms) or `first` (record form)
template <int N>
inline GemmPreload make_preload_words(const GemmArgs<N>& a, int i, uint32_t split_or_first) {
  GemmPreload w{};
  if (i < 0 || i >= N || i >= a.head.n || split_or_first > kPreNoSplit) return w;
  const GemmHot& h = a.hot[i];
  const int tp = a.head.tiles_p[i], tq = a.head.tiles_q[i];
  if (!preload_record_fits(h, tp, tq)) return w;
  w.P0 = h.P; w.Q0 = h.Q; w.ldp = (uint32_t)h.ldp; w.ldq = (uint32_t)h.ldq; w.Kred = (uint32_t)h.Kred;
  w.tiles = (uint32_t)tp | (uint32_t)tq << kPreTilesQShift; w.magic = h.tq_magic;
  w.flags = kPreValid | split_or_first << kPreSplitShift;
  return w;
}
// the record form of record i (preload_record_decode)
template <int N>
inline GemmPreload make_preload_record(const GemmArgs<N>& a, int i, bool off, int first = 0) {
  if (off || first < 0) return GemmPreload{};
  return make_preload_words(a, i, (uint32_t)first);
}
// a grouped launch (preload_decode): one problem, or two of equal shape whose tiles follow each other in the grid
template <int N>
inline GemmPreload make_preload_grouped(const GemmArgs<N>& a, bool off) {
  if (off || a.head.tile_base[0] != 0) return GemmPreload{};
  if (a.head.n == 1) return make_preload_words(a, 0, kPreNoSplit);
  if (N < 2 || a.head.n != 2) return GemmPreload{};
  const GemmHot &h = a.hot[0], &g = a.hot[N > 1 ? 1 : 0];
  const int tp = a.head.tiles_p[0], tq = a.head.tiles_q[0], split = a.head.tile_base[1];
  if (g.ldp != h.ldp || g.ldq != h.ldq || g.Kred != h.Kred || a.head.tiles_p[1] != tp || a.head.tiles_q[1] != tq || g.tq_magic != h.tq_magic) return GemmPreload{};
  if (split < 0 || (uint32_t)split >= kPreNoSplit) return GemmPreload{};
  GemmPreload w = make_preload_words(a, 0, (uint32_t)split);
  if (!(w.flags & kPreValid) || split != tp * tq) return GemmPreload{};
  w.P1 = g.P; w.Q1 = g.Q;
  return w;
}
// The device side: GEMM tile b of a valid block.  The operand bases, leading dimensions, reduction length and tile coordinates come
// from the preloaded words — no scalar load stands in front of the body's first operand loads —; C, the output dimensions and the cold
// record are the epilogue's and are read from the GemmArgs record of the tile's problem, requests that return under the operand loads.
template <int N>
__device__ __forceinline__ GemmProblem problem_of_preload(const GemmPreload& w, const GemmArgs<N>& a, int b, int& tile_p, int& tile_q) {
  const PreTile t = preload_decode(w, b);
  tile_p = t.tile_p; tile_q = t.tile_q;
  const int pi = N == 1 ? 0 : t.pi;
  const GemmHot& h = a.hot[pi];
  return make_problem(t.P, t.Q, h.C, (int)w.ldp, (int)w.ldq, h.ldc, h.Pdim, h.Qdim, (int)w.Kred, h.mode, a.cold[pi], t.tiles_p, t.tiles_q, t.tile_base);
}
// ... and record I of a kernel whose records are a compile-time fact, for a block whose tile t (preload_record_decode) is its own
template <int I, int N>
__device__ __forceinline__ GemmProblem record_of_preload(const GemmPreload& w, const GemmArgs<N>& a, const PreRecordTile& t) {
  static_assert(I < N, "record not carried");
  const GemmHot& h = a.hot[I];
  return make_problem(w.P0, w.Q0, h.C, (int)w.ldp, (int)w.ldq, h.ldc, h.Pdim, h.Qdim, (int)w.Kred, h.mode, a.cold[I], t.tiles_p, t.tiles_q, a.head.tile_base[I]);
}

// Each wave parks its NACC accumulators in LDS (lane-linear: conflict free), then wave w
// returns, for every accumulator e with (e & 3) == w, the fixed-order sum over the 4 waves.
template <int NACC>
__device__ __forceinline__ void park_accumulators(float* smem, const f32x4 (&acc)[NACC], int wave, int lane) {
  f32x4* s = reinterpret_cast<f32x4*>(smem);
#pragma unroll
  for (int e = 0; e < NACC; ++e) s[(wave * NACC + e) * 64 + lane] = acc[e];
}
template <int NACC>
__device__ __forceinline__ f32x4 reduce_accumulator(const float* smem, int e, int lane) {
  const f32x4* s = reinterpret_cast<const f32x4*>(smem);
  const f32x4 a0 = s[(0 * NACC + e) * 64 + lane], a1 = s[(1 * NACC + e) * 64 + lane];
  const f32x4 a2 = s[(2 * NACC + e) * 64 + lane], a3 = s[(3 * NACC + e) * 64 + lane];
  f32x4 r;
  r.x = (a0.x + a1.x) + (a2.x + a3.x); r.y = (a0.y + a1.y) + (a2.y + a3.y);
  r.z = (a0.z + a1.z) + (a2.z + a3.z); r.w = (a0.w + a1.w) + (a2.w + a3.w);
  return r;
}

#define DQN_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
// hipcc otherwise sinks every prefetch load below the whole MFMA block of an iteration
// (collapsing the register ring: measured); pin the COMPUTE/LOAD interleave.
#define DQN_PIN() __builtin_amdgcn_sched_barrier(0)

// GemmProblem::seed_w: the tower-top gradient of the dq = -1 pass, from the finished activations v of this lane
// (k_head_bwd<1>'s arithmetic: s0 = fma(-1, w, 0) = -w, then * lrelu'(x))
__device__ __forceinline__ void store_head_seed(const GemmProblem& pr, int q, int p, const f32x4& v, const f32x4& sw) {
  f32x4 dz;
  dz.x = (-sw.x) * lrelu_mask(v.x); dz.y = (-sw.y) * lrelu_mask(v.y);
  dz.z = (-sw.z) * lrelu_mask(v.z); dz.w = (-sw.w) * lrelu_mask(v.w);
  *reinterpret_cast<f32x4*>(pr.C2 + (size_t)q * pr.ldc + p) = dz;
}

// GemmProblem::dot_w: this lane's four finished activations v against the head weights dw, summed over the four lane groups
// (16 columns), written by lane group 0
__device__ __forceinline__ void store_head_dot(const GemmProblem& pr, int q, int p, int lg, const f32x4& v, const f32x4& dw) {
  float d = fmaf(v.x, dw.x, 0.0f); d = fmaf(v.y, dw.y, d); d = fmaf(v.z, dw.z, d); d = fmaf(v.w, dw.w, d);
  d += __shfl_xor(d, 16, 64);
  d += __shfl_xor(d, 32, 64);
  if (lg == 0) pr.dot_out[(size_t)q * (pr.Pdim >> 4) + (p >> 4)] = d;
}

// ================================ FWD ================================================
// Y[m][n] = lrelu(sum_k X[m][k] W[n][k] + b[n]).  P = W (KC, 16-row blocks), Q = X (KC).
// Tile = (16*TP) x (16*TQ).  Kred % 64 == 0.
template <int TP, int TQ>
__device__ __forceinline__ void fwd_direct_body(const GemmProblem& pr, int tile_p, int tile_q, float* smem) {
  constexpr int NACC = TP * TQ;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int p0 = tile_p * 16 * TP, q0 = tile_q * 16 * TQ;
  const int Kw = pr.Kred >> 2;              // this wave's share of the reduction
  const int nkb = Kw >> 4;                  // 16-wide k blocks
  // (addresses as in fwd_lds_body: a wave-uniform base per 16-row block, one 32-bit lane offset per operand — row li, k chunk lg)
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const char* pp[TP];
  const char* qp[TQ];
  const uint32_t lofp = ((uint32_t)li * (uint32_t)pr.ldp + (uint32_t)lg * 4u) * 4u, lofq = ((uint32_t)li * (uint32_t)pr.ldq + (uint32_t)lg * 4u) * 4u;
#pragma unroll
  for (int c = 0; c < TP; ++c) pp[c] = c == 0 ? reinterpret_cast<const char*>(pr.P + (size_t)p0 * pr.ldp + wave_u * Kw) : pp[c > 0 ? c - 1 : 0] + (size_t)64 * pr.ldp;
#pragma unroll
  for (int a = 0; a < TQ; ++a) qp[a] = a == 0 ? reinterpret_cast<const char*>(pr.Q + (size_t)q0 * pr.ldq + wave_u * Kw) : qp[a > 0 ? a - 1 : 0] + (size_t)64 * pr.ldq;

  f32x4 acc[NACC];
#pragma unroll
  for (int e = 0; e < NACC; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 rp[4][TP], rq[4][TQ];

#define FWD_LOAD(slot, kb)                                                              \
  {                                                                                     \
    _Pragma("unroll") for (int c = 0; c < TP; ++c)                                      \
        rp[slot][c] = *reinterpret_cast<const f32x4*>(pp[c] + ((kb) << 6) + lofp);     \
    _Pragma("unroll") for (int a = 0; a < TQ; ++a)                                      \
        rq[slot][a] = *reinterpret_cast<const f32x4*>(qp[a] + ((kb) << 6) + lofq);     \
  }
#define FWD_COMPUTE(slot)                                                               \
  {                                                                                     \
    _Pragma("unroll") for (int s = 0; s < 4; ++s)                                       \
    _Pragma("unroll") for (int a = 0; a < TQ; ++a)                                      \
    _Pragma("unroll") for (int c = 0; c < TP; ++c)                                      \
        acc[a * TP + c] = DQN_MFMA(rp[slot][c][s], rq[slot][a][s], acc[a * TP + c]);    \
  }

  const int nkb4 = nkb & ~3;
  if (nkb4 > 0) {
    FWD_LOAD(0, 0) FWD_LOAD(1, 1) FWD_LOAD(2, 2) FWD_LOAD(3, 3)
    int kb = 0;
    for (; kb + 4 < nkb4; kb += 4) {
      FWD_COMPUTE(0) DQN_PIN(); FWD_LOAD(0, kb + 4) DQN_PIN();
      FWD_COMPUTE(1) DQN_PIN(); FWD_LOAD(1, kb + 5) DQN_PIN();
      FWD_COMPUTE(2) DQN_PIN(); FWD_LOAD(2, kb + 6) DQN_PIN();
      FWD_COMPUTE(3) DQN_PIN(); FWD_LOAD(3, kb + 7) DQN_PIN();
    }
    FWD_COMPUTE(0) FWD_COMPUTE(1) FWD_COMPUTE(2) FWD_COMPUTE(3)
  }
  // the (up to three) remaining steps: every load first, then the MFMAs (the first tower layer has K_in = 64 / 128,
  // i.e. ONLY these steps: one load round trip instead of one per step)
  {
    const int rem = nkb - nkb4;
    if (rem > 0) FWD_LOAD(0, nkb4)
    if (rem > 1) FWD_LOAD(1, nkb4 + 1)
    if (rem > 2) FWD_LOAD(2, nkb4 + 2)
    if (rem > 0) FWD_COMPUTE(0)
    if (rem > 1) FWD_COMPUTE(1)
    if (rem > 2) FWD_COMPUTE(2)
  }
#undef FWD_LOAD
#undef FWD_COMPUTE

  // this wave's bias (and head-seed) pieces, requested ahead of the cross-wave reduction
  constexpr int NBV = (NACC + 3) / 4;
  f32x4 bvp[NBV], swp[NBV], dwp[NBV];
  if (pr.bias != nullptr) {
#pragma unroll
    for (int j = 0; j < NBV; ++j) {
      const int e = j * 4 + wave;
      if (e < NACC) bvp[j] = *reinterpret_cast<const f32x4*>(pr.bias + p0 + (e % TP) * 16 + (lg << 2));
    }
  }
  if (pr.seed_w != nullptr) {
#pragma unroll
    for (int j = 0; j < NBV; ++j) {
      const int e = j * 4 + wave;
      if (e < NACC) swp[j] = *reinterpret_cast<const f32x4*>(pr.seed_w + p0 + (e % TP) * 16 + (lg << 2));
    }
  }
  if (pr.dot_w != nullptr) {
#pragma unroll
    for (int j = 0; j < NBV; ++j) {
      const int e = j * 4 + wave;
      if (e < NACC) dwp[j] = *reinterpret_cast<const f32x4*>(pr.dot_w + p0 + (e % TP) * 16 + (lg << 2));
    }
  }
  if (pr.xcopy_dst != nullptr && (int)threadIdx.x < 16 * TP) {      // (column j by the workgroup of row tile j mod tiles_q: one or two dwords per thread)
    const float* src = pr.P + (size_t)(p0 + threadIdx.x) * pr.ldp + pr.xcopy_col;
    for (int j = tile_q; j < pr.xcopy_n; j += pr.tiles_q) pr.xcopy_dst[(size_t)j * pr.Pdim + p0 + threadIdx.x] = src[j];
  }
  park_accumulators<NACC>(smem, acc, wave, lane);
  __syncthreads();
#pragma unroll
  for (int e = 0; e < NACC; ++e) {
    if ((e & 3) == wave) {
      const int a = e / TP, c = e % TP;
      f32x4 v = reduce_accumulator<NACC>(smem, e, lane);
      const int q = q0 + a * 16 + li, p = p0 + c * 16 + (lg << 2);
      if (pr.bias != nullptr) {
        const f32x4 bv = bvp[e >> 2];
        v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
      }
      if (pr.relu) { v.x = lrelu_fwd(v.x); v.y = lrelu_fwd(v.y); v.z = lrelu_fwd(v.z); v.w = lrelu_fwd(v.w); }
      *reinterpret_cast<f32x4*>(pr.C + (size_t)q * pr.ldc + p) = v;
      if (pr.seed_w != nullptr) store_head_seed(pr, q, p, v, swp[e >> 2]);
      if (pr.dot_w != nullptr) store_head_dot(pr, q, p, lg, v, dwp[e >> 2]);
    }
  }
}

// ================================ DGRAD ==============================================
// dX[m][j] = (sum_n dY[m][n] W[n][j]) * lrelu'(act[m][j]).  P = W (KS, 64-wide blocks of j),
// Q = dY (KC, 16-row blocks of m).  Tile = (64*TPB) x (16*TQ).  Kred (= n) % 64 == 0.
template <int TPB, int TQ>
__device__ __forceinline__ void dgrad_direct_body(const GemmProblem& pr, int tile_p, int tile_q, float* smem) {
  constexpr int NACC = TPB * 4 * TQ;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int p0 = tile_p * 64 * TPB, q0 = tile_q * 16 * TQ;
  const int Kw = pr.Kred >> 2;
  const int nkb = Kw >> 4;
  // P rows are reduction indices: lane group lg owns n = base + kb*16 + 4*lg + s at step s
  const float* pp = pr.P + (size_t)(wave * Kw + lg * 4) * pr.ldp + p0 + li * 4;
  const float* qp[TQ];
#pragma unroll
  for (int a = 0; a < TQ; ++a) qp[a] = pr.Q + (size_t)(q0 + a * 16 + li) * pr.ldq + wave * Kw + lg * 4;
  const size_t ldp = pr.ldp;

  f32x4 acc[NACC];   // index ((a*TPB + b)*4 + pc)
#pragma unroll
  for (int e = 0; e < NACC; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 rp[4][4][TPB], rq[4][TQ];

#define DG_LOAD(slot, kb)                                                               \
  {                                                                                     \
    _Pragma("unroll") for (int a = 0; a < TQ; ++a)                                      \
        rq[slot][a] = *reinterpret_cast<const f32x4*>(qp[a] + ((kb) << 4));            \
    _Pragma("unroll") for (int s = 0; s < 4; ++s)                                       \
    _Pragma("unroll") for (int b = 0; b < TPB; ++b)                                     \
        rp[slot][s][b] = *reinterpret_cast<const f32x4*>(pp + (size_t)(((kb) << 4) + s) * ldp + b * 64); \
  }
#define DG_COMPUTE(slot)                                                                \
  {                                                                                     \
    _Pragma("unroll") for (int s = 0; s < 4; ++s)                                       \
    _Pragma("unroll") for (int a = 0; a < TQ; ++a)                                      \
    _Pragma("unroll") for (int b = 0; b < TPB; ++b)                                     \
    _Pragma("unroll") for (int pc = 0; pc < 4; ++pc)                                    \
        acc[(a * TPB + b) * 4 + pc] =                                                   \
            DQN_MFMA(rp[slot][s][b][pc], rq[slot][a][s], acc[(a * TPB + b) * 4 + pc]);  \
  }

  const int nkb4 = nkb & ~3;
  if (nkb4 > 0) {
    DG_LOAD(0, 0) DG_LOAD(1, 1) DG_LOAD(2, 2) DG_LOAD(3, 3)
    int kb = 0;
    for (; kb + 4 < nkb4; kb += 4) {
      DG_COMPUTE(0) DQN_PIN(); DG_LOAD(0, kb + 4) DQN_PIN();
      DG_COMPUTE(1) DQN_PIN(); DG_LOAD(1, kb + 5) DQN_PIN();
      DG_COMPUTE(2) DQN_PIN(); DG_LOAD(2, kb + 6) DQN_PIN();
      DG_COMPUTE(3) DQN_PIN(); DG_LOAD(3, kb + 7) DQN_PIN();
    }
    DG_COMPUTE(0) DG_COMPUTE(1) DG_COMPUTE(2) DG_COMPUTE(3)
  }
  for (int kb = nkb4; kb < nkb; ++kb) { DG_LOAD(0, kb) DG_COMPUTE(0) }
#undef DG_LOAD
#undef DG_COMPUTE

  // this wave's ReLU' mask pieces, requested ahead of the cross-wave reduction
  constexpr int NMK = (TQ * TPB + 3) / 4;
  f32x4 mk[NMK][4];
  if (pr.mask != nullptr) {
#pragma unroll
    for (int j = 0; j < NMK; ++j) {
      const int ab = j * 4 + wave;
      if (ab < TQ * TPB) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          mk[j][r] = *reinterpret_cast<const f32x4*>(pr.mask + (size_t)(q0 + (ab / TPB) * 16 + li) * pr.ldm + p0 + (ab % TPB) * 64 + (lg << 4) + (r << 2));
      }
    }
  }
  park_accumulators<NACC>(smem, acc, wave, lane);
  __syncthreads();
  // accumulators (a,b,pc=0..3) form float4s over pc: reduce them as a group of 4
#pragma unroll
  for (int ab = 0; ab < TQ * TPB; ++ab) {
    if ((ab & 3) == wave) {
      const int a = ab / TPB, b = ab % TPB;
      f32x4 r0 = reduce_accumulator<NACC>(smem, ab * 4 + 0, lane);
      f32x4 r1 = reduce_accumulator<NACC>(smem, ab * 4 + 1, lane);
      f32x4 r2 = reduce_accumulator<NACC>(smem, ab * 4 + 2, lane);
      f32x4 r3 = reduce_accumulator<NACC>(smem, ab * 4 + 3, lane);
      const int q = q0 + a * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = p0 + b * 64 + (lg << 4) + (r << 2);
        f32x4 v = f32x4{r0[r], r1[r], r2[r], r3[r]};
        if (pr.mask != nullptr) {
          const f32x4 mv = mk[ab >> 2][r];
          v.x *= lrelu_mask(mv.x); v.y *= lrelu_mask(mv.y); v.z *= lrelu_mask(mv.z); v.w *= lrelu_mask(mv.w);
        }
        *reinterpret_cast<f32x4*>(pr.C + (size_t)q * pr.ldc + p) = v;
      }
    }
  }
}

// ---- DGRAD, narrow: 16 input columns per workgroup ------------------------------------------
// The critic's first-layer input gradient is consumed only in the 10 action columns (inverting
// gradients, src/dqn.cpp:924-957): instead of 64-wide tiles over the whole 128-column panel (32
// workgroups, 4.2 us of MFMA per wave) only the 16-column tiles that contain those columns are
// computed, a quarter of the MFMA chain per wave.  P = W (one column per lane, scalar loads),
// Q = dY (16 rows).  Same K split over the 4 waves, same fixed-order reduction.
// dgrad_narrow_tile: the reduced (and masked) 16 x 16 tile in wave 0's lanes — lane (li, lg), register r = dX[row q0 + li][column
// p0 + 4 lg + r]; the other waves return zeros.  dgrad_narrow_body stores it.
// NS: register ring depth in 16-k steps (a wave's quarter of a 1024-deep reduction is 16 steps: NS = 8 -> two load round trips
// instead of four; the order in which the MFMAs accumulate does not depend on it)
template <int NS = 4>
__device__ __forceinline__ f32x4 dgrad_narrow_tile(const GemmProblem& pr, int tile_p, int tile_q, float* smem) {
  constexpr int NACC = 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int p0 = tile_p * 16, q0 = tile_q * 16;
  const int Kw = pr.Kred >> 2;
  const int nkb = Kw >> 4;
  const float* pp = pr.P + (size_t)(wave * Kw + lg * 4) * pr.ldp + p0 + li;
  const float* qp = pr.Q + (size_t)(q0 + li) * pr.ldq + wave * Kw + lg * 4;
  const size_t ldp = pr.ldp;
  f32x4 acc[NACC];
  acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
  float rp[NS][4]; f32x4 rq[NS];
#define DN_LOAD(slot, kb)                                                               \
  {                                                                                     \
    rq[slot] = *reinterpret_cast<const f32x4*>(qp + ((kb) << 4));                      \
    _Pragma("unroll") for (int s = 0; s < 4; ++s) rp[slot][s] = pp[(size_t)(((kb) << 4) + s) * ldp]; \
  }
#define DN_COMPUTE(slot)                                                                \
  { _Pragma("unroll") for (int s = 0; s < 4; ++s) acc[0] = DQN_MFMA(rp[slot][s], rq[slot][s], acc[0]); }
  const int nkbN = nkb - nkb % NS;
  if (nkbN > 0) {
#pragma unroll
    for (int i = 0; i < NS; ++i) { DN_LOAD(i, i) DQN_PIN(); }
    int kb = 0;
    for (; kb + NS < nkbN; kb += NS) {
#pragma unroll
      for (int i = 0; i < NS; ++i) { DN_COMPUTE(i) DQN_PIN(); DN_LOAD(i, kb + NS + i) DQN_PIN(); }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) { DN_COMPUTE(i) }
  }
  for (int kb = nkbN; kb < nkb; ++kb) { DN_LOAD(0, kb) DN_COMPUTE(0) }
#undef DN_LOAD
#undef DN_COMPUTE
  f32x4 mv = f32x4{0.f, 0.f, 0.f, 0.f};          // requested ahead of the cross-wave reduction
  if (wave == 0 && pr.mask != nullptr) mv = *reinterpret_cast<const f32x4*>(pr.mask + (size_t)(q0 + li) * pr.ldm + p0 + (lg << 2));
  park_accumulators<NACC>(smem, acc, wave, lane);
  __syncthreads();
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (wave == 0) {
    // C/D map: lane (li, lg) register r = C[i = 4 lg + r][j = li] = dX[row q0 + li][column p0 + 4 lg + r]
    v = reduce_accumulator<NACC>(smem, 0, lane);
    if (pr.mask != nullptr) {
      v.x *= lrelu_mask(mv.x); v.y *= lrelu_mask(mv.y); v.z *= lrelu_mask(mv.z); v.w *= lrelu_mask(mv.w);
    }
  }
  return v;
}
// The same tile from the fp16 learner's operands (round 6): P = the fp16 weight mirror W16[n][k_in] (one column per lane), Q = the
// scaled fp16 gradient panel dY16[rows][n].  fp16 x fp16 products are exact in fp32, so this is the fp16-MFMA dgrad's arithmetic up
// to the order of the fp32 additions; the caller removes the loss scale.  No mask (the layer's input has no ReLU).
template <int NS = 4>
__device__ __forceinline__ f32x4 dgrad_narrow_tile16(const NarrowTile16& pr, int tile_q, float* smem) {
  typedef __attribute__((ext_vector_type(4))) _Float16 h4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int q0 = tile_q * 16;
  const int Kw = pr.Kred >> 2;
  const int nkb = Kw >> 4;
  const _Float16* pp = pr.P + (size_t)(wave * Kw + lg * 4) * pr.ldp + li;
  const _Float16* qp = pr.Q + (size_t)(q0 + li) * pr.ldq + wave * Kw + lg * 4;
  const size_t ldp = pr.ldp;
  f32x4 acc[1];
  acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
  _Float16 rp[NS][4]; h4 rq[NS];
#define DN_LOAD(slot, kb)                                                               \
  {                                                                                     \
    rq[slot] = *reinterpret_cast<const h4*>(qp + ((kb) << 4));                         \
    _Pragma("unroll") for (int s = 0; s < 4; ++s) rp[slot][s] = pp[(size_t)(((kb) << 4) + s) * ldp]; \
  }
#define DN_COMPUTE(slot)                                                                \
  { _Pragma("unroll") for (int s = 0; s < 4; ++s) acc[0] = DQN_MFMA((float)rp[slot][s], (float)rq[slot][s], acc[0]); }
  const int nkbN = nkb - nkb % NS;
  if (nkbN > 0) {
#pragma unroll
    for (int i = 0; i < NS; ++i) { DN_LOAD(i, i) DQN_PIN(); }
    int kb = 0;
    for (; kb + NS < nkbN; kb += NS) {
#pragma unroll
      for (int i = 0; i < NS; ++i) { DN_COMPUTE(i) DQN_PIN(); DN_LOAD(i, kb + NS + i) DQN_PIN(); }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) { DN_COMPUTE(i) }
  }
  for (int kb = nkbN; kb < nkb; ++kb) { DN_LOAD(0, kb) DN_COMPUTE(0) }
#undef DN_LOAD
#undef DN_COMPUTE
  park_accumulators<1>(smem, acc, wave, lane);
  __syncthreads();
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (wave == 0) v = reduce_accumulator<1>(smem, 0, lane);
  return v;
}
__device__ __forceinline__ void dgrad_narrow_body(const GemmProblem& pr, int tile_p, int tile_q, float* smem) {
  const f32x4 v = dgrad_narrow_tile<4>(pr, tile_p, tile_q, smem);
  if ((threadIdx.x >> 6) == 0) {
    const int lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
    const int q = tile_q * 16 + li, p = tile_p * 16 + (lg << 2);
    *reinterpret_cast<f32x4*>(pr.C + (size_t)q * pr.ldc + p) = v;
  }
}

// ================================ WGRAD ==============================================
// dW[n][j] = sum_m dY[m][n] X[m][j];  db[n] = sum_m dY[m][n].  P = X (KS, 64-wide blocks of
// j), Q = dY (KS, 64-wide blocks of n).  Tile = (64*TPB) x (64*TQB).  Kred (= rows m) % 16 == 0.
constexpr int kWgradRing = 4;   // register ring of wgrad_direct_body (8 measured slower inside the pair kernel: 16.4 vs 15.3 us)
template <int TPB, int TQB>
__device__ __forceinline__ void wgrad_direct_body(const GemmProblem& pr, int tile_p, int tile_q, float* smem) {
  constexpr int NACC = TPB * 4 * TQB * 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int p0 = tile_p * 64 * TPB, q0 = tile_q * 64 * TQB;
  const int Kw = pr.Kred >> 2;
  const int nst = Kw >> 2;                 // steps of 4 rows
  // (addresses as in fwd_lds_body: a wave-uniform base — this wave's rows, the tile's columns — and one 32-bit lane offset per
  // operand: row lg, columns 4 li; the steps advance the scalar base)
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const char* pp = reinterpret_cast<const char*>(pr.P + (size_t)(wave_u * Kw) * pr.ldp + p0);
  const char* qp = reinterpret_cast<const char*>(pr.Q + (size_t)(wave_u * Kw) * pr.ldq + q0);
  const uint32_t lofp = ((uint32_t)lg * (uint32_t)pr.ldp + (uint32_t)li * 4u) * 4u, lofq = ((uint32_t)lg * (uint32_t)pr.ldq + (uint32_t)li * 4u) * 4u;
  const size_t ldp = (size_t)pr.ldp * 4, ldq = (size_t)pr.ldq * 4;        // bytes
  const bool want_db = (pr.db != nullptr) && (tile_p == 0);

  f32x4 acc[NACC];   // index (((d*4 + qc)*TPB + b)*4 + pc)
#pragma unroll
  for (int e = 0; e < NACC; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 dbacc[TQB];
#pragma unroll
  for (int d = 0; d < TQB; ++d) dbacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
  // register ring of NS steps (4 rows of X and dY each): NS-1 steps of lookahead
  constexpr int NS = kWgradRing;
  f32x4 rp[NS][TPB], rq[NS][TQB];

#define WG_LOAD(slot, st)                                                               \
  {                                                                                     \
    _Pragma("unroll") for (int b = 0; b < TPB; ++b)                                     \
        rp[slot][b] = *reinterpret_cast<const f32x4*>(pp + (size_t)((st) << 2) * ldp + b * 256 + lofp); \
    _Pragma("unroll") for (int d = 0; d < TQB; ++d)                                     \
        rq[slot][d] = *reinterpret_cast<const f32x4*>(qp + (size_t)((st) << 2) * ldq + d * 256 + lofq); \
  }
#define WG_COMPUTE(slot)                                                                \
  {                                                                                     \
    _Pragma("unroll") for (int d = 0; d < TQB; ++d) {                                   \
      dbacc[d].x += rq[slot][d].x; dbacc[d].y += rq[slot][d].y;                         \
      dbacc[d].z += rq[slot][d].z; dbacc[d].w += rq[slot][d].w;                         \
      _Pragma("unroll") for (int qc = 0; qc < 4; ++qc)                                  \
      _Pragma("unroll") for (int b = 0; b < TPB; ++b)                                   \
      _Pragma("unroll") for (int pc = 0; pc < 4; ++pc)                                  \
          acc[((d * 4 + qc) * TPB + b) * 4 + pc] = DQN_MFMA(                            \
              rp[slot][b][pc], rq[slot][d][qc], acc[((d * 4 + qc) * TPB + b) * 4 + pc]); \
    }                                                                                   \
  }

  const int nstN = nst - nst % NS;
  if (nstN > 0) {
#pragma unroll
    for (int i = 0; i < NS; ++i) { WG_LOAD(i, i) DQN_PIN(); }
    int st = 0;
    for (; st + NS < nstN; st += NS) {
#pragma unroll
      for (int i = 0; i < NS; ++i) { WG_COMPUTE(i) DQN_PIN(); WG_LOAD(i, st + NS + i) DQN_PIN(); }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) { WG_COMPUTE(i) }
  }
  {   // the (up to NS - 1) remaining steps: every load first (minibatch 32: these two steps are the whole reduction)
    const int rem = nst - nstN;
    if (rem > 0) WG_LOAD(0, nstN)
    if (rem > 1) WG_LOAD(1, nstN + 1)
    if (rem > 2) WG_LOAD(2, nstN + 2)
    if (rem > 0) WG_COMPUTE(0)
    if (rem > 1) WG_COMPUTE(1)
    if (rem > 2) WG_COMPUTE(2)
  }
#undef WG_LOAD
#undef WG_COMPUTE

  park_accumulators<NACC>(smem, acc, wave, lane);
  float* sdb = smem + 4 * NACC * 64 * 4;      // [4 waves][TQB][16 li] float4
  if (want_db) {
#pragma unroll
    for (int d = 0; d < TQB; ++d) {
      f32x4 v = dbacc[d];
      // add the 4 lane groups (rows m+0..3): lanes l, l^16, l^32, l^48
      v.x += __shfl_xor(v.x, 16, 64); v.y += __shfl_xor(v.y, 16, 64); v.z += __shfl_xor(v.z, 16, 64); v.w += __shfl_xor(v.w, 16, 64);
      v.x += __shfl_xor(v.x, 32, 64); v.y += __shfl_xor(v.y, 32, 64); v.z += __shfl_xor(v.z, 32, 64); v.w += __shfl_xor(v.w, 32, 64);
      if (lg == 0) reinterpret_cast<f32x4*>(sdb)[(wave * TQB + d) * 16 + li] = v;
    }
  }
  __syncthreads();
  float ssq = 0.0f;
  // accumulators (d,qc,b,pc=0..3) form float4s over pc
#pragma unroll
  for (int g4 = 0; g4 < TQB * 4 * TPB; ++g4) {
    if ((g4 & 3) == wave) {
      const int b = g4 % TPB, dq = g4 / TPB, qc = dq & 3, d = dq >> 2;
      f32x4 r0 = reduce_accumulator<NACC>(smem, g4 * 4 + 0, lane);
      f32x4 r1 = reduce_accumulator<NACC>(smem, g4 * 4 + 1, lane);
      f32x4 r2 = reduce_accumulator<NACC>(smem, g4 * 4 + 2, lane);
      f32x4 r3 = reduce_accumulator<NACC>(smem, g4 * 4 + 3, lane);
      const int n = q0 + d * 64 + (li << 2) + qc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = p0 + b * 64 + (lg << 4) + (r << 2);
        const f32x4 v = f32x4{r0[r], r1[r], r2[r], r3[r]};
        ssq = fmaf(v.x, v.x, ssq); ssq = fmaf(v.y, v.y, ssq); ssq = fmaf(v.z, v.z, ssq); ssq = fmaf(v.w, v.w, ssq);
        *reinterpret_cast<f32x4*>(pr.C + (size_t)n * pr.ldc + p) = v;
      }
    }
  }
  if (want_db && wave == 0 && lane < 16 * TQB) {
    const int d = lane >> 4, l16 = lane & 15;
    const f32x4* s4 = reinterpret_cast<const f32x4*>(sdb);
    const f32x4 a0 = s4[(0 * TQB + d) * 16 + l16], a1 = s4[(1 * TQB + d) * 16 + l16];
    const f32x4 a2 = s4[(2 * TQB + d) * 16 + l16], a3 = s4[(3 * TQB + d) * 16 + l16];
    f32x4 v;
    v.x = (a0.x + a1.x) + (a2.x + a3.x); v.y = (a0.y + a1.y) + (a2.y + a3.y);
    v.z = (a0.z + a1.z) + (a2.z + a3.z); v.w = (a0.w + a1.w) + (a2.w + a3.w);
    *reinterpret_cast<f32x4*>(pr.db + q0 + d * 64 + (l16 << 2)) = v;
    ssq = fmaf(v.x, v.x, ssq); ssq = fmaf(v.y, v.y, ssq); ssq = fmaf(v.z, v.z, ssq); ssq = fmaf(v.w, v.w, ssq);
  }
  if (pr.partial != nullptr) {
    ssq = wave_sum64(ssq);
    __syncthreads();                       // every wave is done reading the parked tiles
    if (lane == 0) smem[wave] = ssq;
    __syncthreads();
    if (threadIdx.x == 0) pr.partial[tile_q * pr.tiles_p + tile_p] = (smem[0] + smem[1]) + (smem[2] + smem[3]);
  }
}

// ---- WGRAD, narrow: 16 columns of dY per workgroup ------------------------------------------
// The first tower layer's dW_0[n][j] has only K_in = 64 / 128 columns j: with 64 x 64 tiles it is 16 / 32
// workgroups whose waves each hold 4.2 us of MFMA (a latency-bound 8 us launch on a sliver of the chip).
// Here a workgroup owns 16 outputs n (one dY column per lane, scalar loads) x 64 columns j: a quarter of
// the MFMA chain per wave, four times the workgroups.  Same K split over the 4 waves, same fixed-order
// reduction; db and the sum-of-squares partial (slot = tile_q * tiles_p + tile_p over 16-wide tiles).
template <int TPB>
__device__ __forceinline__ void wgrad_narrow_body(const GemmProblem& pr, int tile_p, int tile_q, float* smem) {
  constexpr int NACC = TPB * 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int p0 = tile_p * 64 * TPB, q0 = tile_q * 16;
  const int Kw = pr.Kred >> 2;
  const int nst = Kw >> 2;
  // (addresses as in wgrad_direct_body; the dY operand one column per lane)
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const char* pp = reinterpret_cast<const char*>(pr.P + (size_t)(wave_u * Kw) * pr.ldp + p0);
  const char* qp = reinterpret_cast<const char*>(pr.Q + (size_t)(wave_u * Kw) * pr.ldq + q0);
  const uint32_t lofp = ((uint32_t)lg * (uint32_t)pr.ldp + (uint32_t)li * 4u) * 4u, lofq = ((uint32_t)lg * (uint32_t)pr.ldq + (uint32_t)li) * 4u;
  const size_t ldp = (size_t)pr.ldp * 4, ldq = (size_t)pr.ldq * 4;        // bytes
  const bool want_db = (pr.db != nullptr) && (tile_p == 0);
  f32x4 acc[NACC];
#pragma unroll
  for (int e = 0; e < NACC; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.0f;
  constexpr int NS = kWgradRing;
  f32x4 rp[NS][TPB]; float rq[NS];
#define WN_LOAD(slot, st)                                                               \
  {                                                                                     \
    _Pragma("unroll") for (int b = 0; b < TPB; ++b)                                     \
        rp[slot][b] = *reinterpret_cast<const f32x4*>(pp + (size_t)((st) << 2) * ldp + b * 256 + lofp); \
    rq[slot] = *reinterpret_cast<const float*>(qp + (size_t)((st) << 2) * ldq + lofq);  \
  }
#define WN_COMPUTE(slot)                                                                \
  {                                                                                     \
    dbacc += rq[slot];                                                                  \
    _Pragma("unroll") for (int b = 0; b < TPB; ++b)                                     \
    _Pragma("unroll") for (int pc = 0; pc < 4; ++pc)                                    \
        acc[b * 4 + pc] = DQN_MFMA(rp[slot][b][pc], rq[slot], acc[b * 4 + pc]);         \
  }
  const int nstN = nst - nst % NS;
  if (nstN > 0) {
#pragma unroll
    for (int i = 0; i < NS; ++i) { WN_LOAD(i, i) DQN_PIN(); }
    int st = 0;
    for (; st + NS < nstN; st += NS) {
#pragma unroll
      for (int i = 0; i < NS; ++i) { WN_COMPUTE(i) DQN_PIN(); WN_LOAD(i, st + NS + i) DQN_PIN(); }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) { WN_COMPUTE(i) }
  }
  for (int st = nstN; st < nst; ++st) { WN_LOAD(0, st) WN_COMPUTE(0) }
#undef WN_LOAD
#undef WN_COMPUTE

  park_accumulators<NACC>(smem, acc, wave, lane);
  float* sdb = smem + 4 * NACC * 64 * 4;      // [4 waves][16 li]
  if (want_db) {
    float v = dbacc;                          // add the 4 lane groups (rows m+0..3)
    v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
    if (lg == 0) sdb[wave * 16 + li] = v;
  }
  __syncthreads();
  float ssq = 0.0f;
#pragma unroll
  for (int b = 0; b < TPB; ++b) {
    const f32x4 r0 = reduce_accumulator<NACC>(smem, b * 4 + 0, lane), r1 = reduce_accumulator<NACC>(smem, b * 4 + 1, lane);
    const f32x4 r2 = reduce_accumulator<NACC>(smem, b * 4 + 2, lane), r3 = reduce_accumulator<NACC>(smem, b * 4 + 3, lane);
    const int n = q0 + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (((b + r) & 3) == wave) {           // the four row groups of an accumulator set are shared out over the waves
        const int p = p0 + b * 64 + (lg << 4) + (r << 2);
        const f32x4 v = f32x4{r0[r], r1[r], r2[r], r3[r]};
        ssq = fmaf(v.x, v.x, ssq); ssq = fmaf(v.y, v.y, ssq); ssq = fmaf(v.z, v.z, ssq); ssq = fmaf(v.w, v.w, ssq);
        *reinterpret_cast<f32x4*>(pr.C + (size_t)n * pr.ldc + p) = v;
      }
    }
  }
  if (want_db && wave == 0 && lane < 16) {
    const float v = (sdb[0 * 16 + lane] + sdb[1 * 16 + lane]) + (sdb[2 * 16 + lane] + sdb[3 * 16 + lane]);
    pr.db[q0 + lane] = v;
    ssq = fmaf(v, v, ssq);
  }
  if (pr.partial != nullptr) {
    ssq = wave_sum64(ssq);
    __syncthreads();
    if (lane == 0) smem[wave] = ssq;
    __syncthreads();
    if (threadIdx.x == 0) pr.partial[tile_q * pr.tiles_p + tile_p] = (smem[0] + smem[1]) + (smem[2] + smem[3]);
  }
}

// ================================ FWD, coalesced =====================================
// Same tile / split-K structure as fwd_direct_body, but the k-contiguous operands are
// fetched as WHOLE 128-byte lines (8 rows x 128 B per wave instruction) and transposed into
// MFMA fragment layout through a wave-private LDS image — the fragment-shaped loads of
// fwd_direct_body (sixteen 64-B pieces per instruction) run the texture addresser at 1/4
// rate: measured 8.5 TB/s vs 20 TB/s for the same bytes (ablation v6/v9).
//   global (coalesced)  lane l -> row l>>3, 16-B chunk l&7          [2 loads / 16 rows / 32 k]
//   LDS image per 16-row block: [16 rows][8 chunks], chunk ^= row&7 (ds_write_b128: 8 lanes
//   of a row hit 8 distinct chunks; ds_read_b128 in MFMA layout is conflict-free, see
//   DESIGN.md for the lane-group check)
//   fragment            lane (i=l&15, g=l>>4), kb -> row i, chunk kb*4+g
// The LDS image is private to the wave (no barrier anywhere in the main loop); two images
// ping-pong, global loads run two 32-k steps ahead in registers.
// Requires Kred % 256 == 0 and Kred >= 512 (>= 4 steps of 32 k per wave, even count).
// WT (probe only, csrc/gemm_bench.hip): the output tile is stored write-through (`sc1`), the producer side of an
// in-launch hand-off without a release fence (guide G16 R1).  The learner instantiates WT = false.
template <int TP, int TQ, bool PIN, int NSLOT = 2, bool WT = false>
__device__ __forceinline__ void fwd_lds_body(const GemmProblem& pr, int tile_p, int tile_q, float* smem) {
  constexpr int NB = TP + TQ;
  constexpr int NACC = TP * TQ;
  constexpr int SLOT = NB * 512;                 // floats per LDS image (NB blocks x 16 rows x 32 k)
  // NSLOT = 1: one image per wave.  LDS operations of one wave execute in issue order, so the next
  // step's ds_write cannot overtake this step's ds_read of the same image; half the LDS lets two
  // workgroups share a CU.
  constexpr int WSTR = (NSLOT * SLOT > NACC * 256) ? NSLOT * SLOT : NACC * 256;   // floats per wave region (images, later the parked tile)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int lr = lane >> 3, lc = lane & 7;
  const int p0 = tile_p * 16 * TP, q0 = tile_q * 16 * TQ;
  const int Kw = pr.Kred >> 2;
  const int T = Kw >> 5;                         // steps of 32 k
  // Operand addresses: per 16-row block ONE wave-uniform base (scalar registers: tile row, this wave's k range) and per operand
  // ONE per-lane 32-bit byte offset (row lr, chunk lc) — the loads take the scalar-base form; a 64-bit multiply-add and shift-add
  // per block pointer in the vector unit used to stand between the arguments' arrival and the first load.  (The lane offset is
  // at most 7 rows and 128 bytes: gemm_form_accepts bounds the leading dimensions, kMaxLeadingDim.)
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const char* gp[NB];
  size_t ld8[NB];                                              // 8 rows on, in bytes
  uint32_t lof[NB];
  const uint32_t lofp = ((uint32_t)lr * (uint32_t)pr.ldp + (uint32_t)lc * 4u) * 4u, lofq = ((uint32_t)lr * (uint32_t)pr.ldq + (uint32_t)lc * 4u) * 4u;
#pragma unroll
  for (int b = 0; b < NB; ++b) {               // (later blocks: the block before + 16 rows, a scalar add)
    if (b < TP) { gp[b] = b == 0 ? reinterpret_cast<const char*>(pr.P + (size_t)p0 * pr.ldp + wave_u * Kw) : gp[b > 0 ? b - 1 : 0] + (size_t)64 * pr.ldp; ld8[b] = (size_t)32 * pr.ldp; lof[b] = lofp; }
    else { gp[b] = b == TP ? reinterpret_cast<const char*>(pr.Q + (size_t)q0 * pr.ldq + wave_u * Kw) : gp[b > 0 ? b - 1 : 0] + (size_t)64 * pr.ldq; ld8[b] = (size_t)32 * pr.ldq; lof[b] = lofq; }
  }
  float* wsm = smem + wave * WSTR;
  const int woff = lr * 32 + ((lc ^ lr) << 2);                 // + h*256 + b*512
  int roff[2];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) roff[kb] = li * 32 + ((((kb << 2) + lg) ^ (li & 7)) << 2);

  f32x4 acc[NACC];
#pragma unroll
  for (int e = 0; e < NACC; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 G0[NB][2], G1[NB][2], F[NB][2], Fn[NB][2];

#define L_GLOAD(G, t)                                                                   \
  { _Pragma("unroll") for (int b = 0; b < NB; ++b) {                                    \
      G[b][0] = *reinterpret_cast<const f32x4*>(gp[b] + ((t) << 7) + lof[b]);          \
      G[b][1] = *reinterpret_cast<const f32x4*>(gp[b] + ld8[b] + ((t) << 7) + lof[b]); } }
#define L_SWRITE(slot, G)                                                               \
  { _Pragma("unroll") for (int b = 0; b < NB; ++b) {                                    \
      *reinterpret_cast<f32x4*>(wsm + ((slot) % NSLOT) * SLOT + b * 512 + woff) = G[b][0];        \
      *reinterpret_cast<f32x4*>(wsm + ((slot) % NSLOT) * SLOT + b * 512 + 256 + woff) = G[b][1]; } }
#define L_SREAD(FF, slot)                                                               \
  { _Pragma("unroll") for (int b = 0; b < NB; ++b) {                                    \
      FF[b][0] = *reinterpret_cast<const f32x4*>(wsm + ((slot) % NSLOT) * SLOT + b * 512 + roff[0]); \
      FF[b][1] = *reinterpret_cast<const f32x4*>(wsm + ((slot) % NSLOT) * SLOT + b * 512 + roff[1]); } }
#define L_MFMA(FF)                                                                      \
  { _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                    \
    _Pragma("unroll") for (int s = 0; s < 4; ++s)                                       \
    _Pragma("unroll") for (int a = 0; a < TQ; ++a)                                      \
    _Pragma("unroll") for (int c = 0; c < TP; ++c)                                      \
        acc[a * TP + c] = DQN_MFMA(FF[c][kb][s], FF[TP + a][kb][s], acc[a * TP + c]); }
#define L_PIN() { if (PIN) DQN_PIN(); }
  // PIN: every half step {stage the next image: ds_write x2NB, global_load x2NB, ds_read x2NB | MFMA of the
  // current fragments} is one scheduling region whose staging instructions are spread through the MFMAs
  // in that order (hipcc on its own either sinks the loads to the end of the iteration — zero lookahead —
  // or, with plain order pinning, issues the 3 x 2NB staging instructions as a block with the MFMA pipe idle)
  constexpr int NOPS = 2 * NB, NMF = 8 * NACC;
  constexpr int MW = (NMF >= 5 * NOPS) ? 2 : 1, ML = (NMF >= 5 * NOPS) ? 2 : (NMF >= 2 * NOPS ? 1 : 0),
                MR = (NMF >= 3 * NOPS) ? 1 : 0;          // small tiles: fewer MFMAs than staging instructions
  constexpr bool SGB = PIN && (NMF >= NOPS);
#define L_SCHED_(HASLD)                                                                 \
  { if constexpr (SGB) {                                                                \
      _Pragma("unroll") for (int i_ = 0; i_ < NOPS; ++i_) {                             \
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0); __builtin_amdgcn_sched_group_barrier(0x008, MW, 0); } \
      if (HASLD) { _Pragma("unroll") for (int i_ = 0; i_ < NOPS; ++i_) {                \
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); if (ML > 0) __builtin_amdgcn_sched_group_barrier(0x008, ML, 0); } } \
      _Pragma("unroll") for (int i_ = 0; i_ < NOPS; ++i_) {                             \
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); if (MR > 0) __builtin_amdgcn_sched_group_barrier(0x008, MR, 0); } \
      if (NMF - (MW + (HASLD ? ML : 0) + MR) * NOPS > 0)                                \
        __builtin_amdgcn_sched_group_barrier(0x008, NMF - (MW + (HASLD ? ML : 0) + MR) * NOPS, 0); } }
#define L_SCHED() L_SCHED_(true)

  // (pinned prologue: the waitcnt pass merges the prologue's load order into the loop header, so an
  // interleaved prologue makes every in-loop vmcnt wait conservative)
  L_GLOAD(G0, 0) L_PIN() L_GLOAD(G1, 1) L_PIN()
  L_SWRITE(0, G0) L_PIN() L_GLOAD(G0, 2) L_PIN() L_SREAD(F, 0) L_PIN()
  int t = 0;
  for (; t + 4 < T; t += 2) {
    if constexpr (SGB) {
      L_SWRITE(1, G1) L_GLOAD(G1, t + 3) L_SREAD(Fn, 1) L_MFMA(F) L_SCHED() L_PIN()
      L_SWRITE(0, G0) L_GLOAD(G0, t + 4) L_SREAD(F, 0) L_MFMA(Fn) L_SCHED() L_PIN()
    } else {
      L_SWRITE(1, G1) L_PIN() L_GLOAD(G1, t + 3) L_PIN() L_SREAD(Fn, 1) L_PIN()
      L_MFMA(F) L_PIN()
      L_SWRITE(0, G0) L_PIN() L_GLOAD(G0, t + 4) L_PIN() L_SREAD(F, 0) L_PIN()
      L_MFMA(Fn) L_PIN()
    }
  }
  // t == T-4
  if constexpr (SGB) {
    L_SWRITE(1, G1) L_GLOAD(G1, T - 1) L_SREAD(Fn, 1) L_MFMA(F) L_SCHED() L_PIN()
    L_SWRITE(0, G0) L_SREAD(F, 0) L_MFMA(Fn) L_SCHED_(false) L_PIN()
    L_SWRITE(1, G1) L_SREAD(Fn, 1) L_MFMA(F) L_SCHED_(false) L_PIN()
    L_MFMA(Fn)
  } else {
    L_SWRITE(1, G1) L_GLOAD(G1, T - 1) L_SREAD(Fn, 1) L_PIN()
    L_MFMA(F) L_PIN()
    L_SWRITE(0, G0) L_SREAD(F, 0) L_PIN()
    L_MFMA(Fn) L_PIN()
    L_SWRITE(1, G1) L_SREAD(Fn, 1) L_PIN()
    L_MFMA(F) L_PIN()
    L_MFMA(Fn)
  }
#undef L_GLOAD
#undef L_SWRITE
#undef L_SREAD
#undef L_MFMA
#undef L_PIN
#undef L_SCHED
#undef L_SCHED_

  // this wave's bias pieces, requested ahead of the cross-wave reduction
  constexpr int NBV = (NACC + 3) / 4;
  f32x4 bvp[NBV], swp[NBV], dwp[NBV];
  if (pr.bias != nullptr) {
#pragma unroll
    for (int j = 0; j < NBV; ++j) {
      const int e = j * 4 + wave;
      if (e < NACC) bvp[j] = *reinterpret_cast<const f32x4*>(pr.bias + p0 + (e % TP) * 16 + (lg << 2));
    }
  }
  if (pr.seed_w != nullptr) {
#pragma unroll
    for (int j = 0; j < NBV; ++j) {
      const int e = j * 4 + wave;
      if (e < NACC) swp[j] = *reinterpret_cast<const f32x4*>(pr.seed_w + p0 + (e % TP) * 16 + (lg << 2));
    }
  }
  if (pr.dot_w != nullptr) {
#pragma unroll
    for (int j = 0; j < NBV; ++j) {
      const int e = j * 4 + wave;
      if (e < NACC) dwp[j] = *reinterpret_cast<const f32x4*>(pr.dot_w + p0 + (e % TP) * 16 + (lg << 2));
    }
  }
  // park into this wave's own (now idle) staging region, reduce across waves in fixed order
  f32x4* park = reinterpret_cast<f32x4*>(wsm);
#pragma unroll
  for (int e = 0; e < NACC; ++e) park[e * 64 + lane] = acc[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < NACC; ++e) {
    if ((e & 3) == wave) {
      const int a = e / TP, c = e % TP;
      const f32x4 a0 = reinterpret_cast<const f32x4*>(smem + 0 * WSTR)[e * 64 + lane];
      const f32x4 a1 = reinterpret_cast<const f32x4*>(smem + 1 * WSTR)[e * 64 + lane];
      const f32x4 a2 = reinterpret_cast<const f32x4*>(smem + 2 * WSTR)[e * 64 + lane];
      const f32x4 a3 = reinterpret_cast<const f32x4*>(smem + 3 * WSTR)[e * 64 + lane];
      f32x4 v;
      v.x = (a0.x + a1.x) + (a2.x + a3.x); v.y = (a0.y + a1.y) + (a2.y + a3.y);
      v.z = (a0.z + a1.z) + (a2.z + a3.z); v.w = (a0.w + a1.w) + (a2.w + a3.w);
      const int q = q0 + a * 16 + li, p = p0 + c * 16 + (lg << 2);
      if (pr.bias != nullptr) {
        const f32x4 bv = bvp[e >> 2];
        v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
      }
      if (pr.relu) { v.x = lrelu_fwd(v.x); v.y = lrelu_fwd(v.y); v.z = lrelu_fwd(v.z); v.w = lrelu_fwd(v.w); }
      if constexpr (WT) {
        typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(pr.C, 0, pr.Qdim * pr.ldc * 4, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), rs, (int)(((size_t)q * pr.ldc + p) * 4), 0, 16 /* sc1 */);
      } else {
        *reinterpret_cast<f32x4*>(pr.C + (size_t)q * pr.ldc + p) = v;
      }
      if (pr.seed_w != nullptr) store_head_seed(pr, q, p, v, swp[e >> 2]);
      if (pr.dot_w != nullptr) store_head_dot(pr, q, p, lg, v, dwp[e >> 2]);
    }
  }
}

// ================================ DGRAD, coalesced ===================================
// dgrad_direct_body with the k-contiguous operand (dY, 16-row blocks) fetched as whole 128-B
// lines through the wave-private LDS transpose of fwd_lds_body; the weight operand (k-strided)
// stays a direct full-line load.  Requires Kred % 256 == 0 and Kred >= 512.
// s_rowscale (LDS, [16 TQ] floats, published before this body's barrier by a wave that does not run it — k_dgrad_qtrain): the
// reduced sums of row r are multiplied by s_rowscale[r] before the ReLU' mask (a dY panel whose rows share a late-known scalar factor)
// hook (k_dgrad_qtrain): after_prologue() runs once the operand pipeline is primed (a place to REQUEST data whose latency the
// main loop then hides), before_park() after the last MFMA and before this body's only barrier (a place to publish s_rowscale).
struct DgradNoHook { __device__ __forceinline__ void after_prologue() {} __device__ __forceinline__ void before_park() {} };
template <int TPB, int TQ, bool SCH = true, typename Hook = DgradNoHook>
__device__ __forceinline__ void dgrad_lds_body(const GemmProblem& pr, int tile_p, int tile_q, float* smem, const float* s_rowscale, Hook& hook) {
  constexpr int NACC = TPB * 4 * TQ;
  constexpr int SLOT = TQ * 512;
  constexpr int WAVE_FLOATS = (2 * SLOT > NACC * 256) ? 2 * SLOT : NACC * 256;   // staging, later the parked tile
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int lr = lane >> 3, lc = lane & 7;
  const int p0 = tile_p * 64 * TPB, q0 = tile_q * 16 * TQ;
  const int Kw = pr.Kred >> 2;
  const int T = Kw >> 5;
  float* wsm = smem + wave * WAVE_FLOATS;
  // (addresses as in fwd_lds_body: wave-uniform bases and 32-bit lane offsets.  dY: row lr, chunk lc of a 16-row block.  W: the
  // lane's row 4 lg + s2 of a 16-row k block, columns 4 li — one lane offset per s2, so that a step needs two scalar bases, not eight)
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const char* pp = reinterpret_cast<const char*>(pr.P + (size_t)(wave_u * Kw) * pr.ldp + p0);
  const size_t ldp = (size_t)pr.ldp * 4;                                   // bytes
  uint32_t lofp[4];
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2) lofp[s2] = ((uint32_t)(lg * 4 + s2) * (uint32_t)pr.ldp + (uint32_t)li * 4u) * 4u;
  const char* gq[TQ];
#pragma unroll
  for (int a = 0; a < TQ; ++a) gq[a] = a == 0 ? reinterpret_cast<const char*>(pr.Q + (size_t)q0 * pr.ldq + wave_u * Kw) : gq[a > 0 ? a - 1 : 0] + (size_t)64 * pr.ldq;
  const uint32_t lofq = ((uint32_t)lr * (uint32_t)pr.ldq + (uint32_t)lc * 4u) * 4u;
  const size_t ldq8 = (size_t)32 * pr.ldq;                                 // 8 rows on, in bytes
  const int woff = lr * 32 + ((lc ^ lr) << 2);
  int roff[2];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) roff[kb] = li * 32 + ((((kb << 2) + lg) ^ (li & 7)) << 2);

  f32x4 mk[TQ * TPB];
  f32x4 acc[NACC];
#pragma unroll
  for (int e = 0; e < NACC; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 G0[TQ][2], G1[TQ][2], F[TQ][2], Fn[TQ][2];
  f32x4 P0[2][4][TPB], P1[2][4][TPB];

#define D_GLOADQ(G, t)                                                                  \
  { _Pragma("unroll") for (int a = 0; a < TQ; ++a) {                                    \
      G[a][0] = *reinterpret_cast<const f32x4*>(gq[a] + ((t) << 7) + lofq);            \
      G[a][1] = *reinterpret_cast<const f32x4*>(gq[a] + ldq8 + ((t) << 7) + lofq); } }
#define D_GLOADP(PP, t)                                                                 \
  { _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                    \
    _Pragma("unroll") for (int s2 = 0; s2 < 4; ++s2)                                    \
    _Pragma("unroll") for (int b = 0; b < TPB; ++b)                                     \
        PP[kb][s2][b] = *reinterpret_cast<const f32x4*>(pp + (size_t)(((t) << 5) + (kb << 4)) * ldp + b * 256 + lofp[s2]); }
#define D_SWRITE(slot, G)                                                               \
  { _Pragma("unroll") for (int a = 0; a < TQ; ++a) {                                    \
      *reinterpret_cast<f32x4*>(wsm + (slot) * SLOT + a * 512 + woff) = G[a][0];        \
      *reinterpret_cast<f32x4*>(wsm + (slot) * SLOT + a * 512 + 256 + woff) = G[a][1]; } }
#define D_SREAD(FF, slot)                                                               \
  { _Pragma("unroll") for (int a = 0; a < TQ; ++a) {                                    \
      FF[a][0] = *reinterpret_cast<const f32x4*>(wsm + (slot) * SLOT + a * 512 + roff[0]); \
      FF[a][1] = *reinterpret_cast<const f32x4*>(wsm + (slot) * SLOT + a * 512 + roff[1]); } }
#define D_MFMA(FF, PP)                                                                  \
  { _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                    \
    _Pragma("unroll") for (int s2 = 0; s2 < 4; ++s2)                                    \
    _Pragma("unroll") for (int a = 0; a < TQ; ++a)                                      \
    _Pragma("unroll") for (int b = 0; b < TPB; ++b)                                     \
    _Pragma("unroll") for (int pc = 0; pc < 4; ++pc)                                    \
        acc[(a * TPB + b) * 4 + pc] = DQN_MFMA(PP[kb][s2][b][pc], FF[a][kb][s2], acc[(a * TPB + b) * 4 + pc]); }

  // One scheduling region per half step, staging instructions spread through the MFMAs in this order
  // (see fwd_lds_body): dY image ds_writes, next dY loads, fragment ds_reads among the first MFMAs;
  // the W loads that refill the P registers among the second half (their registers are free once the
  // kb = 0 MFMAs have issued).  Pinned prologue so that the in-loop vmcnt waits are counted, not 0.
  constexpr int NQ = 2 * TQ, NPL = 8 * TPB, NMF = 32 * TQ * TPB, HALF = NMF / 2;
#define D_PIN() { if (SCH) DQN_PIN(); }
#define D_SCHED_(HASQ, HASP)                                                            \
  if constexpr (SCH) { _Pragma("unroll") for (int i_ = 0; i_ < NQ; ++i_) {                                 \
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0); __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); } \
    if (HASQ) { _Pragma("unroll") for (int i_ = 0; i_ < NQ; ++i_) {                     \
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); } } \
    _Pragma("unroll") for (int i_ = 0; i_ < NQ; ++i_) {                                 \
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); } \
    __builtin_amdgcn_sched_group_barrier(0x008, HALF - (HASQ ? 3 : 2) * NQ, 0);         \
    if (HASP) { _Pragma("unroll") for (int i_ = 0; i_ < NPL; ++i_) {                    \
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); __builtin_amdgcn_sched_group_barrier(0x008, HALF / NPL, 0); } } \
    else __builtin_amdgcn_sched_group_barrier(0x008, HALF, 0);                          \
    DQN_PIN(); }

  D_GLOADQ(G0, 0) D_PIN() D_GLOADQ(G1, 1) D_PIN() D_GLOADP(P0, 0) D_PIN()
  // this lane's pieces of the ReLU' mask (one per (a,b): the r this wave owns in the epilogue), requested ahead of the main loop so
  // that their latency is not exposed after it — and behind the first operand requests: pr.mask / pr.ldm are cold launch arguments,
  // a scalar round trip of their own that the operand loads above do not wait for
  if (pr.mask != nullptr) {
#pragma unroll
    for (int ab = 0; ab < TQ * TPB; ++ab) {
      const int r = (wave - ab) & 3;
      mk[ab] = *reinterpret_cast<const f32x4*>(pr.mask + (size_t)(q0 + (ab / TPB) * 16 + li) * pr.ldm + p0 + (ab % TPB) * 64 + (lg << 4) + (r << 2));
    }
  }
  D_PIN()
  hook.after_prologue(); D_PIN()      // (with the first, cold round of operand requests: later, its cold misses hold up the in-order vmcnt of the loop's loads)
  D_SWRITE(0, G0) D_PIN() D_GLOADQ(G0, 2) D_PIN() D_SREAD(F, 0) D_PIN() D_GLOADP(P1, 1) D_PIN()
  int t = 0;
  for (; t + 4 < T; t += 2) {
    D_SWRITE(1, G1) D_GLOADQ(G1, t + 3) D_SREAD(Fn, 1) D_MFMA(F, P0) D_GLOADP(P0, t + 2) D_SCHED_(true, true)
    D_SWRITE(0, G0) D_GLOADQ(G0, t + 4) D_SREAD(F, 0) D_MFMA(Fn, P1) D_GLOADP(P1, t + 3) D_SCHED_(true, true)
  }
  // t == T-4
  D_SWRITE(1, G1) D_GLOADQ(G1, T - 1) D_SREAD(Fn, 1) D_MFMA(F, P0) D_GLOADP(P0, T - 2) D_SCHED_(true, true)
  D_SWRITE(0, G0) D_SREAD(F, 0) D_MFMA(Fn, P1) D_GLOADP(P1, T - 1) D_SCHED_(false, true)
  D_SWRITE(1, G1) D_SREAD(Fn, 1) D_MFMA(F, P0) D_SCHED_(false, false)
  D_MFMA(Fn, P1)
  D_PIN() hook.before_park();
#undef D_SCHED_
#undef D_PIN
#undef D_GLOADQ
#undef D_GLOADP
#undef D_SWRITE
#undef D_SREAD
#undef D_MFMA

  f32x4* park = reinterpret_cast<f32x4*>(wsm);
#pragma unroll
  for (int e = 0; e < NACC; ++e) park[e * 64 + lane] = acc[e];
  __syncthreads();
  auto red = [&](int e) {
    const f32x4 a0 = reinterpret_cast<const f32x4*>(smem + 0 * WAVE_FLOATS)[e * 64 + lane];
    const f32x4 a1 = reinterpret_cast<const f32x4*>(smem + 1 * WAVE_FLOATS)[e * 64 + lane];
    const f32x4 a2 = reinterpret_cast<const f32x4*>(smem + 2 * WAVE_FLOATS)[e * 64 + lane];
    const f32x4 a3 = reinterpret_cast<const f32x4*>(smem + 3 * WAVE_FLOATS)[e * 64 + lane];
    f32x4 v;
    v.x = (a0.x + a1.x) + (a2.x + a3.x); v.y = (a0.y + a1.y) + (a2.y + a3.y);
    v.z = (a0.z + a1.z) + (a2.z + a3.z); v.w = (a0.w + a1.w) + (a2.w + a3.w);
    return v;
  };
#pragma unroll
  for (int ab = 0; ab < TQ * TPB; ++ab) {
    // with TQ*TPB < 4 the four pc-accumulator groups of one (a,b) are shared out over the waves by r
    const int a = ab / TPB, b = ab % TPB;
    const f32x4 r0 = red(ab * 4 + 0), r1 = red(ab * 4 + 1), r2 = red(ab * 4 + 2), r3 = red(ab * 4 + 3);
    const int q = q0 + a * 16 + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (((ab + r) & 3) == wave) {
        const int p = p0 + b * 64 + (lg << 4) + (r << 2);
        f32x4 v = f32x4{r0[r], r1[r], r2[r], r3[r]};
        if (s_rowscale != nullptr) { const float sc = s_rowscale[a * 16 + li]; v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc; }
        if (pr.mask != nullptr) {
          const f32x4 mv = mk[ab];
          v.x *= lrelu_mask(mv.x); v.y *= lrelu_mask(mv.y); v.z *= lrelu_mask(mv.z); v.w *= lrelu_mask(mv.w);
        }
        *reinterpret_cast<f32x4*>(pr.C + (size_t)q * pr.ldc + p) = v;
      }
    }
  }
}

// ---- rider blocks ------------------------------------------------------------------------
// q(s, mu(s)) = q_values(critic tower top) and its avg-Q partials (src/dqn.cpp:913-916) as RIDER blocks of the narrow dgrad
// launch: a handful of 16 x 16 tiles (16 workgroups at 256 rows) that leaves most of the chip idle.  Nothing on the
// backward chain reads q — only the update's statistics do — so it needs no launch of its own (it used to ride in the
// dq = -1 head-backward launch, which is gone: the seed comes out of the top layer's forward epilogue, GemmProblem::seed_w).
// One wave per row, k-strips of float4; the riders come LAST in the grid.
__device__ __forceinline__ void q_head_rider(const QHeadRider& r, const int blk) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blk * 4 + wave;
  if (row >= r.rows) return;
  const size_t x0 = (size_t)row * r.H;
  float acc = 0.0f;
  if (r.X416 != nullptr) {
    typedef __attribute__((ext_vector_type(4))) _Float16 h4;
    for (int k = lane * 4; k < r.H; k += 256) {
      const h4 xh = *reinterpret_cast<const h4*>(r.X416 + x0 + k); const f32x4 wv = *reinterpret_cast<const f32x4*>(r.W + k);
      acc = fmaf((float)xh.x, wv.x, acc); acc = fmaf((float)xh.y, wv.y, acc); acc = fmaf((float)xh.z, wv.z, acc); acc = fmaf((float)xh.w, wv.w, acc);
    }
  } else
  for (int k = lane * 4; k < r.H; k += 256) {
    const f32x4 xv = *reinterpret_cast<const f32x4*>(r.X4 + x0 + k), wv = *reinterpret_cast<const f32x4*>(r.W + k);
    acc = fmaf(xv.x, wv.x, acc); acc = fmaf(xv.y, wv.y, acc); acc = fmaf(xv.z, wv.z, acc); acc = fmaf(xv.w, wv.w, acc);
  }
  acc = wave_sum64(acc);
  if (lane == 0) { const float v = acc + r.bias[0]; r.q_out[row] = v; r.qsum_partial[row] = (double)v; }
}

// The head layer's weight / bias gradients (dWh[j][k] = sum_m dYh[m][j] X4[m][k], dbh[j] = sum_m dYh[m][j]) as RIDER blocks of a
// later launch of the same net's backward.  The head-backward kernel produces dZ for that launch and used to produce dWh too — through
// row-chunk slabs and an arrival counter whose tail (drain, barrier, counter, barrier, slab reads) was 2.5 us per launch at the end
// of a 5-8 us kernel.  Nothing before the optimiser pass reads dWh, and a rider block (8 columns x 32 row groups, every row of its
// columns: no cross-block reduction) is done in ~3 us.  dy: the head diffs the head-backward kernel consumed (critic: dq [rows]; actor: the post-invert diffs [rows][16]).
template <int NH>
__device__ __forceinline__ void head_wgrad_rider(const HeadWgradRider& r, const int blk, float* smem) {
  constexpr int CW = kRiderCW, RG = 256 / CW;
  const int tid = threadIdx.x, kc = tid % CW, rg = tid / CW;
  const int k = blk * CW + kc;
  float* s_dy = smem;                          // [rows][NH]
  float* s_acc = smem + r.rows * NH;           // [RG][NH][CW]
  const int per = (r.rows + RG - 1) / RG, m0 = rg * per, m1 = m0 + per < r.rows ? m0 + per : r.rows;
  constexpr int RB = 8;                        // every row of a 256-row minibatch in flight at once: the tower top was written
                                               // many launches ago (Infinity Cache / HBM latency, not L2)
  float xpre[RB];
#pragma unroll
  for (int u = 0; u < RB; ++u) xpre[u] = (m0 + u < m1) ? r.X4[(size_t)(m0 + u) * r.H + k] : 0.0f;
  for (int i = tid; i < r.rows * NH; i += 256) s_dy[i] = r.dy[(size_t)(i / NH) * r.lddy + (i % NH)];
  __syncthreads();
  float acc[NH];
#pragma unroll
  for (int j = 0; j < NH; ++j) acc[j] = 0.0f;
  for (int mb = m0; mb < m1; mb += RB) {
    float xb[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) xb[u] = (mb == m0) ? xpre[u] : ((mb + u < m1) ? r.X4[(size_t)(mb + u) * r.H + k] : 0.0f);
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const int m = mb + u;
      if (m >= m1) break;
#pragma unroll
      for (int j = 0; j < NH; ++j) acc[j] = fmaf(s_dy[m * NH + j], xb[u], acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < NH; ++j) s_acc[(rg * NH + j) * CW + kc] = acc[j];
  __syncthreads();
  float ssq = 0.0f;
  if (tid < NH * CW) {                         // row groups added in index order
    const int j = tid / CW, c = tid % CW;
    float v = 0.0f;
#pragma unroll 8
    for (int g = 0; g < RG; ++g) v += s_acc[(g * NH + j) * CW + c];
    r.dW[(size_t)j * r.H + blk * CW + c] = v;
    ssq = v * v;
  } else if (blk == 0 && tid < NH * CW + NH) { // bias gradient: rows in index order
    const int j = tid - NH * CW;
    float v = 0.0f;
    for (int m = 0; m < r.rows; ++m) v += s_dy[m * NH + j];
    r.db[j] = v;
    ssq = v * v;
  }
  ssq = wave_sum64(ssq);
  __syncthreads();
  if ((tid & 63) == 0) s_acc[tid >> 6] = ssq;
  __syncthreads();
  if (tid == 0 && r.partial != nullptr) r.partial[blk] = (s_acc[0] + s_acc[1]) + (s_acc[2] + s_acc[3]);
}

}  // namespace dqnhip
