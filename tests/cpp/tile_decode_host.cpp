// Host-side check of what stands between a GEMM launch's arguments and its first operand load (dqn-hfo_amd/csrc/gemm_bodies.hip.h,
// gemm_direct.hip.h): the division-free tile decode against tile_of_counts, the reciprocal pack_args() stores for it, and the bound
// under which a lane's 32-bit operand offset cannot wrap.  No HIP call is made: runs on a box without a GPU.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gemm_direct.hip.h"

using namespace dqnhip;

static long fails = 0;
#define EXPECT(c) do { if (!(c)) { if (fails < 20) std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static GemmBatch batch_of(const std::vector<std::pair<int, int>>& tiles, bool grouped = true) {
  GemmBatch b{}; b.n = (int)tiles.size();
  int base = 0;
  for (int i = 0; i < b.n; ++i) {
    GemmProblem& p = b.prob[i];
    p.tiles_p = tiles[i].first; p.tiles_q = tiles[i].second; p.tile_base = grouped ? base : 0;
    p.ldp = 64; p.ldq = 64; p.ldc = 64;
    base = (int)((int64_t)base + (int64_t)p.tiles_p * p.tiles_q);
  }
  b.total_tiles = base;
  return b;
}

int main() {
  // 1. tile_decode == tile_of_counts over the WHOLE range pack_args lets through (tile_magic_covers): every tiles_q in
  // [1, kTileDecodeMaxQ] and, for each, every block index of the largest problem on either side of the tiles_p % 8 switch —
  // tiles_p = the largest multiple of 8 with tiles_p tiles_q <= kTileDecodeMaxTiles (the XCD map: j = b >> 3) and the largest
  // tiles_p that is none (j = b).  The decode reads tiles_p only through that switch, so smaller problems of the same tiles_q see
  // a prefix of these block indices: nothing the forms can produce lies outside the sweep.
  long swept = 0;
  for (int tq = 1; tq <= kTileDecodeMaxQ; ++tq) {
    const uint32_t magic = tile_magic(tq);
    const int tp_max = kTileDecodeMaxTiles / tq;
    const int tp_x = tp_max & ~7, tp_n = (tp_max & 7) ? tp_max : tp_max - 1;
    for (int tp : {tp_x, tp_n}) {
      if (tp < 1) continue;
      EXPECT(tile_magic_covers(tp, tq));
      long bad = 0;
      for (int b = 0; b < tp * tq; ++b) {
        int p, q, rp, rq;
        tile_decode(tp, tq, magic, b, p, q);
        tile_of_counts(tp, tq, b, rp, rq);
        bad += (p != rp) | (q != rq);
      }
      EXPECT(bad == 0);
      swept += (long)tp * tq;
    }
  }
  // the small counts of packed_args_host.cpp's bijection check, both maps
  for (int tp = 1; tp <= 48; ++tp)
    for (int tq = 1; tq <= 9; ++tq)
      for (int b = 0; b < tp * tq; ++b) {
        int p, q, rp, rq;
        tile_decode(tp, tq, tile_magic(tq), b, p, q);
        tile_of_counts(tp, tq, b, rp, rq);
        EXPECT(p == rp && q == rq);
      }
  // 2. pack_args: the reciprocal of every problem, group sizes 1 to 4, in every record count the kernels carry
  const std::vector<std::pair<int, int>> shapes = {{8, 3}, {5, 6}, {16, 12}, {20, 1}};
  for (int n = 1; n <= kMaxGroup; ++n) {
    const GemmBatch b = batch_of({shapes.begin(), shapes.begin() + n});
    GemmArgs<kMaxGroup> a;
    EXPECT(pack_args(b, a));
    for (int i = 0; i < n; ++i) {
      EXPECT(a.hot[i].tq_magic == tile_magic(shapes[i].second));
      EXPECT(a.hot[i].tq_magic == (uint32_t)((0x80000000ull + shapes[i].second - 1) / shapes[i].second));
    }
    if (n <= 2) { GemmArgs<2> a2; EXPECT(pack_args(b, a2) && a2.hot[n - 1].tq_magic == tile_magic(shapes[n - 1].second)); }
    if (n == 1) { GemmArgs<1> a1; EXPECT(pack_args(b, a1) && a1.hot[0].tq_magic == tile_magic(shapes[0].second)); }
  }
  {   // ... and refuses what lies outside the swept range, on each side of each bound
    GemmArgs<kMaxGroup> a;
    EXPECT(pack_args(batch_of({{1, kTileDecodeMaxQ}}), a));
    EXPECT(!pack_args(batch_of({{1, kTileDecodeMaxQ + 1}}), a));
    EXPECT(pack_args(batch_of({{kTileDecodeMaxTiles / 8, 8}}), a));
    EXPECT(!pack_args(batch_of({{kTileDecodeMaxTiles / 8 + 1, 8}}), a));
    EXPECT(!pack_args(batch_of({{8, 3}, {kTileDecodeMaxTiles, 2}}), a));
    EXPECT(!pack_args(batch_of({{1 << 20, 1 << 12}}), a));                      // (a count that overflows int)
    GemmArgs<2> a2;
    EXPECT(!pack_args(batch_of({{8, 3}, {1, kTileDecodeMaxQ + 1}}, false), a2, false));
  }
  // 3. the lanes' 32-bit operand offsets.  Every body forms (row * ld + column) * 4 bytes in 32 bits with row <= 15 (fwd_direct: li;
  // dgrad: 4 lg + s2) and column <= 60 (wgrad: 4 li): at the largest accepted leading dimension the offset of the last element a
  // lane reaches (its float4's last float) is what 64-bit arithmetic gives; one more row of that pitch would wrap.
  {
    const uint64_t ld = kMaxLeadingDim;
    const uint32_t off32 = ((uint32_t)15 * (uint32_t)ld + 60u) * 4u;
    const uint64_t off64 = (15 * ld + 60) * 4;
    EXPECT(off32 == off64 && off64 + 16 <= (1ull << 32));
    EXPECT((16 * ld + 60) * 4 >= (1ull << 32));
    GemmBatch b{}; b.n = 1;
    GemmProblem& p = b.prob[0];
    p.mode = GEMM_FWD; p.Pdim = 64; p.Qdim = 32; p.Kred = 512; p.ldp = kMaxLeadingDim; p.ldq = kMaxLeadingDim; p.ldc = 64;
    EXPECT(gemm_form_accepts(GEMM_FORM_FWD_LDS_2x2, b));
    tile_batch(b, 32, 32);
    GemmArgs<kMaxGroup> a;
    EXPECT(pack_args(b, a));
    p.ldp = kMaxLeadingDim + 1;
    EXPECT(!gemm_form_accepts(GEMM_FORM_FWD_LDS_2x2, b) && !pack_args(b, a));
    p.ldp = 512; p.ldq = kMaxLeadingDim + 1;
    EXPECT(!gemm_form_accepts(GEMM_FORM_FWD_LDS_2x2, b) && !pack_args(b, a));
    p.ldq = 512;
    EXPECT(gemm_form_accepts(GEMM_FORM_FWD_LDS_2x2, b) && pack_args(b, a));
  }
  if (fails) { std::printf("%ld checks failed\n", fails); return 1; }
  std::printf("tile decode host OK (%ld block indices swept)\n", swept);
  return 0;
}
