// Host-side check of the kernarg preload block (GemmPreload, dqn-hfo_amd/csrc/gemm_common.hip.h): the 14 words a chain kernel
// receives in SGPRs at wave launch, built by make_preload_grouped / make_preload_record (gemm_bodies.hip.h) from a packed GemmArgs
// and decoded by preload_decode (grouped forms) / preload_record_decode (record form) — the functions the kernels call.  For every form the decode must equal the fields of the packed
// GemmArgs for every tile of problems 0 and 1, and whatever a field cannot hold must make the block "not valid" (all zero), never
// a truncated value.  No HIP call is made: runs on a box without a GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gemm_direct.hip.h"
#include "head_kernels.hip.h"

using namespace dqnhip;

static long fails = 0;
#define EXPECT(c) do { if (!(c)) { if (fails < 20) std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static float arena[64];     // operand "addresses": only compared, never read

struct Shape { int tp, tq, ldp, ldq, kred; };
static GemmBatch batch_of(const std::vector<Shape>& s, bool grouped = true) {
  GemmBatch b{}; b.n = (int)s.size();
  int base = 0;
  for (int i = 0; i < b.n; ++i) {
    GemmProblem& p = b.prob[i];
    p.tiles_p = s[i].tp; p.tiles_q = s[i].tq; p.tile_base = grouped ? base : 0;
    p.ldp = s[i].ldp; p.ldq = s[i].ldq; p.ldc = 64 + i; p.Kred = s[i].kred;
    p.P = arena + 4 * i; p.Q = arena + 4 * i + 1; p.C = arena + 4 * i + 2;
    base += p.tiles_p * p.tiles_q;
  }
  b.total_tiles = base;
  return b;
}
static bool all_zero(const GemmPreload& w) {
  const GemmPreload z{};
  return std::memcmp(&w, &z, sizeof w) == 0;
}
// tile b of a valid block against record pi of the packed arguments; want_pi: the problem index the decode must report (a lone
// record is the block's problem 0 whichever record of the launch it is)
template <int N>
static long check_tile(const GemmPreload& w, const GemmArgs<N>& a, int b, int pi, int want_pi) {
  const PreTile t = preload_decode(w, b);
  const GemmHot& h = a.hot[pi];
  int rp, rq;
  tile_decode(a.head.tiles_p[pi], a.head.tiles_q[pi], h.tq_magic, b - a.head.tile_base[pi], rp, rq);
  return (t.pi != want_pi) | (t.tile_p != rp) | (t.tile_q != rq) | (t.tiles_p != a.head.tiles_p[pi]) | (t.tiles_q != a.head.tiles_q[pi]) |
         (t.tile_base != a.head.tile_base[pi]) | (t.P != h.P) | (t.Q != h.Q) | ((int)w.ldp != h.ldp) | ((int)w.ldq != h.ldq) | ((int)w.Kred != h.Kred);
}

int main() {
  long swept = 0;
  // the tile counts: the small ones on both sides of the tiles_p % 8 switch, and pack_args' own limits (kTileDecodeMaxQ row tiles,
  // kTileDecodeMaxTiles tiles, either side of the switch)
  std::vector<std::pair<int, int>> counts;
  for (int tp = 1; tp <= 24; ++tp)
    for (int tq = 1; tq <= 9; ++tq) counts.push_back({tp, tq});
  counts.push_back({kTileDecodeMaxTiles, 1}); counts.push_back({kTileDecodeMaxTiles - 1, 1});
  counts.push_back({kTileDecodeMaxTiles / kTileDecodeMaxQ, kTileDecodeMaxQ}); counts.push_back({kTileDecodeMaxTiles / kTileDecodeMaxQ - 1, kTileDecodeMaxQ});
  counts.push_back({kTileDecodeMaxTiles / 8, 8}); counts.push_back({255, 1023});
  const int lds[] = {64, 1000, kMaxLeadingDim};
  const int kreds[] = {64, 512, 1 << 20};

  // 1. one problem (gemm_fwd_lds<2,2,true,2>, gemm_dgrad_lds<1,1>): every tile
  for (const auto& c : counts)
    for (int ld : lds)
      for (int kr : kreds) {
        if ((c.first > 64 || c.second > 64) && (ld != kMaxLeadingDim || kr != 512)) continue;       // the large counts once
        const GemmBatch b = batch_of({{c.first, c.second, ld, ld == 64 ? 128 : ld, kr}});
        GemmArgs<kMaxGroup> a;
        EXPECT(pack_args(b, a));
        const GemmPreload w = make_preload_grouped(a, false);
        EXPECT((w.flags & kPreValid) && (w.flags >> kPreSplitShift) == kPreNoSplit && w.P1 == nullptr && w.Q1 == nullptr);
        long bad = 0;
        for (int t = 0; t < b.total_tiles; ++t) bad += check_tile(w, a, t, 0, 0);
        EXPECT(bad == 0);
        swept += b.total_tiles;
        EXPECT(all_zero(make_preload_grouped(a, true)));                    // the tuning bit
      }
  // 2. two problems of equal shape, different pointers (gemm_fwd_lds<4,2,true,1>): every tile of both
  for (const auto& c : counts)
    for (int ld : lds) {
      if ((int64_t)c.first * c.second * 2 > kTileDecodeMaxTiles * 2) continue;
      if ((c.first > 64 || c.second > 64) && ld != kMaxLeadingDim) continue;
      const Shape s{c.first, c.second, ld, ld, 512};
      const GemmBatch b = batch_of({s, s});
      GemmArgs<kMaxGroup> a;
      EXPECT(pack_args(b, a));
      const GemmPreload w = make_preload_grouped(a, false);
      EXPECT((w.flags & kPreValid) && (int)(w.flags >> kPreSplitShift) == c.first * c.second);
      EXPECT(w.P0 != w.P1 && w.Q0 != w.Q1);
      long bad = 0;
      const int n = c.first * c.second;
      for (int t = 0; t < 2 * n; ++t) bad += check_tile(w, a, t, t >= n, t >= n);
      EXPECT(bad == 0);
      swept += 2 * n;
      EXPECT(all_zero(make_preload_grouped(a, true)));
      GemmArgs<2> a2;
      EXPECT(pack_args(b, a2));
      const GemmPreload w2 = make_preload_grouped(a2, false);
      EXPECT(std::memcmp(&w, &w2, sizeof w) == 0);
    }
  // 3. what the block cannot express: "not valid", all zero
  {
    const Shape s{8, 3, 256, 320, 512};
    GemmArgs<kMaxGroup> a;
    EXPECT(pack_args(batch_of({s, s, s}), a) && all_zero(make_preload_grouped(a, false)));          // three problems
    EXPECT(pack_args(batch_of({s, s, s, s}), a) && all_zero(make_preload_grouped(a, false)));       // four
    const Shape d[] = {{8, 3, 257, 320, 512}, {8, 3, 256, 321, 512}, {8, 3, 256, 320, 768}, {16, 3, 256, 320, 512}, {8, 6, 256, 320, 512},
                       {4, 6, 256, 320, 512}, {3, 8, 256, 320, 512}};                               // pairs that differ in one field (the last two: same tile COUNT)
    for (const Shape& o : d) {
      EXPECT(pack_args(batch_of({s, o}), a) && all_zero(make_preload_grouped(a, false)));
      EXPECT(pack_args(batch_of({o, s}), a) && all_zero(make_preload_grouped(a, false)));
    }
    EXPECT(pack_args(batch_of({s, s}), a) && (make_preload_grouped(a, false).flags & kPreValid));
    // a pair whose problems both count from 0 (gemm_bwd_seq's accounting) is no grouped pair
    GemmArgs<2> a2;
    EXPECT(pack_args(batch_of({s, s}, false), a2, false) && all_zero(make_preload_grouped(a2, false)));
    // values a field cannot hold.  pack_args refuses most of them itself; the block must not rely on that
    EXPECT(pack_args(batch_of({s}), a));
    GemmArgs<kMaxGroup> t = a;
    t.hot[0].ldp = kMaxLeadingDim + 1; EXPECT(all_zero(make_preload_grouped(t, false)));
    t = a; t.hot[0].ldq = kMaxLeadingDim + 1; EXPECT(all_zero(make_preload_grouped(t, false)));
    t = a; t.hot[0].ldp = -1; EXPECT(all_zero(make_preload_grouped(t, false)));
    t = a; t.hot[0].Kred = -64; EXPECT(all_zero(make_preload_grouped(t, false)));
    t = a; t.head.tiles_p[0] = 1 << kPreTilesQShift; t.head.tiles_q[0] = 1; EXPECT(all_zero(make_preload_grouped(t, false)));
    t = a; t.head.tiles_p[0] = 1; t.head.tiles_q[0] = 1 << (32 - kPreTilesQShift); EXPECT(all_zero(make_preload_grouped(t, false)));
    t = a; t.head.tiles_q[0] = kTileDecodeMaxQ + 1; EXPECT(all_zero(make_preload_grouped(t, false)));
    t = a; t.head.tiles_p[0] = 0; EXPECT(all_zero(make_preload_grouped(t, false)));
    t = a; t.hot[0].tq_magic += 1; EXPECT(all_zero(make_preload_grouped(t, false)));                // a reciprocal that is not tiles_q's
    t = a; t.head.tile_base[0] = 1; EXPECT(all_zero(make_preload_grouped(t, false)));
    EXPECT(pack_args(batch_of({s, s}), a));
    t = a; t.head.tile_base[1] += 1; EXPECT(all_zero(make_preload_grouped(t, false)));              // a split that is not problem 0's tile count
    t = a; t.hot[1].tq_magic += 1; EXPECT(all_zero(make_preload_grouped(t, false)));
    // leading dimensions and tile counts AT the limits are held whole
    const Shape big{kTileDecodeMaxTiles / kTileDecodeMaxQ, kTileDecodeMaxQ, kMaxLeadingDim, kMaxLeadingDim, 1 << 30};
    EXPECT(pack_args(batch_of({big}), a));
    const GemmPreload w = make_preload_grouped(a, false);
    EXPECT((w.flags & kPreValid) && (int)w.ldp == kMaxLeadingDim && (int)w.ldq == kMaxLeadingDim && (int)w.Kred == (1 << 30));
    EXPECT((int)(w.tiles & ((1u << kPreTilesQShift) - 1)) == big.tp && (int)(w.tiles >> kPreTilesQShift) == big.tq);
  }
  // 4. the record form, decoded by preload_record_decode — the function gemm_wgrad_tail and k_dgrad_qtrain call.  gemm_wgrad_tail:
  // the 64 x 64 wgrad record (0), whose tiles come behind `first` = riders + narrow tiles blocks and in front of the tails block;
  // EVERY block of the grid: the blocks in front and behind are not the record's, the others map onto its tiles one to one, as the
  // kernel's GemmArgs path maps them (tile_decode of the record's counts on b - first).
  for (int tpd = 1; tpd <= 20; tpd += 3)
    for (int tqd = 1; tqd <= 12; tqd += 5)
      for (int tpw = 1; tpw <= 18; tpw += 4)
        for (int tqw = 1; tqw <= 9; tqw += 4) {
          const GemmBatch g = batch_of({{tpw, tqw, 192, 512, 96}, {tpd, tqd, 256, 320, 512}});
          GemmArgs<2> a;
          EXPECT(pack_args(g, a));
          for (int riders : {0, 7}) {
            const int first = riders + tpd * tqd, n1 = tpw * tqw;
            const GemmPreload v = make_preload_record(a, 0, false, first);
            EXPECT((v.flags & kPreValid) && v.P0 == a.hot[0].P && v.Q0 == a.hot[0].Q && v.P1 == nullptr && v.Q1 == nullptr);
            EXPECT((int)v.ldp == a.hot[0].ldp && (int)v.ldq == a.hot[0].ldq && (int)v.Kred == a.hot[0].Kred);
            long bad = 0;
            for (int blk = 0; blk < first + n1 + 2; ++blk) {        // (+ the tails block and one beyond)
              const PreRecordTile t = preload_record_decode(v, blk);
              const bool mine = blk >= first && blk < first + n1;
              bad += t.mine != mine;
              if (!mine) continue;
              int rp, rq;
              tile_decode(a.head.tiles_p[0], a.head.tiles_q[0], a.hot[0].tq_magic, blk - first, rp, rq);
              bad += (t.tile_p != rp) | (t.tile_q != rq) | (t.tiles_p != tpw) | (t.tiles_q != tqw);
            }
            EXPECT(bad == 0);
            swept += n1;
          }
          EXPECT(all_zero(make_preload_record(a, 0, true, 5)) && all_zero(make_preload_record(a, 2, false)) && all_zero(make_preload_record(a, 0, false, -1)));
          // k_dgrad_qtrain: its one record from block 0 on
          GemmArgs<1> a1;
          EXPECT(pack_args(batch_of({{tpd, tqd, 256, 320, 512}}), a1));
          const GemmPreload q = make_preload_record(a1, 0, false);
          long bad = 0;
          for (int blk = 0; blk < tpd * tqd + 1; ++blk) {
            const PreRecordTile t = preload_record_decode(q, blk);
            int rp, rq;
            tile_decode(tpd, tqd, a1.hot[0].tq_magic, blk, rp, rq);
            bad += blk < tpd * tqd ? (!t.mine) | (t.tile_p != rp) | (t.tile_q != rq) : (long)t.mine;
          }
          EXPECT(bad == 0 && (q.flags & kPreValid) && q.P0 == a1.hot[0].P && q.Q0 == a1.hot[0].Q);
        }
  {   // a first block the word cannot hold
    GemmArgs<2> a;
    EXPECT(pack_args(batch_of({{4, 2, 192, 512, 96}, {3, 5, 256, 320, 512}}), a));
    EXPECT(make_preload_record(a, 0, false, (int)kPreNoSplit).flags & kPreValid);
    EXPECT(all_zero(make_preload_record(a, 0, false, (int)kPreNoSplit + 1)));
  }
  // 5. k_dqda_head_bwd<false>'s block (DqdaPreload, head_kernels.hip.h): routing and first-load words against the DqdaHeadArgs they
  // were taken from, for tower tops on both sides of the 256-column chunk, with and without dxc; what a field cannot hold, the fp16
  // form and the tuning bit give the all-zero block
  {
    const DqdaPreload zero{};
    auto is_zero = [&](const DqdaPreload& w) { return std::memcmp(&w, &zero, sizeof w) == 0; };
    _Float16 half_panel[4];
    for (int H : {64, 128, 255, 256, 257, 1024, 0xFFFF})
      for (int rows : {16, 64, 256, 16 * 0xFFFF})
        for (int kred : {64, 1024, 0xFFFF})
          for (int with_dxc = 0; with_dxc < 2; ++with_dxc) {
            DqdaHeadArgs a{};
            a.pr.P = arena + 1; a.pr.Q = arena + 2; a.pr.ldp = 128; a.pr.ldq = kred + 8; a.pr.Kred = kred;
            a.W = arena + 3; a.X4 = arena + 4; a.aout16 = arena + 5; a.H = H; a.rows = rows;
            if (with_dxc) a.dxc = arena + 6;
            const int rt = rows / 16;
            const DqdaPreload w = make_dqda_preload(a, rt, false);
            EXPECT(w.route & kPreValid);
            const DqdaFirst f = dqda_preload_decode(w);
            EXPECT(f.H == H && f.row_tiles == rt && f.tiles == rt * (with_dxc ? 1 : (H + 255) / 256));
            EXPECT(f.W == a.W && f.X4 == a.X4 && f.aout16 == a.aout16 && w.P == a.pr.P && w.Q == a.pr.Q);
            EXPECT((int)w.ldp == a.pr.ldp && (int)w.ldq == a.pr.ldq && (int)(w.h_kred >> 16) == kred);
            EXPECT(is_zero(make_dqda_preload(a, rt, true)));                                        // the tuning bit
            DqdaHeadArgs t = a; t.H = 0x10000; EXPECT(is_zero(make_dqda_preload(t, rt, false)));
            t = a; t.H = 0; EXPECT(is_zero(make_dqda_preload(t, rt, false)));
            t = a; t.pr.Kred = 0x10000; EXPECT(is_zero(make_dqda_preload(t, rt, false)));
            t = a; t.pr.Kred = -64; EXPECT(is_zero(make_dqda_preload(t, rt, false)));
            t = a; t.pr.ldp = kMaxLeadingDim + 1; EXPECT(is_zero(make_dqda_preload(t, rt, false)));
            t = a; t.pr.ldq = -1; EXPECT(is_zero(make_dqda_preload(t, rt, false)));
            EXPECT(is_zero(make_dqda_preload(a, 0x10000, false)) && is_zero(make_dqda_preload(a, 0, false)));
            t = a; t.dZ16 = half_panel; EXPECT(is_zero(make_dqda_preload(t, rt, false)));           // the fp16 form keeps its scalar round
            t = a; t.X4 = nullptr; EXPECT(is_zero(make_dqda_preload(t, rt, false)));
          }
  }
  if (fails) { std::printf("%ld checks failed\n", fails); return 1; }
  std::printf("kernarg preload host OK (%ld tiles swept)\n", swept);
  return 0;
}
