// Host-side check of the packed GEMM launch arguments (dqn-hfo_amd/csrc/gemm_direct.hip.h): the tile map a workgroup applies to
// its block index and what pack_args() hands the kernels.  No HIP call is made: runs on a box without a GPU.
#include <cstdio>
#include <cstring>
#include <vector>

#include "gemm_direct.hip.h"

using namespace dqnhip;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

// the map as the kernels documented it before it was made branch-free
static void tile_map_reference(int tiles_p, int tiles_q, int b, int& tile_p, int& tile_q) {
  if ((tiles_p & 7) == 0) { const int xcd = b & 7, j = b >> 3; tile_q = j % tiles_q; tile_p = (j / tiles_q) * 8 + xcd; }
  else { tile_q = b % tiles_q; tile_p = b / tiles_q; }
}

static GemmBatch batch_of(std::vector<std::pair<int, int>> tiles, float* base) {
  GemmBatch b{}; b.n = (int)tiles.size();
  for (int i = 0; i < b.n; ++i) {
    GemmProblem& p = b.prob[i];
    p.Pdim = 32 * tiles[i].first; p.Qdim = 32 * tiles[i].second; p.Kred = 512 + i;
    p.P = base + 100 * i; p.Q = base + 100 * i + 1; p.C = base + 100 * i + 2; p.ldp = 10 + i; p.ldq = 20 + i; p.ldc = 30 + i;
    p.bias = base + 100 * i + 3; p.mask = base + 100 * i + 4; p.ldm = 40 + i; p.db = base + 100 * i + 5; p.partial = base + 100 * i + 6;
    p.relu = i & 1; p.seed_w = base + 100 * i + 7; p.C2 = base + 100 * i + 8; p.dot_w = base + 100 * i + 9; p.dot_out = base + 100 * i + 10;
    p.xcopy_dst = base + 100 * i + 11; p.xcopy_col = 50 + i; p.xcopy_n = 60 + i; p.mode = i % 3;
  }
  tile_batch(b, 32, 32);
  return b;
}

int main() {
  // 1. the tile map: equal to the documented one, and a bijection of [0, tiles_p tiles_q) onto the tiles
  for (int tp = 1; tp <= 48; ++tp)
    for (int tq = 1; tq <= 9; ++tq) {
      std::vector<int> seen(tp * tq, 0);
      for (int b = 0; b < tp * tq; ++b) {
        int p, q, rp, rq;
        tile_of_counts(tp, tq, b, p, q);
        tile_map_reference(tp, tq, b, rp, rq);
        EXPECT(p == rp && q == rq);
        EXPECT(p >= 0 && p < tp && q >= 0 && q < tq);
        if (p >= 0 && p < tp && q >= 0 && q < tq) ++seen[q * tp + p];
      }
      for (int v : seen) EXPECT(v == 1);
    }
  // 2. pack_args: header, hot and cold records of every group size
  float mem[512];
  const std::vector<std::pair<int, int>> shapes = {{8, 1}, {2, 2}, {16, 1}, {4, 2}};
  for (int n = 1; n <= kMaxGroup; ++n) {
    GemmBatch b = batch_of({shapes.begin(), shapes.begin() + n}, mem);
    GemmArgs<kMaxGroup> a;
    EXPECT(pack_args(b, a));
    EXPECT(a.head.n == n && a.head.total_tiles == b.total_tiles);
    int base = 0;
    for (int i = 0; i < kMaxGroup; ++i) {
      if (i >= n) { EXPECT(a.head.tile_base[i] == INT32_MAX); EXPECT(a.hot[i].P == nullptr && a.cold[i].bias == nullptr); continue; }
      const GemmProblem& p = b.prob[i];
      EXPECT(a.head.tile_base[i] == base && a.head.tiles_p[i] == shapes[i].first && a.head.tiles_q[i] == shapes[i].second);
      base += shapes[i].first * shapes[i].second;
      const GemmHot& h = a.hot[i]; const GemmCold& c = a.cold[i];
      EXPECT(h.P == p.P && h.Q == p.Q && h.C == p.C && h.ldp == p.ldp && h.ldq == p.ldq && h.ldc == p.ldc);
      EXPECT(h.Pdim == p.Pdim && h.Qdim == p.Qdim && h.Kred == p.Kred && h.mode == p.mode);
      EXPECT(c.bias == p.bias && c.mask == p.mask && c.ldm == p.ldm && c.db == p.db && c.partial == p.partial && c.relu == p.relu);
      EXPECT(c.seed_w == p.seed_w && c.C2 == p.C2 && c.dot_w == p.dot_w && c.dot_out == p.dot_out);
      EXPECT(c.xcopy_dst == p.xcopy_dst && c.xcopy_col == p.xcopy_col && c.xcopy_n == p.xcopy_n);
    }
    EXPECT(base == b.total_tiles);
  }
  // 3. accounting that does not hold together never reaches a launch
  {
    GemmBatch b = batch_of(shapes, mem);
    GemmArgs<kMaxGroup> a;
    GemmBatch t = b; t.prob[2].tile_base += 1; EXPECT(!pack_args(t, a));          // a gap: the workgroup before it would fall into problem 1 past its tiles
    t = b; t.prob[1].tile_base -= 1; EXPECT(!pack_args(t, a));                      // an overlap
    t = b; t.prob[3].tiles_q = 0; EXPECT(!pack_args(t, a));
    t = b; t.n = 0; EXPECT(!pack_args(t, a));
    t = b; t.n = kMaxGroup + 1; EXPECT(!pack_args(t, a));
    GemmArgs<2> a2;
    EXPECT(!pack_args(b, a2));                                                      // more problems than the kernel carries records for
    t = batch_of({{8, 1}, {2, 2}}, mem);
    EXPECT(pack_args(t, a2) && !pack_args(t, a2, false));                           // gemm_bwd_seq's form: both problems count from 0
    t.prob[1].tile_base = 0;
    EXPECT(pack_args(t, a2, false) && a2.head.tile_base[0] == 0 && a2.head.tile_base[1] == 0);
  }
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("packed args host OK\n");
  return 0;
}
