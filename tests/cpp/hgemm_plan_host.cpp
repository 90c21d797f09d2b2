// Host-side check of the fp16 GEMM launch planning (dqn-hfo_amd/csrc/hgemm.hip.h): which tile hgemm_plan picks, the block ranges
// it hands a grouped launch, what it and the launchers refuse before any launch, and the two block -> tile maps the kernels apply
// (hg_tile_of_block, hg_tile_2d: __host__ __device__ for this).  No HIP call is made: runs on a box without a GPU — every launcher
// call below is one the launcher turns down before it reaches launch().
#include <cstdio>
#include <vector>

#include "hgemm.hip.h"

using namespace dqnhip;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static HGemm prob(int M, int N, int K, int ta = 0, int tb = 0) {
  HGemm g{}; g.M = M; g.N = N; g.K = K; g.ta = ta; g.tb = tb;
  return g;
}
struct Plan { hipError_t e; int wm, wn; long blocks; HGemmBatch b; };
static Plan plan(std::vector<HGemm> gs, int force) {
  Plan p{}; p.wm = p.wn = -1; p.blocks = -1;
  p.e = hgemm_plan(gs.data(), (int)gs.size(), force, p.b, p.wm, p.wn, p.blocks);
  return p;
}
static bool is(const Plan& p, int wm, int wn, long blocks) { return p.e == hipSuccess && p.wm == wm && p.wn == wn && p.blocks == blocks; }

int main() {
  // 1. force = 0: 128 x 128 tiles from 192 of them, 256 x 128 from 192 of those (k-major problems only), else 64 x 64
  EXPECT(is(plan({prob(128 * 3, 128 * 64, 128)}, 0), 2, 2, 192));                 // 192 big tiles; M % 256 != 0: no huge tile
  EXPECT(is(plan({prob(128 * 191, 128, 128)}, 0), 1, 1, 191 * 4));                // 191: the small tile, four times the blocks
  EXPECT(is(plan({prob(256 * 12, 128 * 16, 64)}, 0), 4, 2, 192));                 // 192 huge tiles
  EXPECT(is(plan({prob(256, 128 * 191, 64)}, 0), 2, 2, 382));                     // 191 huge tiles: 382 big ones
  EXPECT(is(plan({prob(256 * 12, 128 * 16, 64, 0, 1)}, 0), 2, 2, 384));           // a reduction-major operand: never the huge tile
  EXPECT(is(plan({prob(384, 4096, 128), prob(384, 4096, 256)}, 0), 2, 2, 192));   // two problems: the tiles of both count (96 + 96)
  EXPECT(is(plan({prob(384, 3968, 128), prob(384, 4096, 256)}, 0), 1, 1, 4 * 189));
  EXPECT(is(plan({prob(4096, 1024, 1024), prob(4096, 1024, 1024)}, 0), 4, 2, 256));   // the learner's forward pair at 4096 rows
  EXPECT(is(plan({prob(4096, 1024, 1024)}, 0), 2, 2, 256));                       // alone: 128 huge tiles, 256 big ones
  EXPECT(is(plan({prob(192, 128 * 300, 128)}, 0), 1, 1, 3 * 600));                // M % 128 != 0: small whatever the count
  // forced tiles
  EXPECT(is(plan({prob(128, 128, 64)}, 1), 2, 2, 1) && is(plan({prob(64, 64, 128)}, 2), 1, 1, 1) && is(plan({prob(256, 128, 64)}, 3), 4, 2, 1));
  // 2. tile_end: four problems of different shapes
  {
    const Plan p = plan({prob(128, 192, 256), prob(64, 64, 128), prob(128, 128, 640), prob(192, 64, 384)}, 2);
    EXPECT(is(p, 1, 1, 6 + 1 + 4 + 3) && p.b.n == 4);
    EXPECT(p.b.tile_end[0] == 6 && p.b.tile_end[1] == 7 && p.b.tile_end[2] == 11 && p.b.tile_end[3] == 14);
    EXPECT(p.b.g[2].M == 128 && p.b.g[2].K == 640 && p.b.g[3].N == 64);
    const Plan q = plan({prob(256, 384, 128, 1, 1), prob(128, 128, 64, 1, 1), prob(384, 128, 192, 1, 1)}, 1);
    EXPECT(is(q, 2, 2, 6 + 1 + 3) && q.b.tile_end[0] == 6 && q.b.tile_end[1] == 7 && q.b.tile_end[2] == 10);
    const Plan h = plan({prob(512, 256, 128), prob(256, 128, 64)}, 3);
    EXPECT(is(h, 4, 2, 4 + 1) && h.b.tile_end[0] == 4 && h.b.tile_end[1] == 5);
  }
  // 3. refusals
  EXPECT(plan({}, 0).e == hipErrorInvalidValue);
  EXPECT(plan(std::vector<HGemm>(5, prob(64, 64, 128)), 2).e == hipErrorInvalidValue);
  EXPECT(plan({prob(128, 128, 32)}, 1).e == hipErrorInvalidValue);                 // K < 64
  EXPECT(plan({prob(128, 128, 96)}, 1).e == hipErrorInvalidValue);                 // K % 64
  EXPECT(plan({prob(128, 128, 0)}, 1).e == hipErrorInvalidValue);
  EXPECT(plan({prob(192, 128, 64)}, 1).e == hipErrorInvalidValue);                 // M = 192 on the 128-tile
  EXPECT(plan({prob(128, 128, 64), prob(128, 192, 64)}, 1).e == hipErrorInvalidValue);
  EXPECT(plan({prob(64, 64, 64)}, 2).e == hipErrorInvalidValue);                   // K = 64 on the small tile
  EXPECT(plan({prob(64, 64, 192)}, 2).e == hipErrorInvalidValue);
  EXPECT(plan({prob(64, 64, 192)}, 0).e == hipErrorInvalidValue);                  // ... which force 0 falls to as well
  EXPECT(plan({prob(96, 64, 128)}, 2).e == hipErrorInvalidValue && plan({prob(64, 32, 128)}, 2).e == hipErrorInvalidValue);
  EXPECT(plan({prob(128, 128, 64)}, 3).e == hipErrorInvalidValue);                 // M % 256 on the huge tile
  EXPECT(plan({prob(256, 128, 64, 1, 1)}, 3).e == hipErrorInvalidValue);           // a reduction-major problem on the huge tile
  EXPECT(plan({prob(256, 128, 64), prob(256, 128, 64, 0, 1)}, 3).e == hipErrorInvalidValue);
  // the launchers, before any launch: orientations no kernel was built for, the tall probe tile, what hgemm_group_db does not carry
  {
    const LaunchOn on(nullptr);
    const HGemm d = prob(64, 64, 128, 0, 1), w = prob(64, 64, 128, 1, 1), f = prob(64, 64, 128);
    const HGemm ddw[3] = {d, d, w}, wd[2] = {w, d}, fd[2] = {f, d}, five[5] = {w, w, w, w, w};
    EXPECT(hgemm_launch_batch(ddw, 3, on, 2) == hipErrorInvalidValue);             // mixed orientations beyond problem 1
    EXPECT(hgemm_launch_batch(wd, 2, on, 2) == hipErrorInvalidValue);              // (3, 2): no such kernel
    EXPECT(hgemm_launch_batch(fd, 2, on, 2) == hipErrorInvalidValue);
    EXPECT(hgemm_launch_batch(five, 5, on, 2) == hipErrorInvalidValue);
    const HGemm big_pair[2] = {prob(128, 128, 64, 0, 1), prob(128, 128, 64, 1, 1)};
    EXPECT(hgemm_launch_batch(big_pair, 2, on, 1) == hipErrorInvalidValue);        // the dgrad + wgrad pair exists on the small tile only
    const HGemm tall = prob(256, 128, 64);
    EXPECT(hgemm_launch_batch(&tall, 1, on, 4) == hipErrorInvalidValue);           // the four-wave 256 x 128 probe is not in the product's build
    Db16Batch db{};
    EXPECT(hgemm_group_db_launch(&d, 1, false, db, 0, on) == hipErrorInvalidValue);   // a k-major problem
    EXPECT(hgemm_group_db_launch(&f, 1, false, db, 0, on) == hipErrorInvalidValue);
    const HGemm w64 = prob(64, 64, 128, 1, 1);
    EXPECT(hgemm_group_db_launch(&w64, 1, true, db, 0, on) == hipErrorInvalidValue);  // 64 x 64 on the 128-tile
    HeadWsum head{}; head.H = 128; head.blocks = 1; head.nh = 1;
    EXPECT(hgemm_group_db_launch(&w, 1, false, db, 0, on, &head) == hipErrorInvalidValue);   // head.blocks * 64 != H
    head.blocks = 2; head.nh = 4;
    EXPECT(hgemm_group_db_launch(&w, 1, false, db, 0, on, &head) == hipErrorInvalidValue);   // nh = 4
  }
  // 4. hgemm_uses_small_tile: what a stand-alone launch with force 0 would take
  EXPECT(!hgemm_uses_small_tile(prob(128 * 3, 128 * 64, 128)) && hgemm_uses_small_tile(prob(128 * 191, 128, 128)));
  EXPECT(hgemm_uses_small_tile(prob(192, 128 * 300, 128)) && !hgemm_uses_small_tile(prob(4096, 1024, 1024)));
  EXPECT(hgemm_uses_small_tile(prob(1024, 1024, 512, 1, 1)));                       // a 512-row wgrad: 64 big tiles
  // 5. hg_tile_of_block: a bijection of [0, total) for every total up to 600, XCD x (= bid % 8) owning a contiguous run
  for (int total = 1; total <= 600; ++total) {
    std::vector<int> seen(total, 0);
    int prev[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    for (int bid = 0; bid < total; ++bid) {
      const int T = hg_tile_of_block(bid, total);
      EXPECT(T >= 0 && T < total);
      if (T >= 0 && T < total) ++seen[T];
      if (prev[bid & 7] >= 0) EXPECT(T == prev[bid & 7] + 1);
      prev[bid & 7] = T;
    }
    for (int v : seen) EXPECT(v == 1);
  }
  // 6. hg_tile_2d: a bijection on every grid it accepts up to 32 x 64 tiles (an XCD's 8 concurrent blocks: a 2 x 4 block of the grid),
  // false on the others
  int accepted = 0;
  for (int tm_n = 1; tm_n <= 32; ++tm_n)
    for (int tn_n = 1; tn_n <= 64; ++tn_n) {
      const bool want = !(tm_n & 1) && !(tn_n & 3) && (((tm_n >> 1) * (tn_n >> 2)) & 7) == 0;
      std::vector<int> seen(tm_n * tn_n, 0);
      for (int bid = 0; bid < tm_n * tn_n; ++bid) {
        int tm = -1, tn = -1;
        const bool ok = hg_tile_2d(bid, tm_n, tn_n, tm, tn);
        EXPECT(ok == want);
        if (!ok) { EXPECT(tm == -1 && tn == -1); continue; }
        EXPECT(tm >= 0 && tm < tm_n && tn >= 0 && tn < tn_n);
        if (tm >= 0 && tm < tm_n && tn >= 0 && tn < tn_n) ++seen[tm * tn_n + tn];
        // the 8 blocks of one XCD that run together (same bid % 8, consecutive j = bid / 8 within a group of 8) share a 2 x 4 block
        int tm0, tn0;
        hg_tile_2d((bid & 7) + ((bid >> 6) << 6), tm_n, tn_n, tm0, tn0);
        EXPECT((tm >> 1) == (tm0 >> 1) && (tn >> 2) == (tn0 >> 2));
      }
      if (want) { ++accepted; for (int v : seen) EXPECT(v == 1); }
    }
  EXPECT(accepted > 0);
  {
    int tm, tn;
    EXPECT(hg_tile_2d(0, 4, 16, tm, tn) && hg_tile_2d(0, 2, 16, tm, tn) == false);   // the grids tests/test_gpu_hgemm_forms.py runs: 4 x 16 accepted
  }
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("hgemm plan host OK\n");
  return 0;
}
