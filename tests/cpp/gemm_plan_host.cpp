// Host-side check of the fp32 GEMM launch planning (dqn-hfo_amd/csrc/gemm_plan.hip.h): every form a chooser can return accepts the
// shape it was chosen for (exhaustively, over everything the learner's config validation admits and the padded acting batches),
// the choices at the shapes the learner is measured at, and what gemm_form_accepts turns down.  No HIP call is made: runs on a box
// without a GPU.
#include <cstdio>

#include "gemm_plan.hip.h"

using namespace dqnhip;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

// problems as learner.hip builds them (layer_forward; dgrad_of / wgrad_of of tower_backward); the pointers only say "present"
static float dummy[1];
static GemmProblem fwd(int kred, int pdim, int rows) {
  GemmProblem p{}; p.mode = GEMM_FWD; p.P = p.Q = p.bias = dummy; p.C = dummy; p.Pdim = pdim; p.Qdim = rows; p.Kred = kred; p.ldp = p.ldq = kred; p.ldc = pdim;
  return p;
}
static GemmProblem dgrad(int kp_in, int out, int rows) {
  GemmProblem p{}; p.mode = GEMM_DGRAD; p.P = p.Q = p.mask = dummy; p.C = dummy; p.Pdim = kp_in; p.Qdim = rows; p.Kred = out;
  return p;
}
static GemmProblem wgrad(int kp_in, int out, int rows) {
  GemmProblem p{}; p.mode = GEMM_WGRAD; p.P = p.Q = dummy; p.C = p.db = p.partial = dummy; p.Pdim = kp_in; p.Qdim = out; p.Kred = rows;
  return p;
}
static GemmBatch batch(GemmProblem a) { GemmBatch b{}; b.n = 1; b.prob[0] = a; return b; }
static GemmBatch batch(GemmProblem a, GemmProblem c) { GemmBatch b{}; b.n = 2; b.prob[0] = a; b.prob[1] = c; return b; }
static GemmBatch fwd_batch(int kred, int pdim, int rows, int n) {
  GemmBatch b{}; b.n = n;
  for (int i = 0; i < n; ++i) b.prob[i] = fwd(kred, pdim, rows);
  return b;
}
static void report(const char* what, int form, int a, int b, int c, int n) {
  if (++fails <= 20) std::printf("FAILED %s (%d, %d, %d, %d): %s does not accept it\n", what, a, b, c, n, kGemmForms[form].name);
}

int main() {
  // (a) exhaustive: widths in multiples of 64 up to 2048, rows in multiples of 32 up to 4096 (minibatches, and acting batches padded
  // to 32), 1..4 passes — the chosen form accepts the launch, for every launch of a forward and of either backward schedule
  long n_fwd = 0, n_bwd = 0;
  for (int kred = 64; kred <= 2048; kred += 64)
    for (int pdim = 64; pdim <= 2048; pdim += 64)
      for (int rows = 32; rows <= 4096; rows += 32)
        for (int n = 1; n <= 4; ++n, ++n_fwd) {
          const GemmForm f = fwd_form(kred, pdim, rows, n);
          if (!gemm_form_accepts(f, fwd_batch(kred, pdim, rows, n))) report("fwd_form", f, kred, pdim, rows, n);
        }
  for (int kp_in = 64; kp_in <= 2048; kp_in += 64)
    for (int out = 64; out <= 2048; out += 64)
      for (int rows = 32; rows <= 4096; rows += 32, ++n_bwd) {
        auto check = [&](const char* what, GemmForm f, const GemmBatch& b) { if (!gemm_form_accepts(f, b)) report(what, f, kp_in, out, rows, b.n); };
        const GemmProblem d = dgrad(kp_in, out, rows), w = wgrad(kp_in, out, rows);
        // unshifted: the layer's dgrad + wgrad, its dgrad alone, a 16-column slice of it, the first layer's wgrad alone
        check("bwd_form", bwd_form(kp_in, out, rows), batch(d, w));
        check("dgrad_form", dgrad_form(out), batch(d));
        GemmProblem slice = d; slice.Pdim = 16; slice.mask = nullptr;
        check("dgrad_form narrow", dgrad_form(out, true), batch(slice));
        check("wgrad_form", wgrad_form(), batch(w));
        // shifted: the top dgrad is dgrad_form above; a middle launch carries the wgrad of the layer above (kp_in' = out), the tail two wgrads
        check("bwd_shifted_mid_form", bwd_shifted_mid_form(out), batch(d, wgrad(out, kp_in, rows)));
        check("bwd_shifted_tail_form 1", bwd_shifted_tail_form(1), batch(wgrad(out, kp_in, rows), w));
        check("bwd_shifted_tail_form 10", bwd_shifted_tail_form(10), batch(wgrad(out, kp_in, rows), w));
      }
  EXPECT(n_fwd == 524288 && n_bwd == 131072);
  // Step(1)'s merged first layers: four problems of two widths, one with the xcopy epilogue (S = 58 state columns + 10 actions)
  {
    GemmBatch b = fwd_batch(64, 1024, 256, 4);
    b.prob[1] = b.prob[2] = fwd(128, 1024, 256);
    b.prob[2].Kred = 64; b.prob[2].bias = nullptr; b.prob[2].xcopy_dst = dummy; b.prob[2].xcopy_col = 58; b.prob[2].xcopy_n = 10;
    EXPECT(gemm_form_accepts(first_layers_form(), b));
    b.prob[2].xcopy_col = 120;                                   // columns past the operand's pitch
    EXPECT(!gemm_form_accepts(first_layers_form(), b));
  }

  // (b) the choices at the learner's measured shapes
  EXPECT(fwd_form(1024, 1024, 256, 2) == GEMM_FORM_FWD_LDS_4x2_ONE_IMAGE);
  EXPECT(fwd_form(1024, 1024, 256, 1) == GEMM_FORM_FWD_LDS_2x2);
  EXPECT(fwd_form(1024, 1024, 64, 1) == GEMM_FORM_FWD_LDS_1x1);
  EXPECT(fwd_form(1024, 1024, 1024, 1) == GEMM_FORM_FWD_LDS_4x2);
  EXPECT(fwd_form(1024, 1024, 64, 2) == GEMM_FORM_FWD_LDS_2x2);
  EXPECT(fwd_form(1024, 1024, 32, 2) == GEMM_FORM_FWD_LDS_1x1);
  EXPECT(fwd_form(512, 512, 32, 2) == GEMM_FORM_FWD_LDS_1x1);
  EXPECT(fwd_form(64, 1024, 256, 1) == GEMM_FORM_FWD_DIRECT_2x2);
  EXPECT(fwd_form(128, 1024, 256, 2) == GEMM_FORM_FWD_DIRECT_4x2);
  EXPECT(fwd_form(128, 128, 32, 2) == GEMM_FORM_FWD_DIRECT_2x2);
  EXPECT(bwd_form(1024, 1024, 256) == GEMM_FORM_BWD_SEQ_LDS);
  EXPECT(bwd_form(1024, 1024, 64) == GEMM_FORM_BWD_SEQ_LDS);
  EXPECT(bwd_form(512, 512, 32) == GEMM_FORM_BWD_PAIR_LDS);
  EXPECT(bwd_form(128, 128, 32) == GEMM_FORM_BWD_PAIR);
  EXPECT(bwd_layer_is_pair(512, 512, 32) && !bwd_layer_is_pair(1024, 1024, 64));
  EXPECT(dgrad_form(1024) == GEMM_FORM_DGRAD_LDS && dgrad_form(448) == GEMM_FORM_DGRAD_DIRECT && dgrad_form(1024, true) == GEMM_FORM_DGRAD_NARROW);
  EXPECT(bwd_shifted_mid_form(1024) == GEMM_FORM_BWD_SEQ_LDS && bwd_shifted_mid_form(448) == GEMM_FORM_BWD_SEQ);
  EXPECT(bwd_shifted_tail_form(1) == GEMM_FORM_WGRAD_TAIL_1 && bwd_shifted_tail_form(10) == GEMM_FORM_WGRAD_TAIL_NO);

  // (c) what gemm_form_accepts turns down
  EXPECT(gemm_form_accepts(GEMM_FORM_FWD_LDS_2x2, batch(fwd(512, 64, 32))));
  EXPECT(!gemm_form_accepts(GEMM_FORM_FWD_LDS_2x2, batch(fwd(256, 64, 32))));               // an LDS form with Kred = 256
  EXPECT(!gemm_form_accepts(GEMM_FORM_FWD_LDS_1x1, batch(fwd(256, 64, 32))));
  EXPECT(!gemm_form_accepts(GEMM_FORM_DGRAD_LDS, batch(dgrad(64, 256, 32))));
  EXPECT(!gemm_form_accepts(GEMM_FORM_BWD_SEQ_LDS, batch(dgrad(64, 256, 64), wgrad(64, 256, 64))));
  EXPECT(!gemm_form_accepts(GEMM_FORM_FWD_LDS_2x2, batch(fwd(768 + 128, 64, 32))));         // ... or Kred % 256
  EXPECT(gemm_form_accepts(GEMM_FORM_FWD_LDS_4x2, batch(fwd(512, 64, 64))));
  EXPECT(!gemm_form_accepts(GEMM_FORM_FWD_LDS_4x2, batch(fwd(512, 64, 48))));               // Qdim = 48 on the 64x32 tile
  EXPECT(!gemm_form_accepts(GEMM_FORM_FWD_LDS_4x2, batch(fwd(512, 96, 64))));               // Pdim = 96
  EXPECT(gemm_form_accepts(GEMM_FORM_WGRAD_NARROW, batch(wgrad(64, 64, 16))));
  EXPECT(!gemm_form_accepts(GEMM_FORM_WGRAD_NARROW, batch(wgrad(64, 64, 8))));              // a wgrad with Kred = 8
  EXPECT(!gemm_form_accepts(GEMM_FORM_BWD_SEQ, batch(dgrad(64, 64, 64), wgrad(64, 64, 8))));
  EXPECT(!gemm_form_accepts(GEMM_FORM_WGRAD_TAIL_1, batch(wgrad(64, 64, 24), wgrad(64, 64, 24))));
  EXPECT(gemm_form_accepts(GEMM_FORM_BWD_SEQ, batch(dgrad(64, 64, 64), wgrad(64, 64, 64))));
  EXPECT(!gemm_form_accepts(GEMM_FORM_BWD_SEQ, batch(dgrad(64, 64, 64))));                  // BWD_SEQ with n = 1
  EXPECT(!gemm_form_accepts(GEMM_FORM_BWD_SEQ, batch(wgrad(64, 64, 64), dgrad(64, 64, 64))));   // the two problems the wrong way round
  EXPECT(!gemm_form_accepts(GEMM_FORM_DGRAD_DIRECT, fwd_batch(64, 64, 64, 1)));             // a problem of another mode
  {
    GemmBatch x = batch(fwd(512, 64, 32));
    x.prob[0].xcopy_dst = dummy; x.prob[0].xcopy_col = 0; x.prob[0].xcopy_n = 10;
    EXPECT(!gemm_form_accepts(GEMM_FORM_FWD_LDS_2x2, x));                                   // an LDS forward form with xcopy_dst
    x.prob[0].Kred = x.prob[0].ldp = 64;
    EXPECT(gemm_form_accepts(GEMM_FORM_FWD_DIRECT_2x2, x));
    GemmBatch s = batch(fwd(512, 64, 32)); s.prob[0].seed_w = dummy;                        // seed_w without C2, dot_out without dot_w
    EXPECT(!gemm_form_accepts(GEMM_FORM_FWD_LDS_2x2, s));
    s.prob[0].C2 = dummy; EXPECT(gemm_form_accepts(GEMM_FORM_FWD_LDS_2x2, s));
    s.prob[0].dot_out = dummy; EXPECT(!gemm_form_accepts(GEMM_FORM_FWD_LDS_2x2, s));
    GemmBatch m = batch(fwd(512, 64, 32)); m.prob[0].mask = dummy;                          // fields of another mode
    EXPECT(!gemm_form_accepts(GEMM_FORM_FWD_LDS_2x2, m));
    GemmBatch d = batch(dgrad(64, 64, 64)); d.prob[0].db = dummy;
    EXPECT(!gemm_form_accepts(GEMM_FORM_DGRAD_DIRECT, d));
    GemmBatch w = batch(wgrad(64, 64, 64)); w.prob[0].bias = dummy;
    EXPECT(!gemm_form_accepts(GEMM_FORM_WGRAD_NARROW, w));
  }
  EXPECT(!gemm_form_accepts(-1, batch(fwd(64, 64, 32))) && !gemm_form_accepts(GEMM_FORM_COUNT, batch(fwd(64, 64, 32))));
  EXPECT(!gemm_form_accepts(GEMM_FORM_FWD_DIRECT_2x2, fwd_batch(64, 64, 32, 0)));
  { GemmBatch five = fwd_batch(64, 64, 32, 4); five.n = 5; EXPECT(!gemm_form_accepts(GEMM_FORM_FWD_DIRECT_2x2, five)); }

  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("gemm plan host OK: %ld forward and %ld backward shapes\n", n_fwd, n_bwd);
  return 0;
}
