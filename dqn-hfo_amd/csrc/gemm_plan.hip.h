// gemm_plan.hip.h — the host side of the fp32 GEMM family (gemm_direct.hip.h): the launch forms of the fp32 tower, what each form
// accepts, and which form a launch of the learner takes.  Part of the argument layer (learner_args.hip.h): no kernel, no launcher;
// gemm_form_launch (gemm_direct.hip.h) launches what this header says.  The choosers are pure functions of integers, so that a
// host-only program can enumerate them (tests/cpp/gemm_plan_host.cpp).
#pragma once
#include "gemm_common.hip.h"

namespace dqnhip {

// ---- the forms: one per launcher template instance the learner reaches for the fp32 tower -------------------------------------
// Riders are not forms: the head's dW / db rider, the q-head rider, dgrad_qtrain, dqda_head_bwd and the tails block are arguments
// of the launch that carries them.  (Values: tests/csrc/dqnhip_internal.h mirrors them in plain C for ctypes.)
enum GemmForm {
  GEMM_FORM_FWD_DIRECT_2x2 = 0, GEMM_FORM_FWD_DIRECT_4x2 = 1,
  GEMM_FORM_FWD_LDS_1x1 = 2, GEMM_FORM_FWD_LDS_2x2 = 3, GEMM_FORM_FWD_LDS_4x2 = 4, GEMM_FORM_FWD_LDS_4x2_ONE_IMAGE = 5,
  GEMM_FORM_DGRAD_DIRECT = 6, GEMM_FORM_DGRAD_LDS = 7, GEMM_FORM_DGRAD_NARROW = 8, GEMM_FORM_WGRAD_NARROW = 9,
  GEMM_FORM_BWD_SEQ = 10, GEMM_FORM_BWD_SEQ_LDS = 11,            // prob[0] dgrad, prob[1] wgrad
  GEMM_FORM_BWD_PAIR = 12, GEMM_FORM_BWD_PAIR_LDS = 13,          // prob[0] dgrad, prob[1] wgrad
  GEMM_FORM_WGRAD_TAIL_1 = 14, GEMM_FORM_WGRAD_TAIL_NO = 15,     // prob[0] wgrad on 64x64 tiles, prob[1] on 64x16 tiles
  GEMM_FORM_COUNT = 16
};
enum GemmFormKind { GEMM_KIND_FWD_DIRECT, GEMM_KIND_FWD_LDS, GEMM_KIND_DGRAD, GEMM_KIND_DGRAD_NARROW, GEMM_KIND_WGRAD_NARROW,
                    GEMM_KIND_BWD /* dgrad + wgrad, pair or seq */, GEMM_KIND_TAIL };
// bp x bq: the tile (of prob[0], where the two problems of a form take different ones: the wgrad beside a dgrad is 64 x 64, the narrow
// wgrad of a tail 64 x 16); lds: the reduction operand goes through the LDS transpose
struct GemmFormSpec { GemmFormKind kind; int bp, bq; bool lds; int n_min, n_max; const char* name; };
inline constexpr GemmFormSpec kGemmForms[GEMM_FORM_COUNT] = {
    {GEMM_KIND_FWD_DIRECT, 32, 32, false, 1, kMaxGroup, "fwd_direct<2,2>"},
    {GEMM_KIND_FWD_DIRECT, 64, 32, false, 1, kMaxGroup, "fwd_direct<4,2>"},
    {GEMM_KIND_FWD_LDS, 16, 16, true, 1, kMaxGroup, "fwd_lds<1,1,true>"},
    {GEMM_KIND_FWD_LDS, 32, 32, true, 1, kMaxGroup, "fwd_lds<2,2,true>"},
    {GEMM_KIND_FWD_LDS, 64, 32, true, 1, kMaxGroup, "fwd_lds<4,2,true>"},
    {GEMM_KIND_FWD_LDS, 64, 32, true, 1, kMaxGroup, "fwd_lds<4,2,true,1>"},
    {GEMM_KIND_DGRAD, 64, 16, false, 1, kMaxGroup, "dgrad_direct<1,1>"},
    {GEMM_KIND_DGRAD, 64, 16, true, 1, kMaxGroup, "dgrad_lds<1,1>"},
    {GEMM_KIND_DGRAD_NARROW, 16, 16, false, 1, kMaxGroup, "dgrad_narrow"},
    {GEMM_KIND_WGRAD_NARROW, 64, 16, false, 1, kMaxGroup, "wgrad_narrow<1>"},
    {GEMM_KIND_BWD, 64, 16, false, 2, 2, "bwd_seq<false>"},
    {GEMM_KIND_BWD, 64, 16, true, 2, 2, "bwd_seq<true>"},
    {GEMM_KIND_BWD, 64, 16, false, 2, 2, "bwd_pair_direct<1,false>"},
    {GEMM_KIND_BWD, 64, 16, true, 2, 2, "bwd_pair_direct<1,true>"},
    {GEMM_KIND_TAIL, 64, 64, false, 2, 2, "wgrad_tail<1>"},
    {GEMM_KIND_TAIL, 64, 64, false, 2, 2, "wgrad_tail<kNO>"},
};

// ---- what a form accepts: nothing that fails here may be launched ---------------------------------------------------------------
// The launchers count tiles by integer division and the bodies walk the reduction in fixed steps: a tile that does not divide the
// shape silently drops a strip of the output, a reduction of the wrong length is read past its end.
// K >= 512 and K % 256 == 0: full-line loads + wave-private LDS transpose; else the plain direct body
inline bool gemm_lds_ok(int kred) { return kred >= 512 && kred % 256 == 0; }
inline bool gemm_tiles_ok(const GemmProblem& p, int bp, int bq) {
  if (p.ldp > kMaxLeadingDim || p.ldq > kMaxLeadingDim) return false;      // the lanes' 32-bit operand offsets (gemm_common.hip.h)
  return p.Pdim > 0 && p.Qdim > 0 && p.Kred > 0 && p.Pdim % bp == 0 && p.Qdim % bq == 0;
}
// the reduction: every body splits it over the four waves (Kred / 4 each).  The k-contiguous operands advance in 16-k blocks per
// wave (Kred % 64 == 0); the LDS-transpose bodies in 32-k steps, an even count of at least four (gemm_lds_ok); the wgrad bodies in
// steps of four rows (Kred % 16 == 0)
inline bool gemm_kred_ok(int kred, bool lds) { return lds ? gemm_lds_ok(kred) : (kred >= 64 && kred % 64 == 0); }
inline bool gemm_fwd_extras_absent(const GemmProblem& p) {
  return !p.bias && !p.seed_w && !p.dot_w && !p.C2 && !p.dot_out && !p.xcopy_dst;
}
inline bool gemm_fwd_accepts(const GemmProblem& p, const GemmFormSpec& f) {
  if (p.mode != GEMM_FWD || !gemm_tiles_ok(p, f.bp, f.bq) || !gemm_kred_ok(p.Kred, f.lds)) return false;
  if (p.mask || p.db || p.partial) return false;
  // xcopy: fwd_direct_body only (first_layers_launch), columns inside the operand's pitch; the lds body has no such epilogue
  if (p.xcopy_dst && (f.lds || p.xcopy_n <= 0 || p.xcopy_col < 0 || (long)p.xcopy_col + p.xcopy_n > p.ldp)) return false;
  return !p.seed_w == !p.C2 && !p.dot_w == !p.dot_out;
}
// dgrad: P = W [Kred][Pdim] (rows are the reduction index), Q = dY [Qdim][Kred], mask / C [Qdim][Pdim]; 64 x 16 tiles, narrow: 16 x 16
inline bool gemm_dgrad_accepts(const GemmProblem& p, bool lds, bool narrow) {
  if (p.mode != GEMM_DGRAD || !gemm_tiles_ok(p, narrow ? 16 : 64, 16) || !gemm_kred_ok(p.Kred, lds)) return false;
  return gemm_fwd_extras_absent(p) && !p.db && !p.partial;
}
// wgrad: P = X [Kred][Pdim], Q = dY [Kred][Qdim], C = dW [Qdim][Pdim], db [Qdim], one partial per tile; 64 x 64 tiles, narrow: 64 x 16
inline bool gemm_wgrad_accepts(const GemmProblem& p, bool narrow) {
  if (p.mode != GEMM_WGRAD || !gemm_tiles_ok(p, 64, narrow ? 16 : 64) || p.Kred < 16 || p.Kred % 16) return false;
  return gemm_fwd_extras_absent(p) && !p.mask;
}
inline bool gemm_form_accepts(int form, const GemmBatch& b) {
  if (form < 0 || form >= GEMM_FORM_COUNT) return false;
  const GemmFormSpec& f = kGemmForms[form];
  if (b.n < f.n_min || b.n > f.n_max) return false;
  switch (f.kind) {
    case GEMM_KIND_FWD_DIRECT: case GEMM_KIND_FWD_LDS:
      for (int i = 0; i < b.n; ++i) if (!gemm_fwd_accepts(b.prob[i], f)) return false;
      return true;
    case GEMM_KIND_DGRAD: case GEMM_KIND_DGRAD_NARROW:
      for (int i = 0; i < b.n; ++i) if (!gemm_dgrad_accepts(b.prob[i], f.lds, f.kind == GEMM_KIND_DGRAD_NARROW)) return false;
      return true;
    case GEMM_KIND_WGRAD_NARROW:
      for (int i = 0; i < b.n; ++i) if (!gemm_wgrad_accepts(b.prob[i], true)) return false;
      return true;
    case GEMM_KIND_BWD: return gemm_dgrad_accepts(b.prob[0], f.lds, false) && gemm_wgrad_accepts(b.prob[1], false);
    case GEMM_KIND_TAIL: return gemm_wgrad_accepts(b.prob[0], false) && gemm_wgrad_accepts(b.prob[1], true);
  }
  return false;
}

// ---- the choosers: which form a launch of the learner takes ---------------------------------------------------------------------
// One tower layer forward, n passes of identical shape: kred = the layer's padded input width, pdim = its outputs, rows = the batch.
// One problem: 32x32 tiles (256 workgroups for a 256x1024 layer); grouped: 64x32.  Without the LDS transpose (first layer, narrow
// towers): the plain direct kernel.
inline GemmForm fwd_form(int kred, int pdim, int rows, int n) {
  const bool lds = gemm_lds_ok(kred);
  if (n == 1) {
    // acting-time batches (<= 128 rows, e.g. 64 env workers): 16x16 tiles so that one layer still spreads
    // over 256 workgroups (64 rows x 1024 outputs = 256 tiles) instead of 64
    if (lds && rows <= 128) return GEMM_FORM_FWD_LDS_1x1;
    // enough rows to fill the chip with 64x32 tiles (fewer bytes per FLOP)
    if (lds && rows >= 512 && pdim % 64 == 0) return GEMM_FORM_FWD_LDS_4x2;
    return lds ? GEMM_FORM_FWD_LDS_2x2 : GEMM_FORM_FWD_DIRECT_2x2;
  }
  // grouped launches: 64x32 tiles when they still give the chip something to do; small minibatches / narrow layers
  // (the reference's defaults: 32 rows into 512 outputs = 16 such tiles for two problems, one long chain each) take
  // 32x32 or 16x16 tiles — same K split over the four waves, same reduction order, more workgroups
  const long t42 = (long)n * (pdim / 64) * (rows / 32), t22 = (long)n * (pdim / 32) * (rows / 32);
  if (lds) {
    // one LDS image per wave (48 KiB): both tiles of a CU resident at once — same-box A/B +0.6 %
    if (t42 >= 192) return GEMM_FORM_FWD_LDS_4x2_ONE_IMAGE;
    if (t22 >= 128 || rows > 128 || rows % 16) return GEMM_FORM_FWD_LDS_2x2;
    return GEMM_FORM_FWD_LDS_1x1;
  }
  return t42 >= 64 ? GEMM_FORM_FWD_DIRECT_4x2 : GEMM_FORM_FWD_DIRECT_2x2;
}
// Step(1)'s four first layers in one launch (learner.hip first_layers_launch: three or four problems of two widths, one with the
// xcopy epilogue): the 64x32 direct tile whatever the count — plan_of admits the merged launch for first layers of 64 k outputs only
inline GemmForm first_layers_form() { return GEMM_FORM_FWD_DIRECT_4x2; }

// One tower layer backward: kp_in = the layer's padded input width (the dgrad's and the wgrad's Pdim), out = its outputs (the
// dgrad's reduction, the wgrad's Qdim), rows = the batch.
// small minibatches / narrow layers: when the dgrad's 64x16 tiles and the wgrad's 64x64 tiles together still fit the chip in one
// round, they run side by side on their own workgroups (gemm_bwd_pair_direct: one tile's chain per launch, not two)
inline bool bwd_layer_is_pair(int kp_in, int out, int rows) {
  const long tiles = (long)(kp_in / 64) * (rows / 16) + (long)(kp_in / 64) * (out / 64);
  return tiles <= 256 && rows % 16 == 0 && kp_in % 64 == 0 && out % 64 == 0;
}
// the layer's input gradient alone; narrow: only some 16-column tiles of it are consumed (the critic's action columns)
inline GemmForm dgrad_form(int out, bool narrow = false) {
  return narrow ? GEMM_FORM_DGRAD_NARROW : (gemm_lds_ok(out) ? GEMM_FORM_DGRAD_LDS : GEMM_FORM_DGRAD_DIRECT);
}
// wgrad alone = the first layer (K_in = 64 / 128 columns): 16-output tiles, 4x the workgroups
inline GemmForm wgrad_form() { return GEMM_FORM_WGRAD_NARROW; }
// dgrad + wgrad of one layer in one launch: side by side (pair) or ONE workgroup type, its wgrad tile and then its dgrad tile (seq)
inline GemmForm bwd_form(int kp_in, int out, int rows) {
  if (bwd_layer_is_pair(kp_in, out, rows)) return gemm_lds_ok(out) ? GEMM_FORM_BWD_PAIR_LDS : GEMM_FORM_BWD_PAIR;
  return gemm_lds_ok(out) ? GEMM_FORM_BWD_SEQ_LDS : GEMM_FORM_BWD_SEQ;
}
// The SHIFTED schedule (learner.hip tower_backward): the top layer's dgrad alone (dgrad_form), then per middle layer its dgrad with
// the wgrad of the layer above — never a pair: the schedule is taken only where no layer above the first is one —, then the two
// lowest wgrads with the head's riders (nh = the net's heads)
inline GemmForm bwd_shifted_mid_form(int out) { return gemm_lds_ok(out) ? GEMM_FORM_BWD_SEQ_LDS : GEMM_FORM_BWD_SEQ; }
inline GemmForm bwd_shifted_tail_form(int nh) { return nh == 1 ? GEMM_FORM_WGRAD_TAIL_1 : GEMM_FORM_WGRAD_TAIL_NO; }

}  // namespace dqnhip
