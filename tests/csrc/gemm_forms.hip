// gemm_forms.hip — dqnhip_test_gemm_form: ONE launch of a GEMM form the learner launches, on buffers the caller made
// (tests/csrc/dqnhip_internal.h).  Where gemm_bench.hip fills dense operands on the device and hands back one max-abs number,
// this entry is a thin host-visible door to the product's own launchers: every operand may sit at an offset inside a wider,
// guard-banded buffer with a leading dimension larger than its width, and every in/out buffer comes back whole, so that the
// Python side (tests/gemm_ref.py) can judge each element against a float64 reference and check that nothing outside the
// tiles was touched.  Test infrastructure, not on the hot path.  The kernel-test entries: dqnhip_test_gemm / dqnhip_test_hgemm /
// dqnhip_test_hgemm_backward (gemm_bench.hip: device-side reference, one figure), dqnhip_test_gemm_form (here: the fp32 tower's
// forms) and dqnhip_test_hgemm_form (hgemm_forms.hip, in libdqnhip_test_h.so: the fp16 learner's launches).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "dqnhip_internal.h"
#include "gemm_direct.hip.h"
#include "learner_args.hip.h"   // kNO

using namespace dqnhip;

namespace {

// ---- the form table -----------------------------------------------------------------------------------------------------
// Every launcher template instance learner.hip calls for the fp32 tower (riders aside: wgrad_narrow_rider, dgrad_narrow_qrider,
// dgrad_qtrain and dqda_head_bwd are head kernels with their own tests through the C-ABI), against the line that launches it:
//   form                              launcher                              learner.hip
//   FWD_DIRECT_2x2                    fwd_direct_launch<2, 2>               layer_forward :45, :58
//   FWD_DIRECT_4x2                    fwd_direct_launch<4, 2>               layer_forward :57, first_layers_launch :680 (xcopy_dst)
//   FWD_LDS_1x1                       fwd_lds_launch<1, 1, true>            layer_forward :43, :55
//   FWD_LDS_2x2                       fwd_lds_launch<2, 2, true>            layer_forward :45, :54
//   FWD_LDS_4x2                       fwd_lds_launch<4, 2, true>            layer_forward :44
//   FWD_LDS_4x2_ONE_IMAGE             fwd_lds_launch<4, 2, true, 1>         layer_forward :53
//   DGRAD_DIRECT                      dgrad_direct_launch<1, 1>             tower_backward :127, :180
//   DGRAD_LDS                         dgrad_lds_launch<1, 1>                tower_backward :127, :179
//   DGRAD_NARROW                      dgrad_narrow_launch                   tower_backward :176
//   WGRAD_NARROW                      wgrad_narrow_launch<1>                tower_backward :186
//   BWD_SEQ / BWD_SEQ_LDS             bwd_seq_launch<false> / <true>        tower_backward :132, :159, :160
//   BWD_PAIR / BWD_PAIR_LDS           bwd_pair_direct_launch<1, false/true> tower_backward :158
//   WGRAD_TAIL_1 / WGRAD_TAIL_NO      wgrad_tail_launch<1> / <kNO>          tower_backward :139
// (the seed_w / C2 and dot_w / dot_out epilogues ride on whichever forward form the top layer takes: layer_forward :33-34)
enum Kind { K_FWD_DIRECT, K_FWD_LDS, K_DGRAD, K_DGRAD_NARROW, K_WGRAD_NARROW, K_BWD, K_TAIL };
struct FormSpec { Kind kind; int bp, bq; bool lds; int n_min, n_max; };
const FormSpec kForms[DQNHIP_FORM_COUNT] = {
    {K_FWD_DIRECT, 32, 32, false, 1, kMaxGroup}, {K_FWD_DIRECT, 64, 32, false, 1, kMaxGroup},
    {K_FWD_LDS, 16, 16, true, 1, kMaxGroup},     {K_FWD_LDS, 32, 32, true, 1, kMaxGroup},
    {K_FWD_LDS, 64, 32, true, 1, kMaxGroup},     {K_FWD_LDS, 64, 32, true, 1, kMaxGroup},
    {K_DGRAD, 64, 16, false, 1, kMaxGroup},      {K_DGRAD, 64, 16, true, 1, kMaxGroup},
    {K_DGRAD_NARROW, 16, 16, false, 1, kMaxGroup}, {K_WGRAD_NARROW, 64, 16, false, 1, kMaxGroup},
    {K_BWD, 64, 16, false, 2, 2},                {K_BWD, 64, 16, true, 2, 2},
    {K_BWD, 64, 16, false, 2, 2},                {K_BWD, 64, 16, true, 2, 2},
    {K_TAIL, 64, 64, false, 2, 2},               {K_TAIL, 64, 64, false, 2, 2},
};

// ---- shape validation: nothing that fails here reaches the GPU ---------------------------------------------------------------
constexpr int64_t kMaxDim = 8192, kMaxCount = (int64_t)1 << 26;

bool present(const dqnhip_test_buf& b) { return b.host != nullptr; }
// a [rows][cols] operand of pitch ld at b.offset lies inside b; align: 4 where the kernel moves it as float4 (16-byte loads / stores
// off a 256-byte-aligned allocation), 1 where it moves single dwords
bool fits(const dqnhip_test_buf& b, int64_t rows, int64_t cols, int64_t ld, int align) {
  if (!present(b) || b.count <= 0 || b.count > kMaxCount || b.offset < 0) return false;
  if (rows <= 0 || cols <= 0 || ld < cols) return false;
  if (b.offset % align || (rows > 1 && ld % align)) return false;
  return b.offset + (rows - 1) * ld + cols <= b.count;
}
bool dims_ok(const dqnhip_test_problem& p, int bp, int bq) {
  return p.Pdim > 0 && p.Qdim > 0 && p.Kred > 0 && p.Pdim <= kMaxDim && p.Qdim <= kMaxDim && p.Kred <= kMaxDim && p.Pdim % bp == 0 && p.Qdim % bq == 0;
}
// the reduction: every body splits it over the four waves (Kred / 4 each).  The k-contiguous operands advance in 16-k blocks per
// wave (Kred % 64 == 0); the LDS-transpose bodies in 32-k steps, an even count of at least four (Kred % 256 == 0, Kred >= 512);
// the wgrad bodies in steps of four rows (Kred % 16 == 0)
bool kred_ok(int kred, bool lds) { return lds ? (kred >= 512 && kred % 256 == 0) : (kred >= 64 && kred % 64 == 0); }

bool check_fwd(const dqnhip_test_problem& p, int bp, int bq, bool lds) {
  if (p.mode != GEMM_FWD || !dims_ok(p, bp, bq) || !kred_ok(p.Kred, lds)) return false;
  if (present(p.mask) || present(p.db) || present(p.partial)) return false;
  int64_t pcols = p.Kred;
  if (present(p.xcopy_dst)) {          // fwd_direct_body only (first_layers_launch); the lds body has no such epilogue
    if (lds || p.xcopy_n <= 0 || p.xcopy_col < 0 || (int64_t)p.xcopy_col + p.xcopy_n > p.ldp) return false;
    if (!fits(p.xcopy_dst, p.xcopy_n, p.Pdim, p.Pdim, 1)) return false;
    if ((int64_t)p.xcopy_col + p.xcopy_n > pcols) pcols = (int64_t)p.xcopy_col + p.xcopy_n;
  }
  if (!fits(p.P, p.Pdim, p.Kred, p.ldp, 4) || !fits(p.P, p.Pdim, pcols, p.ldp, 1)) return false;
  if (!fits(p.Q, p.Qdim, p.Kred, p.ldq, 4) || !fits(p.C, p.Qdim, p.Pdim, p.ldc, 4)) return false;
  if (present(p.bias) && !fits(p.bias, 1, p.Pdim, p.Pdim, 4)) return false;
  if (present(p.seed_w) != present(p.C2)) return false;
  if (present(p.seed_w) && (!fits(p.seed_w, 1, p.Pdim, p.Pdim, 4) || !fits(p.C2, p.Qdim, p.Pdim, p.ldc, 4))) return false;   // C2 shares C's pitch
  if (present(p.dot_w) != present(p.dot_out)) return false;
  if (present(p.dot_w) && (!fits(p.dot_w, 1, p.Pdim, p.Pdim, 4) || !fits(p.dot_out, p.Qdim, p.Pdim / 16, p.Pdim / 16, 1))) return false;
  return true;
}
bool fwd_extras_absent(const dqnhip_test_problem& p) {
  return !present(p.bias) && !present(p.seed_w) && !present(p.dot_w) && !present(p.C2) && !present(p.dot_out) && !present(p.xcopy_dst);
}
// dgrad: P = W [Kred][Pdim] (rows are the reduction index), Q = dY [Qdim][Kred], mask / C [Qdim][Pdim]; 64 x 16 tiles, narrow: 16 x 16
// with the weight column read one dword per lane
bool check_dgrad(const dqnhip_test_problem& p, bool lds, bool narrow) {
  if (p.mode != GEMM_DGRAD || !dims_ok(p, narrow ? 16 : 64, 16) || !kred_ok(p.Kred, lds)) return false;
  if (!fwd_extras_absent(p) || present(p.db) || present(p.partial)) return false;
  if (!fits(p.P, p.Kred, p.Pdim, p.ldp, narrow ? 1 : 4) || !fits(p.Q, p.Qdim, p.Kred, p.ldq, 4) || !fits(p.C, p.Qdim, p.Pdim, p.ldc, 4)) return false;
  if (present(p.mask) && !fits(p.mask, p.Qdim, p.Pdim, p.ldm, 4)) return false;
  return true;
}
// wgrad: P = X [Kred][Pdim], Q = dY [Kred][Qdim], C = dW [Qdim][Pdim], db [Qdim], one partial per tile; 64 x 64 tiles, narrow: 64 x 16
// with the dY column read one dword per lane
bool check_wgrad(const dqnhip_test_problem& p, bool narrow) {
  const int bq = narrow ? 16 : 64;
  if (p.mode != GEMM_WGRAD || !dims_ok(p, 64, bq) || p.Kred < 16 || p.Kred % 16) return false;
  if (!fwd_extras_absent(p) || present(p.mask)) return false;
  if (!fits(p.P, p.Kred, p.Pdim, p.ldp, 4) || !fits(p.Q, p.Kred, p.Qdim, p.ldq, narrow ? 1 : 4) || !fits(p.C, p.Qdim, p.Pdim, p.ldc, 4)) return false;
  if (present(p.db) && !fits(p.db, 1, p.Qdim, p.Qdim, narrow ? 1 : 4)) return false;
  const int64_t slots = (int64_t)(p.Qdim / bq) * (p.Pdim / 64);
  if (present(p.partial) && !fits(p.partial, 1, slots, slots, 1)) return false;
  return true;
}
bool validate(int form, int n, const dqnhip_test_problem* probs) {
  if (form < 0 || form >= DQNHIP_FORM_COUNT || probs == nullptr) return false;
  const FormSpec& f = kForms[form];
  if (n < f.n_min || n > f.n_max) return false;
  switch (f.kind) {
    case K_FWD_DIRECT: case K_FWD_LDS:
      for (int i = 0; i < n; ++i) if (!check_fwd(probs[i], f.bp, f.bq, f.lds)) return false;
      return true;
    case K_DGRAD: case K_DGRAD_NARROW:
      for (int i = 0; i < n; ++i) if (!check_dgrad(probs[i], f.lds, f.kind == K_DGRAD_NARROW)) return false;
      return true;
    case K_WGRAD_NARROW:
      for (int i = 0; i < n; ++i) if (!check_wgrad(probs[i], true)) return false;
      return true;
    case K_BWD: return check_dgrad(probs[0], f.lds, false) && check_wgrad(probs[1], false);
    case K_TAIL: return check_wgrad(probs[0], false) && check_wgrad(probs[1], true);
  }
  return false;
}

// ---- device copies -----------------------------------------------------------------------------------------------------------
struct DeviceBufs {
  struct B { float* dev; float* host; size_t bytes; bool out; };
  std::vector<B> v;
  ~DeviceBufs() { for (B& b : v) hipFree(b.dev); }
  // uploads the buffer exactly as given; returns the operand's device address (null: absent, or — with *err set — a HIP error)
  float* up(const dqnhip_test_buf& b, bool out, hipError_t* err) {
    if (!present(b) || *err != hipSuccess) return nullptr;
    float* d = nullptr;
    const size_t bytes = (size_t)b.count * sizeof(float);
    if ((*err = hipMalloc(&d, bytes)) != hipSuccess) return nullptr;
    v.push_back(B{d, b.host, bytes, out});
    if ((*err = hipMemcpy(d, b.host, bytes, hipMemcpyHostToDevice)) != hipSuccess) return nullptr;
    return d + b.offset;
  }
  hipError_t down() {
    for (B& b : v)
      if (b.out) { const hipError_t e = hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost); if (e != hipSuccess) return e; }
    return hipSuccess;
  }
};

#define CKF(e) do { hipError_t e__ = (e); if (e__ != hipSuccess) { fprintf(stderr, "dqnhip_test_gemm_form: %s -> %s\n", #e, hipGetErrorString(e__)); return 2; } } while (0)

hipError_t launch_form(int form, GemmBatch& b, hipStream_t s) {
  const HeadWgradRider no_rider{};     // blocks = 0: no head rider, and no tails block
  switch (form) {
    case DQNHIP_FORM_FWD_DIRECT_2x2: return fwd_direct_launch<2, 2>(b, s);
    case DQNHIP_FORM_FWD_DIRECT_4x2: return fwd_direct_launch<4, 2>(b, s);
    case DQNHIP_FORM_FWD_LDS_1x1: return fwd_lds_launch<1, 1, true>(b, s);
    case DQNHIP_FORM_FWD_LDS_2x2: return fwd_lds_launch<2, 2, true>(b, s);
    case DQNHIP_FORM_FWD_LDS_4x2: return fwd_lds_launch<4, 2, true>(b, s);
    case DQNHIP_FORM_FWD_LDS_4x2_ONE_IMAGE: return fwd_lds_launch<4, 2, true, 1>(b, s);
    case DQNHIP_FORM_DGRAD_DIRECT: return dgrad_direct_launch<1, 1>(b, s);
    case DQNHIP_FORM_DGRAD_LDS: return dgrad_lds_launch<1, 1>(b, s);
    case DQNHIP_FORM_DGRAD_NARROW: return dgrad_narrow_launch(b, s);
    case DQNHIP_FORM_WGRAD_NARROW: return wgrad_narrow_launch<1>(b, s);
    case DQNHIP_FORM_BWD_SEQ: return bwd_seq_launch<false>(b, s);
    case DQNHIP_FORM_BWD_SEQ_LDS: return bwd_seq_launch<true>(b, s);
    case DQNHIP_FORM_BWD_PAIR: return bwd_pair_direct_launch<1, false>(b, s);
    case DQNHIP_FORM_BWD_PAIR_LDS: return bwd_pair_direct_launch<1, true>(b, s);
    case DQNHIP_FORM_WGRAD_TAIL_1: return wgrad_tail_launch<1>(b, no_rider, s);
    case DQNHIP_FORM_WGRAD_TAIL_NO: return wgrad_tail_launch<kNO>(b, no_rider, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace

extern "C" int dqnhip_test_gemm_form(int32_t form, int32_t n_problems, const dqnhip_test_problem* probs) {
  if (!validate(form, n_problems, probs)) return 1;
  CKF(direct_prepare_all());     // the dynamic-LDS limits of THIS unit's copies of the kernels: the list the learner's prepare_kernels sets
  DeviceBufs bufs;
  GemmBatch b{}; b.n = n_problems;
  hipError_t err = hipSuccess;
  for (int i = 0; i < n_problems; ++i) {
    const dqnhip_test_problem& t = probs[i];
    GemmProblem& p = b.prob[i];
    p.mode = t.mode; p.Pdim = t.Pdim; p.Qdim = t.Qdim; p.Kred = t.Kred;
    p.ldp = t.ldp; p.ldq = t.ldq; p.ldc = t.ldc; p.ldm = t.ldm; p.relu = t.relu;
    p.xcopy_col = t.xcopy_col; p.xcopy_n = t.xcopy_n;
    p.P = bufs.up(t.P, false, &err); p.Q = bufs.up(t.Q, false, &err);
    p.bias = bufs.up(t.bias, false, &err); p.mask = bufs.up(t.mask, false, &err);
    p.seed_w = bufs.up(t.seed_w, false, &err); p.dot_w = bufs.up(t.dot_w, false, &err);
    p.C = bufs.up(t.C, true, &err); p.db = bufs.up(t.db, true, &err); p.partial = bufs.up(t.partial, true, &err);
    p.C2 = bufs.up(t.C2, true, &err); p.dot_out = bufs.up(t.dot_out, true, &err); p.xcopy_dst = bufs.up(t.xcopy_dst, true, &err);
  }
  CKF(err);
  hipStream_t s; CKF(hipStreamCreate(&s));
  err = launch_form(form, b, s);
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  hipStreamDestroy(s);
  CKF(err);
  CKF(bufs.down());
  return 0;
}
