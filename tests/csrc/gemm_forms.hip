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

using namespace dqnhip;

namespace {

// The forms, what each accepts and the launch switch are the product's own: gemm_plan.hip.h (GemmForm, kGemmForms,
// gemm_form_accepts) and gemm_form_launch (gemm_direct.hip.h).  dqnhip_internal.h repeats the enum in plain C for ctypes:
#define SAME_FORM(x) static_assert((int)DQNHIP_FORM_##x == (int)GEMM_FORM_##x, "dqnhip_internal.h and gemm_plan.hip.h disagree on " #x)
SAME_FORM(FWD_DIRECT_2x2); SAME_FORM(FWD_DIRECT_4x2); SAME_FORM(FWD_LDS_1x1); SAME_FORM(FWD_LDS_2x2); SAME_FORM(FWD_LDS_4x2);
SAME_FORM(FWD_LDS_4x2_ONE_IMAGE); SAME_FORM(DGRAD_DIRECT); SAME_FORM(DGRAD_LDS); SAME_FORM(DGRAD_NARROW); SAME_FORM(WGRAD_NARROW);
SAME_FORM(BWD_SEQ); SAME_FORM(BWD_SEQ_LDS); SAME_FORM(BWD_PAIR); SAME_FORM(BWD_PAIR_LDS); SAME_FORM(WGRAD_TAIL_1); SAME_FORM(WGRAD_TAIL_NO);
SAME_FORM(COUNT);
#undef SAME_FORM

bool present(const dqnhip_test_buf& b) { return b.host != nullptr; }
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

// the batch as the launcher gets it; dev = null: the host addresses stand in (gemm_form_accepts asks of a pointer only whether
// it is null)
GemmBatch batch_of(int n, const dqnhip_test_problem* probs, DeviceBufs* dev, hipError_t* err) {
  GemmBatch b{}; b.n = n;
  auto at = [&](const dqnhip_test_buf& t, bool out) { return dev ? dev->up(t, out, err) : (present(t) ? t.host + t.offset : nullptr); };
  for (int i = 0; i < n; ++i) {
    const dqnhip_test_problem& t = probs[i];
    GemmProblem& p = b.prob[i];
    p.mode = t.mode; p.Pdim = t.Pdim; p.Qdim = t.Qdim; p.Kred = t.Kred;
    p.ldp = t.ldp; p.ldq = t.ldq; p.ldc = t.ldc; p.ldm = t.ldm; p.relu = t.relu;
    p.xcopy_col = t.xcopy_col; p.xcopy_n = t.xcopy_n;
    p.P = at(t.P, false); p.Q = at(t.Q, false);
    p.bias = at(t.bias, false); p.mask = at(t.mask, false);
    p.seed_w = at(t.seed_w, false); p.dot_w = at(t.dot_w, false);
    p.C = at(t.C, true); p.db = at(t.db, true); p.partial = at(t.partial, true);
    p.C2 = at(t.C2, true); p.dot_out = at(t.dot_out, true); p.xcopy_dst = at(t.xcopy_dst, true);
  }
  return b;
}

// ---- buffer validation: with gemm_form_accepts, nothing that fails here reaches the GPU -------------------------------------------
constexpr int64_t kMaxDim = 8192, kMaxCount = (int64_t)1 << 26;

// a [rows][cols] operand of pitch ld at b.offset lies inside b; align: 4 where the kernel moves it as float4 (16-byte loads / stores
// off a 256-byte-aligned allocation), 1 where it moves single dwords
bool fits(const dqnhip_test_buf& b, int64_t rows, int64_t cols, int64_t ld, int align) {
  if (!present(b) || b.count <= 0 || b.count > kMaxCount || b.offset < 0) return false;
  if (rows <= 0 || cols <= 0 || ld < cols) return false;
  if (b.offset % align || (rows > 1 && ld % align)) return false;
  return b.offset + (rows - 1) * ld + cols <= b.count;
}
bool fits_fwd(const dqnhip_test_problem& p) {
  int64_t pcols = p.Kred;
  if (present(p.xcopy_dst)) {
    if (!fits(p.xcopy_dst, p.xcopy_n, p.Pdim, p.Pdim, 1)) return false;
    if ((int64_t)p.xcopy_col + p.xcopy_n > pcols) pcols = (int64_t)p.xcopy_col + p.xcopy_n;
  }
  if (!fits(p.P, p.Pdim, p.Kred, p.ldp, 4) || !fits(p.P, p.Pdim, pcols, p.ldp, 1)) return false;
  if (!fits(p.Q, p.Qdim, p.Kred, p.ldq, 4) || !fits(p.C, p.Qdim, p.Pdim, p.ldc, 4)) return false;
  if (present(p.bias) && !fits(p.bias, 1, p.Pdim, p.Pdim, 4)) return false;
  if (present(p.seed_w) && (!fits(p.seed_w, 1, p.Pdim, p.Pdim, 4) || !fits(p.C2, p.Qdim, p.Pdim, p.ldc, 4))) return false;   // C2 shares C's pitch
  if (present(p.dot_w) && (!fits(p.dot_w, 1, p.Pdim, p.Pdim, 4) || !fits(p.dot_out, p.Qdim, p.Pdim / 16, p.Pdim / 16, 1))) return false;
  return true;
}
// narrow: the weight column is read one dword per lane
bool fits_dgrad(const dqnhip_test_problem& p, bool narrow) {
  if (!fits(p.P, p.Kred, p.Pdim, p.ldp, narrow ? 1 : 4) || !fits(p.Q, p.Qdim, p.Kred, p.ldq, 4) || !fits(p.C, p.Qdim, p.Pdim, p.ldc, 4)) return false;
  return !present(p.mask) || fits(p.mask, p.Qdim, p.Pdim, p.ldm, 4);
}
// narrow: the dY column is read one dword per lane; one partial per 64 x 64 (narrow: 64 x 16) tile
bool fits_wgrad(const dqnhip_test_problem& p, bool narrow) {
  if (!fits(p.P, p.Kred, p.Pdim, p.ldp, 4) || !fits(p.Q, p.Kred, p.Qdim, p.ldq, narrow ? 1 : 4) || !fits(p.C, p.Qdim, p.Pdim, p.ldc, 4)) return false;
  if (present(p.db) && !fits(p.db, 1, p.Qdim, p.Qdim, narrow ? 1 : 4)) return false;
  const int64_t slots = (int64_t)(p.Qdim / (narrow ? 16 : 64)) * (p.Pdim / 64);
  return !present(p.partial) || fits(p.partial, 1, slots, slots, 1);
}
bool validate(int form, int n, const dqnhip_test_problem* probs) {
  if (form < 0 || form >= GEMM_FORM_COUNT || probs == nullptr || n < 1 || n > kMaxGroup) return false;
  if (!gemm_form_accepts(form, batch_of(n, probs, nullptr, nullptr))) return false;
  const GemmFormKind kind = kGemmForms[form].kind;
  for (int i = 0; i < n; ++i) {
    const dqnhip_test_problem& p = probs[i];
    if (p.Pdim > kMaxDim || p.Qdim > kMaxDim || p.Kred > kMaxDim) return false;
    const bool ok = p.mode == GEMM_FWD ? fits_fwd(p) : p.mode == GEMM_DGRAD ? fits_dgrad(p, kind == GEMM_KIND_DGRAD_NARROW)
                  : fits_wgrad(p, kind == GEMM_KIND_WGRAD_NARROW || (kind == GEMM_KIND_TAIL && i == 1));
    if (!ok) return false;
  }
  return true;
}

}  // namespace

extern "C" int dqnhip_test_gemm_form(int32_t form, int32_t n_problems, const dqnhip_test_problem* probs) {
  if (!validate(form, n_problems, probs)) return 1;
  CKF(direct_prepare_all());     // the dynamic-LDS limits of THIS unit's copies of the kernels: the list the learner's prepare_kernels sets
  DeviceBufs bufs;
  hipError_t err = hipSuccess;
  GemmBatch b = batch_of(n_problems, probs, &bufs, &err);
  CKF(err);
  hipStream_t s; CKF(hipStreamCreate(&s));
  err = gemm_form_launch(form, b, s);
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  hipStreamDestroy(s);
  CKF(err);
  CKF(bufs.down());
  return 0;
}
