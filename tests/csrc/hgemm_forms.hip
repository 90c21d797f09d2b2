// hgemm_forms.hip — dqnhip_test_hgemm_form: ONE launch of an fp16 launch form of the learner, on buffers the caller made
// (tests/csrc/dqnhip_internal.h).  The fp16 analogue of gemm_forms.hip: a thin host-visible door to the product's own launchers
// (hgemm.hip.h), every operand at an offset inside a wider, guard-banded buffer with a leading dimension that may exceed its
// width, every in/out buffer back whole, so that tests/hgemm_ref.py can judge each element against a float64 reference and check
// that nothing outside the outputs was touched.  No timing, no device-side reference.
//
// This unit includes hgemm.hip.h as libdqnhip.so does: neither HG_WITH_CT16 nor HG_CLOCKPROBE.  gemm_bench.hip defines both
// (a third epilogue pass, a store-back into the fp32 tile, clock reads in hgemm_body), so the two units must not share a shared
// object — different bodies behind the same hgemm_nt<...> symbols — and this one is libdqnhip_test_h.so by itself.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#if defined(HG_WITH_CT16) || defined(HG_CLOCKPROBE)
#error "hgemm_forms.hip tests the product's build of hgemm.hip.h: no HG_WITH_CT16, no HG_CLOCKPROBE"
#endif
#include "dqnhip_internal.h"
#include "hgemm.hip.h"

using namespace dqnhip;

namespace {

// ---- the form table -----------------------------------------------------------------------------------------------------
// Every fp16 launch of learner.hip (the tails block of hgemm_group_db aside: TailsArgs has its own callers), against the line that
// launches it.  The learner leaves the tile to hgemm_plan (force 0) except for the per-layer pair; the forms force it, so that each
// kernel is reached at shapes a test can afford:
//   form                      launcher                                           kernel                     learner.hip
//   NT_BIG_FWD                hgemm_launch_batch(.., 1)                          hgemm_nt<2,2,0,0>          tower_forward16 :383, _pair :392
//   NT_BIG_DGRAD              hgemm_launch_batch(.., 1)                          hgemm_nt<2,2,2,2>          tower_backward16 :441, :448
//   NT_BIG_WGRAD              hgemm_launch_batch(.., 1)                          hgemm_nt<2,2,3,3>          tower_backward16 :449, :467
//   NT_SMALL_FWD              hgemm_launch_batch(.., 2)                          hgemm_nt<1,1,0,0>          tower_forward16 :383, _pair :392
//   NT_SMALL_DGRAD            hgemm_launch_batch(.., 2)                          hgemm_nt<1,1,2,2>          tower_backward16 :441, :448
//   NT_SMALL_WGRAD            hgemm_launch_batch(.., 2)                          hgemm_nt<1,1,3,3>          tower_backward16 :449, :467
//   NT_SMALL_BWD              hgemm_launch_batch({dgrad, wgrad}, 2, .., 2)       hgemm_nt<1,1,2,3>          tower_backward16 :446
//   NT_HUGE_FWD               hgemm_launch_batch(.., 3)                          hgemm_nt<4,2,0,0>          tower_forward16_pair :392 (two 4096-row problems)
//   GROUP_DB_BIG              hgemm_group_db_launch(.., big = true, ..)          hgemm_group_db<2,2>        tower_backward16 :461
//   GROUP_DB_SMALL            hgemm_group_db_launch(.., big = false, ..)         hgemm_group_db<1,1>        tower_backward16 :464
//   DB16_COLS                 launch(k_db16_cols<0>)                             k_db16_cols<0>             tower_backward16 :468
//   CVT16                     cvt16_add + cvt16_launch                           k_cvt16<0>                 sync_w16 :361-364
enum Orient { O_FWD = 0, O_DGRAD = 2, O_WGRAD = 3 };      // hgemm_mode(): ta | tb << 1
struct FormSpec { int force; int bm, bn, kstep; int mode0, mode1; int n_min, n_max; };
const FormSpec kForms[DQNHIP_HFORM_COUNT] = {
    {1, 128, 128, 64, O_FWD, O_FWD, 1, kHGemmMax},     {1, 128, 128, 64, O_DGRAD, O_DGRAD, 1, kHGemmMax}, {1, 128, 128, 64, O_WGRAD, O_WGRAD, 1, kHGemmMax},
    {2, 64, 64, 128, O_FWD, O_FWD, 1, kHGemmMax},      {2, 64, 64, 128, O_DGRAD, O_DGRAD, 1, kHGemmMax},  {2, 64, 64, 128, O_WGRAD, O_WGRAD, 1, kHGemmMax},
    {2, 64, 64, 128, O_DGRAD, O_WGRAD, 2, 2},
    {3, 256, 128, 64, O_FWD, O_FWD, 1, kHGemmMax},
    {1, 128, 128, 64, O_WGRAD, O_WGRAD, 1, kHGemmMax}, {2, 64, 64, 128, O_WGRAD, O_WGRAD, 1, kHGemmMax},
    {0, 0, 0, 0, 0, 0, 0, 0},                          {0, 0, 0, 0, 0, 0, 0, 0},
};

// ---- validation: nothing that fails here reaches the GPU ----------------------------------------------------------------------
constexpr int64_t kMaxDim = 8192, kMaxCount = (int64_t)1 << 26;
constexpr int kAlign16 = 8, kAlign32 = 4;      // 16-byte vector loads / stores: 8 halves, 4 floats

template <typename B> bool present(const B& b) { return b.host != nullptr; }
// a [rows][cols] operand of pitch ld at b.offset lies inside b, offset and pitch multiples of `align` elements
template <typename B> bool fits(const B& b, int64_t rows, int64_t cols, int64_t ld, int align) {
  if (!present(b) || b.count <= 0 || b.count > kMaxCount || b.offset < 0) return false;
  if (rows <= 0 || cols <= 0 || ld < cols || rows > kMaxDim || cols > kMaxDim || ld > 2 * kMaxDim) return false;
  if (b.offset % align || ld % align) return false;
  return b.offset + (rows - 1) * ld + cols <= b.count;
}

bool check_problem(const dqnhip_test_hproblem& p, const FormSpec& f, int mode) {
  if (p.M <= 0 || p.N <= 0 || p.K < 64 || p.M > kMaxDim || p.N > kMaxDim || p.K > kMaxDim) return false;
  if (p.M % f.bm || p.N % f.bn || p.K % 64 || p.K % f.kstep) return false;
  if ((p.ta != 0 && p.ta != 1) || (p.tb != 0 && p.tb != 1) || (p.ta | (p.tb << 1)) != mode) return false;
  if (!(p.ta ? fits(p.A, p.K, p.M, p.lda, kAlign16) : fits(p.A, p.M, p.K, p.lda, kAlign16))) return false;
  if (!(p.tb ? fits(p.B, p.K, p.N, p.ldb, kAlign16) : fits(p.B, p.N, p.K, p.ldb, kAlign16))) return false;
  if (!present(p.C16) && !present(p.C32)) return false;
  if (present(p.C16) && !fits(p.C16, p.M, p.N, p.ldc16, kAlign16)) return false;
  if (present(p.C32)) {
    if (p.n_valid32 <= 0 || p.n_valid32 > p.N || p.n_valid32 % 8) return false;
    if (!fits(p.C32, p.M, p.n_valid32, p.ldc32, kAlign32)) return false;
  }
  if (present(p.bias) && !fits(p.bias, 1, p.N, p.N, kAlign32)) return false;
  if (p.relu != 0 && p.relu != 1) return false;
  if (present(p.mask) && !fits(p.mask, p.M, p.N, p.ldm, kAlign16)) return false;
  if (present(p.seed_w) != present(p.CS16)) return false;
  if (present(p.seed_w) && (!present(p.C16) || !fits(p.seed_w, 1, p.N, p.N, kAlign32) || !fits(p.CS16, p.M, p.N, p.ldcs16, kAlign16))) return false;
  if (present(p.sumsq_partial)) {
    const int64_t slots = (int64_t)(p.M / f.bm) * (p.N / f.bn);
    if (!present(p.C32) || !fits(p.sumsq_partial, 1, slots, slots, 1)) return false;
  }
  return true;
}
bool check_db(const dqnhip_test_hriders& r) {
  if (r.n_db < 0 || r.n_db > 8) return false;
  int64_t blocks = 0;
  for (int i = 0; i < r.n_db; ++i) {
    const dqnhip_test_hdb& d = r.db[i];
    if (d.n_out <= 0 || d.n_out % 64 || d.rows <= 0) return false;
    if (!fits(d.dy, d.rows, d.n_out, d.ld, kAlign16) || !fits(d.db, 1, d.n_out, d.n_out, 1)) return false;
    blocks += d.n_out / 64;
  }
  if (present(r.db_sumsq) && (r.n_db == 0 || !fits(r.db_sumsq, 1, blocks, blocks, 1))) return false;
  return true;
}
bool check_head(const dqnhip_test_hriders& r) {
  if (r.nh == 0) return true;
  if (r.nh != 1 && r.nh != 10) return false;
  if (r.H <= 0 || r.H % 64 || r.blocks * 64 != r.H || r.rows <= 0) return false;
  // nh = 1: one dword per row; nh = 10: three float4 of a 64-byte row (head_wsum_block's weights())
  if (r.nh == 1 ? !fits(r.dy, r.rows, 1, r.lddy, 1) : !fits(r.dy, r.rows, 12, r.lddy, kAlign32)) return false;
  if (!fits(r.X16, r.rows, r.H, r.H, kAlign16)) return false;
  if (!fits(r.dW, r.nh, r.H, r.H, 1) || !fits(r.hdb, 1, r.nh, r.nh, 1)) return false;
  if (present(r.partial) && !fits(r.partial, 1, r.blocks, r.blocks, 1)) return false;
  return true;
}
bool check_cvt(const dqnhip_test_hriders& r) {
  if (r.n_cvt < 1 || r.n_cvt > 8) return false;
  for (int i = 0; i < r.n_cvt; ++i) {
    const dqnhip_test_hcvt& c = r.cvt[i];
    if (c.ld16 <= 0 || c.ld16 % 64 || c.cols > c.ld16) return false;          // k_cvt16 writes whole 64-column tiles of a [rows][ld16] panel
    if (!fits(c.src, c.rows, c.cols, c.ld_src, 1) || !fits(c.dst, c.rows, c.ld16, c.ld16, 1)) return false;
  }
  return true;
}
bool validate(int form, int n, const dqnhip_test_hproblem* probs, const dqnhip_test_hriders* r) {
  if (form < 0 || form >= DQNHIP_HFORM_COUNT) return false;
  const bool has_db = r && r->n_db != 0, has_head = r && r->nh != 0, has_cvt = r && r->n_cvt != 0;
  if (r && present(r->db_sumsq) && !has_db) return false;
  if (form == DQNHIP_HFORM_DB16_COLS) return n == 0 && has_db && !has_head && !has_cvt && check_db(*r);
  if (form == DQNHIP_HFORM_CVT16) return n == 0 && has_cvt && !has_db && !has_head && check_cvt(*r);
  const FormSpec& f = kForms[form];
  if (probs == nullptr || n < f.n_min || n > f.n_max) return false;
  for (int i = 0; i < n; ++i) if (!check_problem(probs[i], f, i == 0 ? f.mode0 : f.mode1)) return false;
  const bool group = form == DQNHIP_HFORM_GROUP_DB_BIG || form == DQNHIP_HFORM_GROUP_DB_SMALL;
  if (!group) return !has_db && !has_head && !has_cvt;
  return !has_cvt && (!r || (check_db(*r) && check_head(*r)));
}

// ---- device copies -----------------------------------------------------------------------------------------------------------
struct DeviceBufs {
  struct B { void* dev; void* host; size_t bytes; bool out; };
  std::vector<B> v;
  hipError_t err = hipSuccess;
  ~DeviceBufs() { for (B& b : v) hipFree(b.dev); }
  // uploads the buffer exactly as given; returns the operand's device address (null: absent, or a HIP error in err)
  template <typename T, typename Buf> T* up(const Buf& b, bool out) {
    if (!present(b) || err != hipSuccess) return nullptr;
    void* d = nullptr;
    const size_t bytes = (size_t)b.count * sizeof(T);
    if ((err = hipMalloc(&d, bytes)) != hipSuccess) return nullptr;
    v.push_back(B{d, b.host, bytes, out});
    if ((err = hipMemcpy(d, b.host, bytes, hipMemcpyHostToDevice)) != hipSuccess) return nullptr;
    return static_cast<T*>(d) + b.offset;
  }
  hipError_t down() {
    for (B& b : v)
      if (b.out) { const hipError_t e = hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost); if (e != hipSuccess) return e; }
    return hipSuccess;
  }
};
static_assert(sizeof(h16) == sizeof(uint16_t), "fp16 panels travel as bit patterns");

#define CKH(e) do { hipError_t e__ = (e); if (e__ != hipSuccess) { fprintf(stderr, "dqnhip_test_hgemm_form: %s -> %s\n", #e, hipGetErrorString(e__)); return 2; } } while (0)

}  // namespace

extern "C" int dqnhip_test_hgemm_form(int32_t form, int32_t n_problems, const dqnhip_test_hproblem* probs, const dqnhip_test_hriders* riders) {
  if (!validate(form, n_problems, probs, riders)) return 1;
  DeviceBufs bufs;
  HGemm gs[kHGemmMax];
  for (int i = 0; i < n_problems; ++i) {
    const dqnhip_test_hproblem& t = probs[i];
    HGemm& g = gs[i]; g = HGemm{};
    g.M = t.M; g.N = t.N; g.K = t.K; g.lda = t.lda; g.ldb = t.ldb; g.ta = t.ta; g.tb = t.tb;
    g.ldc16 = t.ldc16; g.ldc32 = t.ldc32; g.n_valid32 = t.n_valid32; g.relu = t.relu; g.ldm = t.ldm; g.ldcs16 = t.ldcs16;
    g.scale32 = t.scale32; g.seed_scale = t.seed_scale;
    g.A = bufs.up<h16>(t.A, false); g.B = bufs.up<h16>(t.B, false); g.mask = bufs.up<h16>(t.mask, false);
    g.bias = bufs.up<float>(t.bias, false); g.seed_w = bufs.up<float>(t.seed_w, false);
    g.C16 = bufs.up<h16>(t.C16, true); g.CS16 = bufs.up<h16>(t.CS16, true);
    g.C32 = bufs.up<float>(t.C32, true); g.sumsq_partial = bufs.up<float>(t.sumsq_partial, true);
  }
  Db16Batch db{}; int db_blocks = 0;
  HeadWsum head{};
  Cvt16Batch cvt{};
  if (riders != nullptr) {
    const dqnhip_test_hriders& r = *riders;
    db.scale = r.db_scale;
    for (int i = 0; i < r.n_db; ++i) {
      const dqnhip_test_hdb& d = r.db[i];
      db.d[db.n++] = Db16{bufs.up<h16>(d.dy, false), d.ld, d.n_out, d.rows, bufs.up<float>(d.db, true), db_blocks};
      db_blocks += d.n_out / 64;
    }
    db.sumsq_partial = bufs.up<float>(r.db_sumsq, true);
    if (r.nh != 0) {
      head.dy = bufs.up<float>(r.dy, false); head.lddy = r.lddy; head.X16 = bufs.up<h16>(r.X16, false); head.H = r.H; head.rows = r.rows;
      head.dW = bufs.up<float>(r.dW, true); head.db = bufs.up<float>(r.hdb, true); head.partial = bufs.up<float>(r.partial, true);
      head.nh = r.nh; head.blocks = r.blocks;
    }
    for (int i = 0; i < r.n_cvt; ++i) {
      const dqnhip_test_hcvt& c = r.cvt[i];
      cvt16_add(cvt, bufs.up<float>(c.src, false), c.ld_src, c.rows, c.cols, bufs.up<h16>(c.dst, true), c.ld16, c.scale);
    }
  }
  CKH(bufs.err);
  CKH(hgemm_prepare_all());      // the dynamic-LDS limits of THIS unit's copies of the kernels: what the learner's prepare_kernels sets
  hipStream_t s; CKH(hipStreamCreate(&s));
  const LaunchOn on(s);
  hipError_t err;
  switch (form) {
    case DQNHIP_HFORM_GROUP_DB_BIG: case DQNHIP_HFORM_GROUP_DB_SMALL:
      err = hgemm_group_db_launch(gs, n_problems, form == DQNHIP_HFORM_GROUP_DB_BIG, db, db_blocks, on, head.nh != 0 ? &head : nullptr, nullptr);
      break;
    case DQNHIP_HFORM_DB16_COLS: err = launch(on, k_db16_cols<0>, dim3((unsigned)db_blocks), dim3(256), 0, db); break;
    case DQNHIP_HFORM_CVT16: err = cvt16_launch(cvt, on); break;
    default: err = hgemm_launch_batch(gs, n_problems, on, kForms[form].force); break;
  }
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  hipStreamDestroy(s);
  CKH(err);
  CKH(bufs.down());
  return 0;
}
