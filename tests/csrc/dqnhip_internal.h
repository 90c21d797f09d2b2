/*
 * dqnhip_internal.h — test / tuning hooks exported by libdqnhip_test.so (csrc/gemm_bench.hip: the timing harness and the
 * probes; csrc/gemm_forms.hip: dqnhip_test_gemm_form, one launch of a product fp32 GEMM form on caller-made buffers) and by
 * libdqnhip_test_h.so (csrc/hgemm_forms.hip: dqnhip_test_hgemm_form, one launch of an fp16 launch form — hgemm_nt on each tile,
 * hgemm_group_db with its riders, k_db16_cols, k_cvt16 — with hgemm.hip.h compiled as the product compiles it).  Not part of
 * the drop-in boundary (include/dqnhip.h); used by tests/ and scripts/gemm_tune.py only.
 */
#ifndef DQNHIP_INTERNAL_H_
#define DQNHIP_INTERNAL_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Run one GEMM kernel variant of the tower layers on random data (uniform [-1,1)),
 * check it against a naive one-thread-per-output device reference and time it.
 *   mode    0 FWD   Y[rows,n_out]  = lrelu(X[rows,k_in] W[n_out,k_in]^T + b)
 *           1 DGRAD dX[rows,k_in]  = (dY[rows,n_out] W[n_out,k_in]) * lrelu'(A[rows,k_in])
 *           2 WGRAD dW[n_out,k_in] = dY^T X ; db = colsum(dY)
 *   variant kernel family / tile (see gemm_bench.hip for the table)
 *   groups  number of independent problems carried by one launch (1..4)
 *   iters   timed back-to-back launches on one stream (after 3 warm-up launches)
 * Returns 0 on success; avg_us = mean time per launch, max_abs_err vs the reference (+inf when a difference is not finite:
 * outputs are prefilled with NaN, so an element the kernel never wrote — or wrote as NaN — cannot pass as "no error"),
 * max_ref = max |reference| (for scaling the error). */
int dqnhip_test_gemm(int32_t mode, int32_t variant, int32_t rows, int32_t n_out, int32_t k_in,
                     int32_t groups, int32_t iters, float* avg_us, float* max_abs_err, float* max_ref);

/* ---- dqnhip_test_gemm_form (csrc/gemm_forms.hip): the GEMM forms learner.hip launches, one launch, host-visible results ----
 * The caller (tests/test_gpu_gemm_forms.py with tests/gemm_ref.py) makes every buffer, guard rows and pad columns included,
 * and judges every element in float64; the entry only uploads, launches ONCE through the product's own *_launch helper
 * (gemm_direct.hip.h) on one stream, synchronises and downloads.  No timing, no iterations, no device-side reference. */
typedef struct dqnhip_test_buf {
  float* host;       /* the whole buffer as uploaded (in/out buffers: and downloaded again, whole); null: operand absent */
  int64_t count;     /* floats in it */
  int64_t offset;    /* float index of the operand's element [0][0] inside it (guard rows in front, an offset panel column) */
} dqnhip_test_buf;
/* One GemmProblem (gemm_common.hip.h: C[q][p] = sum_k Pop(p,k) Qop(q,k), p contiguous).  mode 0 FWD / 1 DGRAD / 2 WGRAD. */
typedef struct dqnhip_test_problem {
  int32_t mode, Pdim, Qdim, Kred, ldp, ldq, ldc, ldm;
  int32_t relu;                                         /* FWD: leaky ReLU in the epilogue */
  int32_t xcopy_col, xcopy_n;                           /* FWD (direct forms): xcopy_dst[j][p] = P[p][xcopy_col + j], j < xcopy_n */
  int32_t reserved;
  dqnhip_test_buf P, Q, bias, mask, seed_w, dot_w;      /* inputs */
  dqnhip_test_buf C, db, partial, C2, dot_out, xcopy_dst; /* in/out: arrive prefilled with the caller's sentinel */
} dqnhip_test_problem;
/* form: one id per launcher template instance learner.hip reaches for the fp32 tower (riders aside): the values of GemmForm
 * (dqn-hfo_amd/csrc/gemm_plan.hip.h, which holds the table and the preconditions; gemm_forms.hip static_asserts the two enums agree) */
enum dqnhip_test_form {
  DQNHIP_FORM_FWD_DIRECT_2x2 = 0, DQNHIP_FORM_FWD_DIRECT_4x2 = 1,
  DQNHIP_FORM_FWD_LDS_1x1 = 2, DQNHIP_FORM_FWD_LDS_2x2 = 3, DQNHIP_FORM_FWD_LDS_4x2 = 4, DQNHIP_FORM_FWD_LDS_4x2_ONE_IMAGE = 5,
  DQNHIP_FORM_DGRAD_DIRECT = 6, DQNHIP_FORM_DGRAD_LDS = 7, DQNHIP_FORM_DGRAD_NARROW = 8, DQNHIP_FORM_WGRAD_NARROW = 9,
  DQNHIP_FORM_BWD_SEQ = 10, DQNHIP_FORM_BWD_SEQ_LDS = 11,            /* probs[0] dgrad, probs[1] wgrad */
  DQNHIP_FORM_BWD_PAIR = 12, DQNHIP_FORM_BWD_PAIR_LDS = 13,          /* probs[0] dgrad, probs[1] wgrad */
  DQNHIP_FORM_WGRAD_TAIL_1 = 14, DQNHIP_FORM_WGRAD_TAIL_NO = 15,     /* probs[0] wgrad on 64x64 tiles, probs[1] on 64x16 tiles; no riders */
  DQNHIP_FORM_COUNT = 16
};
/* Returns 0 on success.
 * Returns 1, before anything is uploaded or launched, when the form id, the problem count, a shape, a leading dimension or an
 * alignment does not satisfy what the launcher and the kernel body assume, or when an operand does not lie wholly inside the
 * buffer it was given in: after a return of 0 or 2 every address the kernel formed was inside the caller's buffers.
 * Returns 2 on a HIP error.
 * Not thread-safe (the one-time dynamic-LDS opt-in is a plain static flag): call it from one thread, as pytest does. */
int dqnhip_test_gemm_form(int32_t form, int32_t n_problems, const dqnhip_test_problem* probs);

/* fp16-input / fp32-accumulate GEMM family (csrc/hgemm.hip.h) on random data against a naive device
 * reference.  C[m][n] = sum_k A[m][k] B[n][k], A [M][K], B [N][K] fp16.
 *   mode 0 FWD-like   bias + leaky ReLU; fp16 [M][N], transposed fp16 [N][M] and fp32 outputs
 *        1 DGRAD-like ReLU' mask; the same three outputs, fp32 one scaled
 *        2 WGRAD-like scaled fp32 output, only the first N/2 columns written
 *        4 / 5   as 0 with the fp16 output only / fp16 + transposed fp16 (the common layer cases)
 *        3 glue check: k_cvt16 (fp32 -> fp16 + transposed, zero padding) and k_db16 on an M x N panel
 *   tile 0 auto, 1 128x128, 2 64x64 with in-workgroup split-K, 3 256x128 on eight waves; +10: two problems (the second a
 *        copy with its own outputs, which must come out bit-identical) in one launch
 * max_abs_err excludes one fp16 rounding of each fp16 result. */
int dqnhip_test_hgemm(int32_t mode, int32_t tile, int32_t M, int32_t N, int32_t K, int32_t iters,
                      float* avg_us, float* max_abs_err, float* max_ref);

/* ---- dqnhip_test_hgemm_form (csrc/hgemm_forms.hip, libdqnhip_test_h.so): the fp16 launches of the learner, one launch ----
 * The fp16 analogue of dqnhip_test_gemm_form, in a library of its own: hgemm_forms.hip compiles hgemm.hip.h exactly as
 * libdqnhip.so does (neither HG_WITH_CT16 nor HG_CLOCKPROBE), gemm_bench.hip compiles it with both, and the two bodies behind
 * the same hgemm_nt<...> symbols must not meet in one shared object.  The caller (tests/test_gpu_hgemm_forms.py with
 * tests/hgemm_ref.py) makes every buffer, guards and pads included; the entry validates, uploads every buffer whole, calls
 * hgemm_prepare_all(), launches ONCE through the product's launcher, synchronises and downloads every output buffer whole. */
typedef struct dqnhip_test_buf16 {
  uint16_t* host;    /* fp16 bit patterns; null: operand absent */
  int64_t count;     /* halves in it */
  int64_t offset;    /* half index of the operand's element [0][0] */
} dqnhip_test_buf16;
/* One HGemm (hgemm.hip.h): C[m][n] = sum_k Aop(m,k) Bop(n,k); ta / tb = 1: the operand is stored [K][M] resp. [K][N]. */
typedef struct dqnhip_test_hproblem {
  int32_t M, N, K, lda, ldb, ta, tb, ldc16, ldc32, n_valid32, relu, ldm, ldcs16, reserved;
  float scale32, seed_scale;
  dqnhip_test_buf16 A, B, mask;                 /* inputs */
  dqnhip_test_buf bias, seed_w;                 /* inputs */
  dqnhip_test_buf16 C16, CS16;                  /* in/out: arrive prefilled with the caller's sentinel */
  dqnhip_test_buf C32, sumsq_partial;           /* in/out (sumsq_partial: one slot per tile of the problem) */
} dqnhip_test_hproblem;
typedef struct dqnhip_test_hdb {                /* one Db16: db[n] = scale * sum_b dy[b][n] */
  dqnhip_test_buf16 dy; int32_t ld, n_out, rows, reserved; dqnhip_test_buf db;
} dqnhip_test_hdb;
typedef struct dqnhip_test_hcvt {               /* one Cvt16 without a transposed output, as the learner calls cvt16_add */
  dqnhip_test_buf src; int32_t ld_src, rows, cols, ld16; float scale; int32_t reserved; dqnhip_test_buf16 dst;
} dqnhip_test_hcvt;
typedef struct dqnhip_test_hriders {
  int32_t n_db; float db_scale; dqnhip_test_hdb db[8]; dqnhip_test_buf db_sumsq;     /* Db16Batch (db_sumsq: one slot per 64-column block) */
  int32_t nh, lddy, H, rows, blocks, reserved;                                       /* HeadWsum; nh 0: none */
  dqnhip_test_buf dy; dqnhip_test_buf16 X16; dqnhip_test_buf dW, hdb, partial;
  int32_t n_cvt, reserved2; dqnhip_test_hcvt cvt[8];                                 /* Cvt16Batch */
} dqnhip_test_hriders;
enum dqnhip_test_hform {
  DQNHIP_HFORM_NT_BIG_FWD = 0, DQNHIP_HFORM_NT_BIG_DGRAD = 1, DQNHIP_HFORM_NT_BIG_WGRAD = 2,        /* hgemm_launch_batch(.., 1) */
  DQNHIP_HFORM_NT_SMALL_FWD = 3, DQNHIP_HFORM_NT_SMALL_DGRAD = 4, DQNHIP_HFORM_NT_SMALL_WGRAD = 5,  /* hgemm_launch_batch(.., 2) */
  DQNHIP_HFORM_NT_SMALL_BWD = 6,                                     /* probs[0] dgrad, probs[1] wgrad, force 2 */
  DQNHIP_HFORM_NT_HUGE_FWD = 7,                                      /* hgemm_launch_batch(.., 3) */
  DQNHIP_HFORM_GROUP_DB_BIG = 8, DQNHIP_HFORM_GROUP_DB_SMALL = 9,    /* hgemm_group_db_launch: 1..4 wgrads + Db16Batch + HeadWsum */
  DQNHIP_HFORM_DB16_COLS = 10,                                       /* k_db16_cols<0>: riders->db only, no problems */
  DQNHIP_HFORM_CVT16 = 11,                                           /* cvt16_add + cvt16_launch: riders->cvt only, no problems */
  DQNHIP_HFORM_COUNT = 12
};
/* Returns 0 on success; 1, before anything is uploaded or launched, on an invalid call (form, counts, tile multiples, K, an
 * alignment, a leading dimension, an orientation that does not belong to the form, an operand outside its buffer, riders the form
 * does not take); 2 on a HIP error.  riders may be null (none). */
int dqnhip_test_hgemm_form(int32_t form, int32_t n_problems, const dqnhip_test_hproblem* problems, const dqnhip_test_hriders* riders);

/* One tower layer's backward without transposed panels (see gemm_bench.hip): dgrad with the weight operand read
 * reduction-major, wgrad with both operands reduction-major, each alone and both in one launch; us[3] = the three
 * timings, max_abs_err over all results against the naive reference. */
int dqnhip_test_hgemm_backward(int32_t rows, int32_t n_out, int32_t k_in, int32_t iters, float* us, float* max_abs_err, float* max_ref);

/* Times the fused clip+Adam+soft-update pass on n_params random parameters (see gemm_bench.hip).
 * variant = 10*U + NT (U in {1,2,4} float4 per array in flight per thread, NT = non-temporal
 * gradient loads); touch_mb = MB of unrelated traffic between two passes (0: back to back). */
int dqnhip_test_adam(int64_t n_params, int32_t variant, int32_t blocks, int32_t iters, int32_t touch_mb, float* avg_us);

/* Persistent-kernel probe: `layers` dependent 256 x 1024 x 1024 forward layers as `layers` launches of the
 * learner's gemm_fwd_lds<2,2> vs ONE launch of 256 co-resident workgroups with per-(layer, 32-row slab)
 * arrival counters (see gemm_bench.hip).  map bit 0: 0 the learner's tile->XCD map, 1 one slab per XCD;
 * bit 1: hand-off by write-through (sc1) tile stores without a release fence instead of plain stores + release;
 * bit 2: the SEPARATE launches use write-through output stores (does a boundary get cheaper with nothing dirty?).
 * max_abs_diff compares the two results (same arithmetic: expected 0); gave_up != 0 if a bounded spin expired. */
int dqnhip_test_chain(int32_t layers, int32_t map, int32_t iters, float* us_launches, float* us_persistent,
                      float* max_abs_diff, int32_t* gave_up);

/* CU load-path probe (see gemm_bench.hip): `blocks` workgroups of 256 threads each stream `iters` 32-KiB pieces from a
 * region of region_kb KiB shared by the workgroups of one XCD.  mode 0 register loads, 1 LDS-DMA, 2 LDS-DMA + fragment
 * reads.  tb_per_s = bytes delivered to the CUs per second, chip-wide. */
int dqnhip_test_loadpath(int32_t mode, int32_t blocks, int32_t region_kb, int32_t iters, int32_t launches,
                         float* avg_us, float* tb_per_s);

/* Optimiser-under-GEMM overlap probe (see gemm_bench.hip): `layers` dependent 256 x 1024 x 1024 forward launches and one
 * k_adam_soft pass over adam_params parameters; us[0] launches alone, [1] pass alone, [2] serial, [3] the pass as rider
 * workgroups of the launches (48-KiB LDS build: riders co-resident), [4] on a second stream, [5] riders with the 96-KiB
 * build (not co-resident).  rider_blocks = rider workgroups per launch. */
int dqnhip_test_overlap(int32_t layers, int64_t adam_params, int32_t rider_blocks, int32_t iters, float* us);
/* launch-floor probe: us per kernel of a `chain`-long dependent chain inside a replayed hipGraph (variant bits: 1 = 640-byte
 * kernarg, 2 = lds_bytes of dynamic LDS, 4 = one dependent global round trip in the body, 8 = 1024 threads per block) */
int dqnhip_test_launch_floor(int32_t variant, int32_t blocks, int32_t lds_bytes, int32_t chain, int32_t iters, float* us_per_kernel);

#ifdef __cplusplus
}
#endif
#endif
