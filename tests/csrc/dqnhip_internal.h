/*
 * dqnhip_internal.h — test / tuning hooks exported by libdqnhip_test.so (csrc/gemm_bench.hip: the timing harness and the
 * probes; csrc/gemm_forms.hip: dqnhip_test_gemm_form, one launch of a product GEMM form on caller-made buffers).  Not part of
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
/* form: one id per launcher template instance learner.hip reaches for the fp32 tower (riders aside) */
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
