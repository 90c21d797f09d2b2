// sweep_kernels.hip.h — the replay sweep (dqnhip_evaluate_memory / dqnhip_per_refresh, include/dqnhip.h has the definitions): the
// row arithmetic and the reduction behind the forward passes of one chunk of B consecutive transitions.  Included and launched by
// learner_eval.hip only; a learner that never sweeps launches none of this.  What a chunk launches in front of k_sweep_rows — the
// update's gather and its forward launches, no backward, no optimiser — is sweep_forward's business (learner.hip).
//
// The chunk base lives in device memory (SweepDev), as the indices of a captured update do: one captured chunk serves every chunk.
//   k_sweep_begin  once per sweep: the window, chunk 0, and chunk 0's indices into the buffer the gather reads
//   k_sweep_rows   once per chunk, ONE workgroup: from the [B] row buffers the forward launches left and the gathered stored actions
//                  it forms td = q - y, q - mc and the action match of the chunk's valid rows (a tail chunk is padded with the
//                  window's last index: pad rows are computed, and counted nowhere), writes the per-row outputs at the rows'
//                  place in the window, |td| of every row for a refresh's write-back (a pad row carries the last valid row's
//                  transition, hence its value), leaves one SweepPart in the chunk's own slot, then advances the chunk counter and
//                  writes the next chunk's indices
//   k_sweep_final  once per sweep, ONE workgroup: the chunks' SweepParts in chunk order into the report
// Sums: diag_kernels.hip.h's accumulators and its one order — double, per-thread partials in element order (thread t: rows t,
// t + 256, ..) -> wave butterfly -> the four waves in order -> the chunk's slot -> the finaliser's threads in chunk order (thread
// t: chunks t, t + 256, ..), butterfly, waves.  No floating-point atomic anywhere: two sweeps of the same memory with the same
// nets are byte-identical.  Counts and histogram bins use integer atomics in LDS.
#pragma once
#include "diag_kernels.hip.h"      // DiagRowAcc, diag_row_add, diag_row_block_raw, diag_hist, DiagLds

namespace dqnhip {

enum SweepQuantity { SWEEP_Q = 0, SWEEP_Y, SWEEP_TD, SWEEP_Q_POLICY, SWEEP_MC, SWEEP_Q_MINUS_MC, SWEEP_REWARD, kSweepQuantities };

struct SweepDev { int first, n, chunk, pad; };
// mn / mx raw: +inf / -inf where the chunk had no finite value of the quantity
struct SweepMom { float mn, mx; double s, ss; unsigned nnf, pad; };
struct SweepPart { SweepMom mom[kSweepQuantities]; int hist[kDiagHistBins]; unsigned n_terminal, n_match, pad[2]; };
struct SweepOut {
  SweepMom mom[kSweepQuantities];      // as a report states them: min = max = 0 where there was no finite value
  int hist[kDiagHistBins];
  long long n_terminal, n_match;
  int first, n, n_chunks, actor_iter, critic_iter, pad;
};
struct SweepRowsArgs {
  SweepDev* sw; int B;
  const float *q, *y, *q_policy, *mc, *reward, *term;      // [B]: what k_head_q_train, the q head and the gather left
  const float* stored; int ld_stored;                        // the gathered stored actor outputs: row i's kNO values at stored[i * ld_stored]
  const float* aout16;                                       // mu(s): [B][kAP]
  int* idx;                                                  // [B]: the buffer the gather reads
  SweepPart* parts;
  float *o_q, *o_y, *o_td, *o_q_policy; int* o_match;        // [window, rounded up to whole chunks]
  float* td_abs;                                             // [B], a refresh only (null: an evaluation)
};

// index i of chunk c of the window [first, first + n): pad rows repeat the window's last index
__device__ __forceinline__ int sweep_index(int first, int n, int c, int B, int i) {
  const long long k = (long long)c * B + i;
  return first + (int)(k < n ? k : n - 1);
}
// GetAction's index (src/dqn.cpp:196-208): TACKLE masked, the first maximum wins
__device__ __forceinline__ int sweep_get_action(const float* ao) {
  const float c0 = ao[0], c1 = ao[1], c2 = -99999.0f, c3 = ao[3];
  int best = 0; float bv = c0;
  if (c1 > bv) { best = 1; bv = c1; }
  if (c2 > bv) { best = 2; bv = c2; }
  if (c3 > bv) { best = 3; bv = c3; }
  return best;
}

static __global__ __launch_bounds__(256) void k_sweep_begin(SweepDev* sw, int first, int n, int* idx, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) { sw->first = first; sw->n = n; sw->chunk = 0; sw->pad = 0; }
  if (i < B && n > 0) idx[i] = sweep_index(first, n, 0, B, i);
}

static __global__ __launch_bounds__(256) void k_sweep_rows(const SweepRowsArgs a) {
  __shared__ DiagLds s;
  __shared__ unsigned s_cnt[2];
  const int t = threadIdx.x, B = a.B;
  if (t < kDiagHistBins) s.hist[t] = 0;
  if (t < 2) s_cnt[t] = 0u;
  __syncthreads();
  const int first = a.sw->first, n = a.sw->n, c = a.sw->chunk;
  const long long base = (long long)c * B;
  DiagRowAcc acc[kSweepQuantities];
#pragma unroll
  for (int k = 0; k < kSweepQuantities; ++k) acc[k] = DiagRowAcc{INFINITY, -INFINITY, 0.0, 0.0, 0u};
  unsigned n_term = 0, n_match = 0;
  for (int i = t; i < B; i += 256) {
    const float q = a.q[i], y = a.y[i];
    const float td = q - y;
    if (a.td_abs != nullptr) a.td_abs[i] = fabsf(td);
    if (base + i >= n) continue;                       // a pad row
    const float qp = a.q_policy[i], mc = a.mc[i], r = a.reward[i];
    const float qmm = q - mc;
    const int match = sweep_get_action(a.aout16 + (size_t)i * kAP) == sweep_get_action(a.stored + (size_t)i * a.ld_stored) ? 1 : 0;
    const size_t o = (size_t)(base + i);
    a.o_q[o] = q; a.o_y[o] = y; a.o_td[o] = td; a.o_q_policy[o] = qp; a.o_match[o] = match;
    diag_row_add(acc[SWEEP_Q], q, true); diag_row_add(acc[SWEEP_Y], y, true); diag_row_add(acc[SWEEP_TD], td, true);
    diag_row_add(acc[SWEEP_Q_POLICY], qp, true); diag_row_add(acc[SWEEP_MC], mc, true);
    diag_row_add(acc[SWEEP_Q_MINUS_MC], qmm, true); diag_row_add(acc[SWEEP_REWARD], r, true);
    diag_hist(s.hist, td);
    n_term += a.term[i] != 0.0f ? 1u : 0u; n_match += (unsigned)match;
  }
  n_term = diag_wave_u(n_term); n_match = diag_wave_u(n_match);
  if ((t & 63) == 0) { atomicAdd(&s_cnt[0], n_term); atomicAdd(&s_cnt[1], n_match); }
  SweepPart* out = a.parts + c;
#pragma unroll
  for (int k = 0; k < kSweepQuantities; ++k) {
    const DiagRowAcc r = diag_row_block_raw(acc[k], s);
    if (t == 0) out->mom[k] = SweepMom{r.mn, r.mx, r.s, r.ss, r.cnt, 0u};
  }
  __syncthreads();                                     // (s.hist, s_cnt complete; every row of the chunk has been read)
  if (t < kDiagHistBins) out->hist[t] = s.hist[t];
  if (t == 0) { out->n_terminal = s_cnt[0]; out->n_match = s_cnt[1]; out->pad[0] = 0u; out->pad[1] = 0u; a.sw->chunk = c + 1; }
  for (int i = t; i < B; i += 256) a.idx[i] = sweep_index(first, n, c + 1, B, i);
}

// (the host launches nothing for n == 0)
static __global__ __launch_bounds__(256) void k_sweep_final(const SweepDev* sw, const DevState* st, const SweepPart* parts, int B, SweepOut* out) {
  __shared__ DiagLds s;
  __shared__ unsigned s_cnt[2];
  const int t = threadIdx.x;
  if (t < kDiagHistBins) s.hist[t] = 0;
  if (t < 2) s_cnt[t] = 0u;
  __syncthreads();
  const int n = sw->n, n_chunks = (n + B - 1) / B;
  DiagRowAcc acc[kSweepQuantities];
#pragma unroll
  for (int k = 0; k < kSweepQuantities; ++k) acc[k] = DiagRowAcc{INFINITY, -INFINITY, 0.0, 0.0, 0u};
  unsigned n_term = 0, n_match = 0;
  for (int c = t; c < n_chunks; c += 256) {
    const SweepPart& p = parts[c];
#pragma unroll
    for (int k = 0; k < kSweepQuantities; ++k) {
      const SweepMom& m = p.mom[k];
      acc[k].mn = fminf(acc[k].mn, m.mn); acc[k].mx = fmaxf(acc[k].mx, m.mx); acc[k].s += m.s; acc[k].ss += m.ss; acc[k].cnt += m.nnf;
    }
    n_term += p.n_terminal; n_match += p.n_match;
  }
  // the bins: wave w takes chunks w, w + 4, .., lane b bin b (k_diag_final's walk)
  {
    const int bin = t & 63;
    int cnt = 0;
    for (int c = t >> 6; c < n_chunks; c += 4) cnt += parts[c].hist[bin];
    if (cnt != 0) atomicAdd(&s.hist[bin], cnt);
  }
  n_term = diag_wave_u(n_term); n_match = diag_wave_u(n_match);
  if ((t & 63) == 0) { atomicAdd(&s_cnt[0], n_term); atomicAdd(&s_cnt[1], n_match); }
#pragma unroll
  for (int k = 0; k < kSweepQuantities; ++k) {
    DiagRowAcc r = diag_row_block_raw(acc[k], s);
    if (r.mn > r.mx) { r.mn = 0.0f; r.mx = 0.0f; }
    if (t == 0) out->mom[k] = SweepMom{r.mn, r.mx, r.s, r.ss, r.cnt, 0u};
  }
  __syncthreads();
  if (t < kDiagHistBins) out->hist[t] = s.hist[t];
  if (t == 0) {
    out->n_terminal = (long long)s_cnt[0]; out->n_match = (long long)s_cnt[1];
    out->first = sw->first; out->n = n; out->n_chunks = n_chunks;
    out->actor_iter = st->actor_iter; out->critic_iter = st->critic_iter; out->pad = 0;
  }
}

}  // namespace dqnhip
