// diag_kernels.hip.h — update diagnostics (dqnhip_diag_collect, include/dqnhip.h has the definitions): what the last update left on
// the device, reduced on the device to a few tens of KB.  Included and launched by learner_eval.hip only; a learner that never collects
// launches none of this.  A collection READS the learner and writes nothing but its own scratch.
//
// Three launches per collection:
//   k_diag_prep    one block: s[net] = lr * adam_correction(beta1, beta2, iter) of both nets from the iteration counters as they stand
//                  (what adam_apply4 multiplied by in the last step), 0 while the iteration is 0
//   k_diag_reduce  one 256-thread workgroup per work item (the table lives in a device buffer, built on first use):
//                    parameter blob  a chunk of kDiagChunk floats of the blob's [rows][pitch] image; w, w', g, m, v are read once,
//                                    together, with 16-byte loads, as the optimiser pass reads them.  Pad columns (layer 0: pitch >
//                                    cols) and whatever follows a blob in its last 16 bytes are loaded and never counted
//                    panel           a strip of 64 (fp16: 128) columns of an activation panel, all rows: a column's rows stay in one
//                                    workgroup, so dead units are counted here
//                    rows            one quantity of the [B] buffers each (the four Q rows, td, an actor-output column, dQ/da +
//                                    terminal, the importance weights): written straight to DiagRows
//                  every item leaves one DiagPart in its own slot of the partial slab
//   k_diag_final   one workgroup per segment (blob / panel): its items' DiagParts in item order
// Sums: double, per-thread partials in element order -> wave butterfly (xor 32 .. 1: both lanes of a pair form the same sum) -> the
// four waves in order -> the slab -> the finaliser's threads in item order, butterfly, waves.  One fixed order, no floating-point
// atomic anywhere: two collections of the same buffers are byte-identical.  Counts and histogram bins use integer atomics in LDS.
#pragma once
#include "update_bodies.hip.h"      // adam_correction

namespace dqnhip {

constexpr int kDiagChunk = 4096;    // floats of a blob image per work item: 4 x 16 bytes per array per thread
constexpr int kDiagHistBins = 64;
enum DiagSegType { DIAG_BLOB = 0, DIAG_PANEL = 1 };
enum DiagRowItem { DIAG_ROW_Q = 0 /* .. 4: q_target, y, q_train, q_policy, td */, DIAG_ROW_ACT = 5 /* .. 14 */, DIAG_ROW_DQDA = 15, DIAG_ROW_PER = 16,
                   kDiagRowItems = 17 };

struct DiagMomPart { double sum_abs, sum_sq; float max_abs; unsigned n_zero, n_nonfinite, pad; };
// blob: mom[0..3] = w, g, lag, step, hist of g.  panel: mom[0], hist, n_negative, dead
struct DiagPart { DiagMomPart mom[4]; int hist[kDiagHistBins]; unsigned n_negative; int dead; int pad[2]; };
struct DiagSeg {
  const float *w, *wt, *g, *m, *v;      // blob: the blob's first float in each arena (16-byte aligned)
  const void* panel;                    // panel: [rows][pitch] float, or _Float16 (is16)
  int type, net, is16;
  int rows, cols, pitch;                // logical columns < pitch only in layer 0's weights
  int first_item, n_items;
};
struct DiagItem { int seg, chunk; };     // seg < 0: rows item `chunk`
struct DiagRowStat { float mn, mx; double sum, sum_sq; unsigned n_nonfinite, pad; };
struct DiagActStat { float mn, mx; double sum; unsigned n_oob, pad; };
struct DiagRows {
  DiagRowStat row[5];
  DiagActStat act[kNO];
  double dqda_sum_abs; float dqda_max_abs; unsigned n_terminal;
  double per_w_sum; float per_w_min, per_prob_min, per_td_abs_max, pad;
  float step_scale[2]; int iter[2];     // k_diag_prep
};
struct DiagArgs {
  const DiagSeg* segs; const DiagItem* items; DiagPart* parts; DiagRows* rows;
  int B; float delta;
  const float *q_t, *y, *q1, *q2, *term, *aout16, *dA16;
  const float *per_w, *per_prob, *per_td;      // null: not a prioritized learner
};

struct DiagAcc { double sa, ss; float mx; unsigned nz, nnf; };
__device__ __forceinline__ void diag_add(DiagAcc& a, double x) {
  if (x == 0.0) a.nz += 1;
  else if (!isfinite(x)) a.nnf += 1;
  else { const double ax = fabs(x); a.sa += ax; a.ss += x * x; a.mx = fmaxf(a.mx, (float)ax); }
}
// bin = min(max(e - 87, 0), 63) of the biased exponent field (denormals: e = 0); finite non-zero values only
__device__ __forceinline__ void diag_hist(int* s_hist, float x) {
  const unsigned b = __float_as_uint(x), e = (b >> 23) & 0xffu;
  if (e == 0xffu || (b & 0x7fffffffu) == 0u) return;
  const int bin = (int)e - 87;
  atomicAdd(&s_hist[bin < 0 ? 0 : (bin > 63 ? 63 : bin)], 1);
}
__device__ __forceinline__ void diag_wave(DiagAcc& a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a.sa += __shfl_xor(a.sa, off, 64); a.ss += __shfl_xor(a.ss, off, 64);
    a.mx = fmaxf(a.mx, __shfl_xor(a.mx, off, 64));
    a.nz += __shfl_xor(a.nz, off, 64); a.nnf += __shfl_xor(a.nnf, off, 64);
  }
}
__device__ __forceinline__ unsigned diag_wave_u(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
struct DiagLds { DiagAcc acc[4][4]; int hist[kDiagHistBins]; int cols[128]; unsigned cnt[4]; int dead; };
// the block's K accumulators and counters -> *out (thread 0 writes; waves combined in order).  s.hist / s.dead are complete before
__device__ __forceinline__ void diag_block_out(DiagLds& s, DiagAcc* a, int K, unsigned nneg, DiagPart* out) {
  const int t = threadIdx.x;
  for (int k = 0; k < K; ++k) { diag_wave(a[k]); if ((t & 63) == 0) s.acc[k][t >> 6] = a[k]; }
  nneg = diag_wave_u(nneg);
  if ((t & 63) == 0) s.cnt[t >> 6] = nneg;
  __syncthreads();
  if (t < kDiagHistBins) out->hist[t] = s.hist[t];
  if (t != 0) return;
  for (int k = 0; k < 4; ++k) {
    DiagMomPart m{0.0, 0.0, 0.0f, 0u, 0u, 0u};
    if (k < K)
      for (int w = 0; w < 4; ++w) {
        const DiagAcc& p = s.acc[k][w];
        m.sum_abs += p.sa; m.sum_sq += p.ss; m.max_abs = fmaxf(m.max_abs, p.mx); m.n_zero += p.nz; m.n_nonfinite += p.nnf;
      }
    out->mom[k] = m;
  }
  out->n_negative = (s.cnt[0] + s.cnt[1]) + (s.cnt[2] + s.cnt[3]);
  out->dead = s.dead; out->pad[0] = 0; out->pad[1] = 0;
}

// ---- a chunk of a parameter blob ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void diag_blob_item(const DiagArgs& a, const DiagSeg& sg, int chunk, DiagLds& s, DiagPart* out) {
  const int t = threadIdx.x;
  const size_t total = (size_t)sg.rows * sg.pitch, n4 = (total + 3) / 4;
  const bool padded = sg.pitch != sg.cols;            // (then pitch % 64 == 0: a float4 never straddles two rows)
  f32x4 w[4], wt[4], g[4], m[4], v[4];
  const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const size_t q = (size_t)chunk * (kDiagChunk / 4) + (size_t)u * 256 + t;
    w[u] = wt[u] = g[u] = m[u] = v[u] = z;
    if (q < n4) {
      w[u] = reinterpret_cast<const f32x4*>(sg.w)[q]; wt[u] = reinterpret_cast<const f32x4*>(sg.wt)[q];
      g[u] = reinterpret_cast<const f32x4*>(sg.g)[q]; m[u] = reinterpret_cast<const f32x4*>(sg.m)[q];
      v[u] = reinterpret_cast<const f32x4*>(sg.v)[q];
    }
  }
  const float scale = a.rows->step_scale[sg.net];
  const bool it0 = a.rows->iter[sg.net] == 0;
  DiagAcc acc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = DiagAcc{0.0, 0.0, 0.0f, 0u, 0u};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const size_t q = (size_t)chunk * (kDiagChunk / 4) + (size_t)u * 256 + t;
    if (q >= n4) continue;
    const int c0 = padded ? (int)((q * 4) % (size_t)sg.pitch) : 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool valid = q * 4 + e < total && (!padded || c0 + e < sg.cols);
      if (!valid) continue;
      const float we = w[u][e], te = wt[u][e], ge = g[u][e], me = m[u][e], ve = v[u][e];
      diag_add(acc[0], (double)we);
      diag_add(acc[1], (double)ge);
      diag_hist(s.hist, ge);
      diag_add(acc[2], (double)we - (double)te);
      const float st = it0 ? 0.0f : scale * (me / (sqrtf(ve) + a.delta));
      diag_add(acc[3], (double)st);
    }
  }
  diag_block_out(s, acc, 4, 0u, out);
}

// ---- a column strip of an activation panel -------------------------------------------------------------------------------------
// 16 lanes x VEC columns per row, 16 rows per step: every load is 16 bytes, a row's piece of the strip is whole 256-byte lines
template <bool IN16>
__device__ __forceinline__ void diag_panel_item(const DiagSeg& sg, int strip, DiagLds& s, DiagPart* out) {
  constexpr int VEC = IN16 ? 8 : 4, SW = 16 * VEC;
  typedef __attribute__((ext_vector_type(8))) _Float16 h16x8;
  const int t = threadIdx.x, lc = t & 15, rg = t >> 4;
  const int col = strip * SW + lc * VEC;
  DiagAcc acc = DiagAcc{0.0, 0.0, 0.0f, 0u, 0u};
  unsigned nneg = 0; bool allneg[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) allneg[e] = true;
  if (col < sg.cols) {                                 // (cols % SW == 0: always)
#pragma unroll 4
    for (int r = rg; r < sg.rows; r += 16) {
      float x[VEC];
      if constexpr (IN16) {
        const h16x8 h = *reinterpret_cast<const h16x8*>(reinterpret_cast<const _Float16*>(sg.panel) + (size_t)r * sg.pitch + col);
#pragma unroll
        for (int e = 0; e < VEC; ++e) x[e] = (float)h[e];
      } else {
        const f32x4 f = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(sg.panel) + (size_t)r * sg.pitch + col);
#pragma unroll
        for (int e = 0; e < VEC; ++e) x[e] = f[e];
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        diag_add(acc, (double)x[e]);
        diag_hist(s.hist, x[e]);
        const bool neg = x[e] < 0.0f;
        nneg += neg ? 1u : 0u; allneg[e] = allneg[e] && neg;
      }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) if (!allneg[e]) atomicAnd(&s.cols[lc * VEC + e], 0);      // (rows >= 16: every thread has seen a row)
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) atomicAnd(&s.cols[lc * VEC + e], 0);
  }
  __syncthreads();
  if (t < SW && s.cols[t] != 0) atomicAdd(&s.dead, 1);
  __syncthreads();
  diag_block_out(s, &acc, 1, nneg, out);
}

// ---- the [B] row buffers ---------------------------------------------------------------------------------------------------
struct DiagRowAcc { float mn, mx; double s, ss; unsigned cnt; };
// over the block: min / max / sums of the finite values, cnt summed; every thread holds the result.  No finite value: min = +inf,
// max = -inf (what a further reduction over several blocks' results needs: sweep_kernels.hip.h)
__device__ __forceinline__ DiagRowAcc diag_row_block_raw(DiagRowAcc r, DiagLds& sm) {
  const int t = threadIdx.x;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    r.mn = fminf(r.mn, __shfl_xor(r.mn, off, 64)); r.mx = fmaxf(r.mx, __shfl_xor(r.mx, off, 64));
    r.s += __shfl_xor(r.s, off, 64); r.ss += __shfl_xor(r.ss, off, 64); r.cnt += __shfl_xor(r.cnt, off, 64);
  }
  __syncthreads();                                     // (the LDS slots may still be read from a previous call)
  if ((t & 63) == 0) { DiagAcc& p = sm.acc[0][t >> 6]; p.sa = r.s; p.ss = r.ss; p.mx = r.mx; p.nz = __float_as_uint(r.mn); p.nnf = r.cnt; }
  __syncthreads();
  DiagRowAcc o{INFINITY, -INFINITY, 0.0, 0.0, 0u};
  for (int w = 0; w < 4; ++w) {
    const DiagAcc& p = sm.acc[0][w];
    o.mn = fminf(o.mn, __uint_as_float(p.nz)); o.mx = fmaxf(o.mx, p.mx); o.s += p.sa; o.ss += p.ss; o.cnt += p.nnf;
  }
  return o;
}
// ... as a report states it: no finite value: min = max = 0
__device__ __forceinline__ DiagRowAcc diag_row_block(DiagRowAcc r, DiagLds& sm) {
  DiagRowAcc o = diag_row_block_raw(r, sm);
  if (o.mn > o.mx) { o.mn = 0.0f; o.mx = 0.0f; }
  return o;
}
__device__ __forceinline__ void diag_row_add(DiagRowAcc& r, float x, bool square) {
  if (!isfinite(x)) { r.cnt += 1; return; }
  r.mn = fminf(r.mn, x); r.mx = fmaxf(r.mx, x); r.s += (double)x; if (square) r.ss += (double)x * (double)x;
}
__device__ __forceinline__ void diag_rows_item(const DiagArgs& a, int what, DiagLds& sm) {
  const int t = threadIdx.x, B = a.B;
  DiagRows* o = a.rows;
  const DiagRowAcc zero{INFINITY, -INFINITY, 0.0, 0.0, 0u};
  if (what < DIAG_ROW_ACT) {
    const float* src = what == 0 ? a.q_t : what == 1 ? a.y : what == 2 ? a.q1 : a.q2;
    DiagRowAcc r = zero;
    for (int i = t; i < B; i += 256) diag_row_add(r, what == 4 ? a.q1[i] - a.y[i] : src[i], true);
    r = diag_row_block(r, sm);
    if (t == 0) o->row[what] = DiagRowStat{r.mn, r.mx, r.s, r.ss, r.cnt, 0u};
  } else if (what < DIAG_ROW_DQDA) {
    const int j = what - DIAG_ROW_ACT;
    float lo, hi; inverting_bounds(j, lo, hi);
    DiagRowAcc r = zero; unsigned oob = 0;
    for (int i = t; i < B; i += 256) {
      const float x = a.aout16[(size_t)i * kAP + j];
      if (isfinite(x)) { r.mn = fminf(r.mn, x); r.mx = fmaxf(r.mx, x); r.s += (double)x; }
      oob += (x >= lo && x <= hi) ? 0u : 1u;             // (NaN is inside no interval)
    }
    r.cnt = oob;
    r = diag_row_block(r, sm);
    if (t == 0) o->act[j] = DiagActStat{r.mn, r.mx, r.s, r.cnt, 0u};
  } else if (what == DIAG_ROW_DQDA) {
    DiagRowAcc r = zero;
    for (int i = t; i < B * kNO; i += 256) {
      const float x = a.dA16[(size_t)(i / kNO) * kAP + (i % kNO)];
      if (isfinite(x)) { const float ax = fabsf(x); r.mx = fmaxf(r.mx, ax); r.mn = fminf(r.mn, ax); r.s += (double)ax; }
    }
    for (int i = t; i < B; i += 256) r.cnt += a.term[i] != 0.0f ? 1u : 0u;
    r = diag_row_block(r, sm);
    if (t == 0) { o->dqda_sum_abs = r.s; o->dqda_max_abs = r.mx; o->n_terminal = r.cnt; }
  } else {
    float wmin = 0.0f, pmin = 0.0f, tmax = 0.0f; double wsum = 0.0;
    if (a.per_w != nullptr) {                          // (block-uniform)
      DiagRowAcc r = zero;
      for (int i = t; i < B; i += 256) diag_row_add(r, a.per_w[i], false);
      r = diag_row_block(r, sm); wmin = r.mn; wsum = r.s;
      r = zero;
      for (int i = t; i < B; i += 256) diag_row_add(r, a.per_prob[i], false);
      r = diag_row_block(r, sm); pmin = r.mn;
      r = zero;
      for (int i = t; i < B; i += 256) diag_row_add(r, a.per_td[i], false);
      r = diag_row_block(r, sm); tmax = r.mx;
    }
    if (t == 0) { o->per_w_sum = wsum; o->per_w_min = wmin; o->per_prob_min = pmin; o->per_td_abs_max = tmax; o->pad = 0.0f; }
  }
}

struct DiagPrepArgs { const DevState* st; DiagRows* rows; float lr[2]; float beta1, beta2; };
static __global__ __launch_bounds__(64) void k_diag_prep(const DiagPrepArgs p) {
  const int which = threadIdx.x;
  if (which >= 2) return;
  const int it = which == 0 ? p.st->actor_iter : p.st->critic_iter;
  p.rows->iter[which] = it;
  p.rows->step_scale[which] = it > 0 ? p.lr[which] * adam_correction(p.beta1, p.beta2, it) : 0.0f;
}

static __global__ __launch_bounds__(256) void k_diag_reduce(const DiagArgs a) {
  __shared__ DiagLds s;
  const int t = threadIdx.x;
  if (t < kDiagHistBins) s.hist[t] = 0;
  if (t < 128) s.cols[t] = 1;
  if (t == 0) s.dead = 0;
  __syncthreads();
  const DiagItem it = a.items[blockIdx.x];
  if (it.seg < 0) { diag_rows_item(a, it.chunk, s); return; }
  const DiagSeg sg = a.segs[it.seg];
  DiagPart* out = a.parts + sg.first_item + it.chunk;
  if (sg.type == DIAG_BLOB) diag_blob_item(a, sg, it.chunk, s, out);
  else if (sg.is16) diag_panel_item<true>(sg, it.chunk, s, out);
  else diag_panel_item<false>(sg, it.chunk, s, out);
}

// one workgroup per segment: thread t takes items t, t + 256, .. in order
static __global__ __launch_bounds__(256) void k_diag_final(const DiagSeg* segs, const DiagPart* parts, DiagPart* out) {
  __shared__ DiagLds s;
  const int t = threadIdx.x;
  if (t < kDiagHistBins) s.hist[t] = 0;
  if (t == 0) s.dead = 0;
  __syncthreads();
  const DiagSeg sg = segs[blockIdx.x];
  DiagAcc acc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = DiagAcc{0.0, 0.0, 0.0f, 0u, 0u};
  unsigned nneg = 0; int dead = 0;
  for (int i = t; i < sg.n_items; i += 256) {
    const DiagPart& p = parts[sg.first_item + i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc[k].sa += p.mom[k].sum_abs; acc[k].ss += p.mom[k].sum_sq; acc[k].mx = fmaxf(acc[k].mx, p.mom[k].max_abs);
      acc[k].nz += p.mom[k].n_zero; acc[k].nnf += p.mom[k].n_nonfinite;
    }
    nneg += p.n_negative; dead += p.dead;
  }
  if (dead != 0) atomicAdd(&s.dead, dead);
  // the bins: wave w takes items w, w + 4, .., lane b bin b — one coalesced 256-byte load per item (a thread walking the 64 bins of
  // its own item made this launch slower than the reduction it finishes: 60 us at the headline shape)
  {
    const int bin = t & 63;
    int c = 0;
    for (int i = t >> 6; i < sg.n_items; i += 4) c += parts[sg.first_item + i].hist[bin];
    if (c != 0) atomicAdd(&s.hist[bin], c);
  }
  __syncthreads();
  diag_block_out(s, acc, 4, nneg, out + blockIdx.x);
}

}  // namespace dqnhip
