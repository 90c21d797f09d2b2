// update_bodies.hip.h — the BODIES of the kernels around the GEMMs: __device__ functions (and the HEAD_DISPATCH macro the head
// kernels enter their loops through), no kernel.  The sampling RNG, the minibatch gather, the head kernels' loads, the optimiser
// pass with its first-layer riders, the update's bookkeeping.  Several kernels carry each of them (a launch of its own, or rider
// blocks of another launch): small_kernels.hip.h, head_*kernels.hip.h, io_kernels.hip.h, env.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "gemm_bodies.hip.h"

namespace dqnhip {

// ---- counter-based RNG (Philox-4x32-10) for SampleTransitionsFromMemory ------
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n1 = (uint32_t)p1;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  const uint32_t n3 = (uint32_t)p0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
__device__ __forceinline__ uint32_t philox_u32(uint64_t seed, uint64_t ctr, uint32_t lane) {
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), lane, 0x9E3779B9u};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) { philox_round(c, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
  return c[0];
}

// correction = sqrt(1 - beta2^t) / (1 - beta1^t), evaluated in double, rounded once (Caffe's AdamSolver)
__device__ __forceinline__ float adam_correction(float beta1, float beta2, int t) {
  return (float)(sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t)));
}

// A scheduled learner's step scale (GatherArgs::sched): the rate of iteration `iter` times the bias correction, both rounded to
// float32 first.  Out of line: the scalars block of a fixed learner keeps its registers and its code.
__device__ __noinline__ float lr_rate_scaled(const LrSchedule& s, int net, int iter, float corr) {
#pragma clang fp contract(off)
  return lr_rate(s, net, iter) * corr;
}

// ---- minibatch gather (k_gather; rider of k_adam_soft_gather / k_adam_soft_fwd1_gather) ---------------------------------------
__device__ __forceinline__ void gather_block(const GatherArgs& g, const int blk) {
  const DevState* st = g.st;
  if (blk == g.blocks - 1) {
    int it_a, it_c;
    if (g.ahead == -2) { it_a = st->actor_iter + 1; it_c = st->critic_iter + 1; }      // rides in the PREVIOUS update's critic launch, before that update's tick (dqnhip_update_chained)
    else if (g.ahead < 0) { it_a = st->actor_iter; it_c = st->critic_iter; }
    else { it_a = st->gbase_it[0] + g.ahead; it_c = st->gbase_it[1] + g.ahead; }
    if (threadIdx.x == 64) *g.soft_now = ((((it_a + 1) > (it_c + 1) ? (it_a + 1) : (it_c + 1)) % g.soft_update_freq) == 0);
    if (threadIdx.x == 65 && g.store_base) { g.st->gbase_counter = st->update_counter; g.st->gbase_it[0] = it_a; g.st->gbase_it[1] = it_c; }
    // four lanes, one pow() each (the two powers of a correction side by side: half the dependent chain), same
    // expression as adam_correction() from there on
    if (threadIdx.x < 64) {
      const int which = (threadIdx.x >> 1) & 1, isb1 = threadIdx.x & 1;
      const int t = (which == 0 ? it_a : it_c) + 1;
      const double pw = pow((double)(isb1 ? g.beta1 : g.beta2), (double)t);
      const double p1 = __shfl_down(pw, 1, 64);          // lane 2*which: pw = beta2^t, p1 = beta1^t
      if (threadIdx.x < 4 && !isb1) {
        const float corr = (float)(sqrt(1.0 - pw) / (1.0 - p1));
        if (g.sched != nullptr) g.corr[which] = lr_rate_scaled(*g.sched, which, t - 1, corr);
        else g.corr[which] = corr;
      }
    }
    return;
  }
  const GatherOut& o = g.o; const Ring& ring = g.ring;
  const int row = blk * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= g.B) return;
  const int size = g.rs->ring_size;
  int li;
  if (g.idx_in != nullptr) li = g.idx_in[row];
  else {
    // SampleTransitionsFromMemory (src/dqn.cpp:501-509): uniform in [0,size-1] with
    // replacement; counter-based so the draw depends only on (seed, update, row)
    const unsigned long long ctr = g.ahead < 0 ? st->update_counter : st->gbase_counter + (unsigned long long)g.ahead;
    const uint32_t u = philox_u32(g.seed, ctr, (uint32_t)row);
    li = (int)(((uint64_t)u * (uint64_t)size) >> 32);
  }
  li = li < 0 ? 0 : (li >= size ? size - 1 : li);
  const long long slot = ((long long)g.rs->ring_head + li) % ring.cap;
  const float* sp = ring.state + slot * ring.SP;
  const float* np = ring.next + slot * ring.SP;
  const float* ap = ring.act + slot * kAP;
  const int S = ring.S;
  if (o.Xa_s != nullptr)                       // (fp16 learner: nothing reads the fp32 panels — not written)
  for (int c = lane; c < o.KcP; c += 64) {
    const float sv = c < S ? sp[c] : 0.0f;
    const float nv = c < S ? np[c] : 0.0f;
    const float av = (c >= S && c < S + kNO) ? ap[c - S] : 0.0f;
    {
      if (c < o.KaP) { o.Xa_s[(size_t)row * o.KaP + c] = sv; o.Xa_n[(size_t)row * o.KaP + c] = nv; }
      o.Xc_tr[(size_t)row * o.KcP + c] = c < S ? sv : av;
      o.Xc_pl[(size_t)row * o.KcP + c] = sv;
      o.Xc_nx[(size_t)row * o.KcP + c] = nv;
    }
  }
  if (o.Ha_s != nullptr) {
    // fp16 learner: the five panels as fp16, two columns per lane (4-byte stores; 2-byte stores cost ~2x per byte and this
    // kernel writes 5 panels x 256 B per row).  Ring rows are whole 256-B lines (SP = roundup(S, 64) floats), so the pair
    // (c, c + 1) is one 8-byte load wherever c < S.  KaP, KcP are multiples of 128 in fp16 mode.
    typedef __attribute__((ext_vector_type(2))) _Float16 h2;
    typedef __attribute__((ext_vector_type(2))) float f2;
    for (int c = lane * 2; c < o.KcP; c += 128) {
      f2 sv = f2{0.f, 0.f}, nv = f2{0.f, 0.f};
      if (c < S) { sv = *reinterpret_cast<const f2*>(sp + c); nv = *reinterpret_cast<const f2*>(np + c); }      // (c even, rows padded to SP >= S + 1: in bounds)
      if (c + 1 >= S) { sv.y = 0.0f; nv.y = 0.0f; }      // whatever the ring holds beyond S never reaches a panel
      const float a0 = (c >= S && c < S + kNO) ? ap[c - S] : 0.0f, a1 = (c + 1 >= S && c + 1 < S + kNO) ? ap[c + 1 - S] : 0.0f;
      const h2 hs = h2{(_Float16)sv.x, (_Float16)sv.y}, hn = h2{(_Float16)nv.x, (_Float16)nv.y};
      if (c < o.KaP) { *reinterpret_cast<h2*>(o.Ha_s + (size_t)row * o.KaP + c) = hs; *reinterpret_cast<h2*>(o.Ha_n + (size_t)row * o.KaP + c) = hn; }
      *reinterpret_cast<h2*>(o.Hc_tr + (size_t)row * o.KcP + c) = h2{(_Float16)(c < S ? sv.x : a0), (_Float16)(c + 1 < S ? sv.y : a1)};
      *reinterpret_cast<h2*>(o.Hc_pl + (size_t)row * o.KcP + c) = hs;
      *reinterpret_cast<h2*>(o.Hc_nx + (size_t)row * o.KcP + c) = hn;
    }
  }
  if (lane == 0) {
    o.reward[row] = ring.reward[slot]; o.mc[row] = ring.mc[slot];
    o.term[row] = ring.term[slot] ? 1.0f : 0.0f; o.idx[row] = li;
  }
}

// ---- the n-step gather (k_gather_n; dqnhip_nstep_enable) ----------------------------------------------------------------------
// The window's discounted reward sum, Horner from the back, in double and without contraction, rounded to float once:
// acc = r[m - 1]; acc = (double)r[k] + gamma acc for k = m - 2 .. 0.  rv: lane k holds r[li + k]; m is wave-uniform and the whole
// wave walks the chain (the shuffles need every lane), so every lane returns R.  At m = 1 it is r[li] exactly.
__device__ __forceinline__ float nstep_reward(float rv, int m, double gamma) {
#pragma clang fp contract(off)
  double acc = (double)__shfl(rv, m - 1, 64);
  for (int k = m - 2; k >= 0; --k) acc = (double)__shfl(rv, k, 64) + gamma * acc;
  return (float)acc;
}
// gamma^m as m - 1 successive products (what a caller who wants the same bits on the host writes down); gamma itself at m = 1
__device__ __forceinline__ double nstep_discount(int m, double gamma) {
  double d = gamma;
  for (int k = 1; k < m; ++k) d = d * gamma;
  return d;
}
// gather_block with a window behind every sampled index (a copy of its row part, so that gather_block — its riders, its register
// budget — stays the code it is; the scalars block IS gather_block's).  One wave per row: lane k < n reads reward and terminal of
// logical li + k where that is inside the ring (slot (ring_head + li + k) % cap: a window may cross the ring's physical end); the
// window ends at the first lane that holds a terminal transition, the ring's last one, or lane n - 1: one ballot gives its length
// m.  State and action come from li, next state and terminal from b = li + m - 1.  Every path that fills the ring appends whole
// episodes contiguously, so b's stored next state is the state m steps after li's (k_nstep_validate checks that).
// Beside gather_block's traffic: at most n reward words and n terminal bytes per row.
__device__ __forceinline__ void gather_n_block(const GatherNArgs& a, const int blk) {
  const GatherArgs& g = a.g;
  if (blk == g.blocks - 1) { gather_block(g, blk); return; }      // the scalars block: the same code
  const DevState* st = g.st;
  const GatherOut& o = g.o; const Ring& ring = g.ring;
  const int row = blk * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= g.B) return;
  const int size = g.rs->ring_size;
  int li;
  if (g.idx_in != nullptr) li = g.idx_in[row];
  else {
    const unsigned long long ctr = g.ahead < 0 ? st->update_counter : st->gbase_counter + (unsigned long long)g.ahead;
    const uint32_t u = philox_u32(g.seed, ctr, (uint32_t)row);
    li = (int)(((uint64_t)u * (uint64_t)size) >> 32);
  }
  li = li < 0 ? 0 : (li >= size ? size - 1 : li);
  const long long head = g.rs->ring_head;
  float rv = 0.0f; int tv = 0;
  if (lane < a.n && li + lane < size) {
    const long long sk = (head + li + lane) % ring.cap;
    rv = ring.reward[sk]; tv = ring.term[sk];
  }
  const unsigned long long ends = __ballot(lane < a.n && (tv != 0 || li + lane >= size - 1 || lane == a.n - 1));
  const int m = __ffsll((long long)ends);          // 1 .. n: lane n - 1 always votes
  const float R = nstep_reward(rv, m, a.gamma);
  const int tb = __shfl(tv, m - 1, 64);
  const long long slot = (head + li) % ring.cap, slot_b = (head + li + m - 1) % ring.cap;
  const float* sp = ring.state + slot * ring.SP;
  const float* np = ring.next + slot_b * ring.SP;
  const float* ap = ring.act + slot * kAP;
  const int S = ring.S;
  if (o.Xa_s != nullptr)
  for (int c = lane; c < o.KcP; c += 64) {
    const float sv = c < S ? sp[c] : 0.0f;
    const float nv = c < S ? np[c] : 0.0f;
    const float av = (c >= S && c < S + kNO) ? ap[c - S] : 0.0f;
    if (c < o.KaP) { o.Xa_s[(size_t)row * o.KaP + c] = sv; o.Xa_n[(size_t)row * o.KaP + c] = nv; }
    o.Xc_tr[(size_t)row * o.KcP + c] = c < S ? sv : av;
    o.Xc_pl[(size_t)row * o.KcP + c] = sv;
    o.Xc_nx[(size_t)row * o.KcP + c] = nv;
  }
  if (o.Ha_s != nullptr) {
    // (gather_block's fp16 panel loop: two columns per lane, 8-byte loads inside whole 256-B ring rows)
    typedef __attribute__((ext_vector_type(2))) _Float16 h2;
    typedef __attribute__((ext_vector_type(2))) float f2;
    for (int c = lane * 2; c < o.KcP; c += 128) {
      f2 sv = f2{0.f, 0.f}, nv = f2{0.f, 0.f};
      if (c < S) { sv = *reinterpret_cast<const f2*>(sp + c); nv = *reinterpret_cast<const f2*>(np + c); }
      if (c + 1 >= S) { sv.y = 0.0f; nv.y = 0.0f; }
      const float a0 = (c >= S && c < S + kNO) ? ap[c - S] : 0.0f, a1 = (c + 1 >= S && c + 1 < S + kNO) ? ap[c + 1 - S] : 0.0f;
      const h2 hs = h2{(_Float16)sv.x, (_Float16)sv.y}, hn = h2{(_Float16)nv.x, (_Float16)nv.y};
      if (c < o.KaP) { *reinterpret_cast<h2*>(o.Ha_s + (size_t)row * o.KaP + c) = hs; *reinterpret_cast<h2*>(o.Ha_n + (size_t)row * o.KaP + c) = hn; }
      *reinterpret_cast<h2*>(o.Hc_tr + (size_t)row * o.KcP + c) = h2{(_Float16)(c < S ? sv.x : a0), (_Float16)(c + 1 < S ? sv.y : a1)};
      *reinterpret_cast<h2*>(o.Hc_pl + (size_t)row * o.KcP + c) = hs;
      *reinterpret_cast<h2*>(o.Hc_nx + (size_t)row * o.KcP + c) = hn;
    }
  }
  if (lane == 0) {
    o.reward[row] = R; o.mc[row] = ring.mc[slot];
    o.term[row] = tb ? 1.0f : 0.0f; o.idx[row] = li;
    a.disc[row] = nstep_discount(m, a.gamma); a.steps[row] = m;
  }
}

// ---- skinny head layers ------------------------------------------------------
// action_layer(4) + actionpara_layer(6) of the actor and q_values_layer(1) of
// the critic (src/dqn.cpp:426-427, 450) are K=H4 dot products per row: one wave
// per row, float4 strips over k, butterfly reduce.
// Tower-top reads of the head kernels.  fp32 learner: the fp32 activation panel.  fp16 learner: the fp16 panel the last
// tower layer's GEMM wrote for the next consumer anyway (x16 != null) — every other layer's input is the fp16-rounded
// activation already, and a separate fp32 copy of the tower top cost 16 MB of writes per forward pass + twice the bytes
// in every head kernel at 4096 rows.  The head arithmetic itself stays fp32.
typedef __attribute__((ext_vector_type(4))) _Float16 head_h4;
__device__ __forceinline__ f32x4 head_ld4(const float* x32, const _Float16* x16, size_t idx) {
  if (x16 != nullptr) {
    const head_h4 v = *reinterpret_cast<const head_h4*>(x16 + idx);
    return f32x4{(float)v.x, (float)v.y, (float)v.z, (float)v.w};
  }
  return *reinterpret_cast<const f32x4*>(x32 + idx);
}
__device__ __forceinline__ float head_ld1(const float* x32, const _Float16* x16, size_t idx) {
  return x16 != nullptr ? (float)x16[idx] : x32[idx];
}
// The same with the panel type fixed at compile time: the hot loops are instantiated once per type and entered through ONE
// branch (HEAD_DISPATCH), so that a per-load pointer test does not sit between the loads of a batch (measured on the fp32
// headline: k_head_q_train 4.9 -> 6.1 us with the test inside the loop).
template <bool IN16> __device__ __forceinline__ f32x4 head_ld4t(const float* x32, const _Float16* x16, size_t idx) {
  if constexpr (IN16) { const head_h4 v = *reinterpret_cast<const head_h4*>(x16 + idx); return f32x4{(float)v.x, (float)v.y, (float)v.z, (float)v.w}; }
  else return *reinterpret_cast<const f32x4*>(x32 + idx);
}
template <bool IN16> __device__ __forceinline__ float head_ld1t(const float* x32, const _Float16* x16, size_t idx) {
  if constexpr (IN16) return (float)x16[idx]; else return x32[idx];
}
#define HEAD_DISPATCH(is16, body) do { if (is16) body(std::true_type{}); else body(std::false_type{}); } while (0)

// ---- optimiser -----------------------------------------------------------------
// SGDSolver::ClipGradients + AdamSolver::ComputeUpdateValue + Net::Update +
// DQN::SoftUpdateNet in ONE pass over (w, g, m, v, w_target)
// (Caffe sgd_solver.cpp/adam_solver.cpp @2ef5847; src/dqn.cpp:
// 904, 964, 967-970, 1085-1096).  36 B/param of HBM traffic instead of Caffe's
// ~7 separate param-sized passes plus the separate soft-update pass.
// body shared by the stand-alone kernel and the mixed GEMM+Adam launch: block `blk` of
// `nblk` 256-thread blocks strides over the arena slice
// per-launch scalars of the optimiser pass into s[4..7]: clip scale, lr * Adam correction, soft-update
// switch, skip flag.  Every block re-derives them from the same partials in the same order.
// PRE: the caller guarantees corr_pre / soft_pre (inside an update) — the stand-alone path's two double pow() are not compiled in
// Dynamic loss scaling, once per net per update: the one place on the device that writes this net's multiplier (DevState::ls_mult has
// the readers — none of them in this launch; the update's later launches, and the next update's, read what is stored here across a
// kernel boundary).  Returns adam_scalars' s[7].  Out of line, so that the one-lane prologue of the optimiser kernels — whose register
// budget was tuned — stays the code it was: only a dynamic learner's block 0 makes the call.
// The reciprocal follows the multiplier by exact halving / doubling (growth below the cap is always x2: both are powers of two).
__device__ __noinline__ float loss_scale_update(DevState* st, int which, bool finite, LossScaleCfg cfg) {
  const float mult = st->ls_mult[which][0];
  const LossScaleStep r = loss_scale_step(LossScaleState{mult, st->ls_good[which]}, finite, cfg);
  if (r.backed_off) { st->ls_mult[which][0] = r.st.mult; st->ls_mult[which][1] *= 2.0f; st->ls_backoffs[which] += 1; }
  if (r.grew) { st->ls_mult[which][0] = r.st.mult; st->ls_mult[which][1] *= 0.5f; st->ls_growths[which] += 1; }
  st->ls_good[which] = r.st.good;
  if (finite) return 0.0f;
  atomicAdd(&st->skipped_steps, 1);
  if (r.raise_flag) atomicOr(&st->flags, kFlagGradNorm);
  return r.raise_flag ? 1.0f : 2.0f;
}
template <bool PRE = false>
__device__ __forceinline__ void adam_scalars(const AdamArgs& a, int blk, float* s /*>= 8 floats*/) {
  // every block re-derives the same global L2 norm from the partials, in the
  // same order -> bit-identical scale everywhere, no extra launch
  float acc = 0.0f;
  for (int i = threadIdx.x; i < a.n_partial; i += 256) acc += a.partial[i];
  acc = wave_sum64(acc);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
  __syncthreads();
  // one lane per block evaluates the per-launch scalars (two double pow() are ~500 instructions: run by
  // every thread they made this kernel VALU-bound: 733 VALU instructions per wave, 8 waves per SIMD)
  if (threadIdx.x == 0) {
    const float sumsq = (s[0] + s[1]) + (s[2] + s[3]);
    const float l2 = sqrtf(sumsq);
    s[4] = (a.clip >= 0.0f && l2 > a.clip) ? a.clip / l2 : 1.0f;
    if (PRE || a.corr_pre != nullptr) {                  // inside an update: both were left in DevState by its first launch
      s[5] = a.lr * *a.corr_pre;
      s[6] = *a.soft_pre ? 1.0f : 0.0f;
    } else {
      const int it_a = a.st->actor_iter, it_c = a.st->critic_iter;
      const int t = (a.which == 0 ? it_a : it_c) + 1;    // t = iter_ + 1 (before increment)
      s[5] = a.lr * adam_correction(a.beta1, a.beta2, t);
      // soft update condition uses max_iter() AFTER both increments (src/dqn.cpp:967)
      const int mx = (it_a + 1) > (it_c + 1) ? (it_a + 1) : (it_c + 1);
      s[6] = ((mx % a.soft_update_freq) == 0) ? 1.0f : 0.0f;
    }
    // A non-finite norm (fp16 mode: an overflowed dZ panel) would give scale = clip/inf = 0 and
    // g*0 = NaN in m, v, w and the targets for good.  Every block derives the same norm, so every
    // block takes the same decision: skip the whole step and raise the sticky flag.
    // s[7]: 0 take the step, 1 skip it and report (kFlagGradNorm), 2 skip it in silence (dynamic loss scaling backed off).  The
    // blocks other than the strided pass's first only tell zero from non-zero.
    const bool finite = isfinite(sumsq);
    s[7] = finite ? 0.0f : 1.0f;
    if (a.ls_dynamic && blk == 0) s[7] = loss_scale_update(a.st, a.which, finite, a.ls);
    else if (!finite && blk == 0) { atomicOr(&a.st->flags, kFlagGradNorm); atomicAdd(&a.st->skipped_steps, 1); }   // one launch per net per update
  }
  __syncthreads();
}
// one float4 of the optimiser step, in place (the strided pass and the first-layer riders share it: same expression, same bits)
__device__ __forceinline__ void adam_apply4(const AdamArgs& a, float scale, float step, bool soft, const f32x4& g, f32x4& m, f32x4& v, f32x4& w, f32x4& wt) {
  const float omb1 = 1.0f - a.beta1, omb2 = 1.0f - a.beta2;
  const float tau = a.tau, omt = 1 - a.tau;
  const float* gp = reinterpret_cast<const float*>(&g); float* mp = reinterpret_cast<float*>(&m);
  float* vp = reinterpret_cast<float*>(&v); float* wp = reinterpret_cast<float*>(&w);
  float* tp = reinterpret_cast<float*>(&wt);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float gi = gp[e] * scale;
    const float mi = fmaf(omb1, gi, a.beta1 * mp[e]);
    const float vi = fmaf(omb2, gi * gi, a.beta2 * vp[e]);
    const float upd = step * (mi / (sqrtf(vi) + a.eps));
    const float wi = wp[e] - upd;
    mp[e] = mi; vp[e] = vi; wp[e] = wi;
    if (soft) tp[e] = fmaf(tau, wi, omt * tp[e]);
  }
}
// ... and one element (a first-layer rider's bias: one per thread)
__device__ __forceinline__ void adam_apply1(const AdamArgs& a, float scale, float step, bool soft, float g, float& m, float& v, float& w, float& wt) {
  const float omb1 = 1.0f - a.beta1, omb2 = 1.0f - a.beta2;
  const float tau = a.tau, omt = 1 - a.tau;
  const float gi = g * scale;
  const float mi = fmaf(omb1, gi, a.beta1 * m);
  const float vi = fmaf(omb2, gi * gi, a.beta2 * v);
  const float upd = step * (mi / (sqrtf(vi) + a.eps));
  const float wi = w - upd;
  m = mi; v = vi; w = wi;
  if (soft) wt = fmaf(tau, wi, omt * wt);
}
// The optimiser launches that carry rider blocks: the block counts that route a workgroup (up to three) and what the strided pass's
// first loads need (the arena pointers and lengths) are requested in ONE round of scalar loads — the (empty) statement reads
// them and hands back the block index everything is routed by (request_args, gemm_bodies.hip.h, has the reasoning).  Left alone
// the compiler requests each rider's count only once the one before it has ruled the block out: up to four dependent rounds
// before a strided block's first load.
__device__ __forceinline__ int adam_routed_block(const AdamArgs& a, int b, int c0, int c1 = 0, int c2 = 0) {
  asm volatile("" : "+s"(b) : "s"(c0), "s"(c1), "s"(c2), "s"(a.w), "s"(a.wt), "s"(a.wt_sh), "s"(a.n4), "s"(a.partial));
  return b;
}
template <int U = 1, int NT = 0, bool PRE = false>
__device__ __forceinline__ void adam_soft_body(const AdamArgs& a, int blk, int nblk, float* s /*>= 8 floats*/) {
  // U float4 per array in flight per thread (U * 5 x 16-B loads before the first use); NT: the gradient is
  // read exactly once per update and never again -> non-temporal
  f32x4 g[U], m[U], v[U], w[U], wt[U];
  f32x4* wq[U]; f32x4* tq[U];
  auto load = [&](size_t i0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = i0 + (size_t)u * 256;
      if (i < a.n4) {
        wq[u] = reinterpret_cast<f32x4*>(i < a.n4_sh ? a.w_sh : a.w) + i;
        tq[u] = reinterpret_cast<f32x4*>(i < a.n4_sh ? a.wt_sh : a.wt) + i;
        g[u] = NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.g) + i) : reinterpret_cast<const f32x4*>(a.g)[i];
        m[u] = reinterpret_cast<const f32x4*>(a.m)[i];
        v[u] = reinterpret_cast<const f32x4*>(a.v)[i];
        w[u] = *wq[u];
        wt[u] = *tq[u];
      }
    }
  };
  // The first (for most threads: the only, or one of two) batch of loads goes out BEFORE the per-launch scalars are
  // derived: none of them depends on the clip scale, and the scalars' own chain (partials from the L2 of other XCDs ->
  // wave sums -> barrier -> sqrt / divide in one lane -> barrier) is ~1.5 us that every block would otherwise spend
  // with nothing in flight.
  size_t i0 = a.skip4 + (size_t)blk * (256 * U) + threadIdx.x;
  if (i0 < a.n4) load(i0);
  adam_scalars<PRE>(a, blk, s);
  if (s[7] != 0.0f) return;
  const float scale = s[4];
  const float step = s[5];
  const bool soft = s[6] != 0.0f;
  for (bool first = true; i0 < a.n4; i0 += (size_t)nblk * (256 * U), first = false) {
    if (!first) load(i0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = i0 + (size_t)u * 256;
      if (i >= a.n4) continue;
      adam_apply4(a, scale, step, soft, g[u], m[u], v[u], w[u], wt[u]);
      const float* wp = reinterpret_cast<const float*>(&w[u]); const float* tp = reinterpret_cast<const float*>(&wt[u]);
      reinterpret_cast<f32x4*>(a.m)[i] = m[u];
      reinterpret_cast<f32x4*>(a.v)[i] = v[u];
      *wq[u] = w[u];
      if (soft) *tq[u] = wt[u];
      if (a.w16 != nullptr) {
        typedef __attribute__((ext_vector_type(4))) _Float16 h16x4_t;
        reinterpret_cast<h16x4_t*>(a.w16)[i] = h16x4_t{(_Float16)wp[0], (_Float16)wp[1], (_Float16)wp[2], (_Float16)wp[3]};
        if (soft) reinterpret_cast<h16x4_t*>(a.wt16)[i] = h16x4_t{(_Float16)tp[0], (_Float16)tp[1], (_Float16)tp[2], (_Float16)tp[3]};
      }
    }
  }
}

// End of update: publish (critic_loss, avg_q), advance both solver iterations
// (Step's ++iter_, set_iter(iter+1): src/dqn.cpp:904, 965) and the sampling counter.
// avg_q = std::accumulate(q, 0.0) / float(B) (src/dqn.cpp:915-916): the double sum
// is taken from the per-block double partials when they are local (single GPU),
// from the all-reduced float tail under data parallelism.
// One block of 256 threads: strided partial sums, fixed butterfly + fixed cross-wave order.
// skipped_now: block 0 of this launch has just raised kFlagGradNorm (adam_scalars' s[7] == 1: a skipped step that is reported)
__device__ __forceinline__ void tick_body(const TickArgs& a, float* sdot /*[4]*/, double* sq /*[4]*/, bool skipped_now) {
  const int t = threadIdx.x;
  double qs = 0.0;
  if (a.q_partial != nullptr) {          // single GPU: reduce the per-block partials here
    float dot = 0.0f;
    for (int i = t; i < a.n_loss; i += 256) dot += a.loss_partial[i];
    for (int i = t; i < a.n_q; i += 256) qs += a.q_partial[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { dot += __shfl_xor(dot, off, 64); qs += __shfl_xor(qs, off, 64); }
    if ((t & 63) == 0) { sdot[t >> 6] = dot; sq[t >> 6] = qs; }
    __syncthreads();
    if (t == 0) {
      dot = (sdot[0] + sdot[1]) + (sdot[2] + sdot[3]);
      qs = (sq[0] + sq[1]) + (sq[2] + sq[3]);
      a.critic_tail[0] = dot / a.batch / 2.0f; a.actor_tail[1] = (float)qs;     // EuclideanLoss: dot / num / 2
    }
  } else qs = (double)a.actor_tail[1];   // data parallel: tails were all-reduced
  if (t != 0) return;
  if (a.q_partial == nullptr && a.critic_tail[2] != 0.0f) atomicOr(&a.st->flags, kFlagTarget);   // some rank's target was not finite
  a.st->critic_loss = a.critic_tail[0];
  a.st->avg_q = (float)(qs / (double)a.batch);
  a.st->actor_iter += 1; a.st->critic_iter += 1; a.st->update_counter += 1;
  if (a.host_stats != nullptr) {
    // the flags were raised with device-scope atomics (by earlier kernels of this update, or by block 0 of THIS launch —
    // whose atomic may still be in flight: this block derived the same skip decision itself); read them the same way
    int fl = __hip_atomic_load(&a.st->flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (skipped_now) fl |= kFlagGradNorm;
    a.host_stats[0] = a.critic_tail[0]; a.host_stats[1] = (float)(qs / (double)a.batch);
    a.host_stats[2] = __builtin_bit_cast(float, fl);
  }
}

// ---- first-layer riders of the optimiser launches (FirstLayerRider, ActorL0, PlainL0: learner_args.hip.h) ---------------------
// One step of a first-layer rider: the four 16-row tiles [t4, t4 + 4) of outputs [out0, out0 + 16) — fwd_direct_body's arithmetic,
// element for element (the reduction split over the four waves, its step order, (w0 + w1) + (w2 + w3)).  pw: this lane's weight
// fragments (row li of the 16, k = wave Kw + 16 kb + 4 lg; LDS or global); qf: the tiles' operands, requested earlier; the
// operands of step t4 + 4 are requested into qf behind the MFMAs; wave w reduces tile t4 + w.  bias16: the 16 outputs' biases
// (LDS or global; null: none).  One 16-KB parking area per workgroup (six workgroups per CU must keep fitting the LDS).
template <int G>
__device__ __forceinline__ void l0_step(const float* pw, const float* xq, int ldx, f32x4 (&qf)[4][G], int t4, int T, const float* bias16, bool relu,
                                        float* Y, int ldy, int out0, float* park, bool first) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
  f32x4 acc[4], pf[G];
#pragma unroll
  for (int kb = 0; kb < G; ++kb) pf[kb] = *reinterpret_cast<const f32x4*>(pw + kb * 16);      // (re-read per step: 8 VGPRs the 80-register budget does not have)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < G; ++kb)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[j] = DQN_MFMA(pf[kb][s], qf[j][kb][s], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int kb = 0; kb < G; ++kb)
      qf[j][kb] = *reinterpret_cast<const f32x4*>(xq + (size_t)(t4 + 4 + j < T ? t4 + 4 + j : T - 1) * 16 * ldx + kb * 16);   // (beyond the last tile: a valid row, unused)
  f32x4* pk = reinterpret_cast<f32x4*>(park);
  if (!first) __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) pk[(j * 4 + wave) * 64 + lane] = acc[j];
  __syncthreads();
  if (t4 + wave < T) {
    const f32x4* pj = pk + wave * 256;
    const f32x4 a0 = pj[lane], a1 = pj[64 + lane], a2 = pj[128 + lane], a3 = pj[192 + lane];
    f32x4 o;
    o.x = (a0.x + a1.x) + (a2.x + a3.x); o.y = (a0.y + a1.y) + (a2.y + a3.y);
    o.z = (a0.z + a1.z) + (a2.z + a3.z); o.w = (a0.w + a1.w) + (a2.w + a3.w);
    if (bias16 != nullptr) {
      const f32x4 bias = *reinterpret_cast<const f32x4*>(bias16 + lg * 4);
      o.x += bias.x; o.y += bias.y; o.z += bias.z; o.w += bias.w;
    }
    if (relu) { o.x = lrelu_fwd(o.x); o.y = lrelu_fwd(o.y); o.z = lrelu_fwd(o.z); o.w = lrelu_fwd(o.w); }
    *reinterpret_cast<f32x4*>(Y + (size_t)((t4 + wave) * 16 + li) * ldy + out0 + (lg << 2)) = o;
  }
}
template <int G>
struct FirstLayerWork {
  const AdamArgs& a; const FirstLayerRider& r; const int blk; float* sW; float* sB; float* park;
  __device__ __forceinline__ FirstLayerWork(const AdamArgs& a_, const FirstLayerRider& r_, int blk_, float* sW_, float* sB_, float* park_)
      : a(a_), r(r_), blk(blk_), sW(sW_), sB(sB_), park(park_) {}
  static constexpr int NH = G == 1 ? 4 : 0;    // (G = 2: the step's own operands are 45 of the 80 registers)
  f32x4 g[G], m[G], v[G], w[G], wt[G], qf[4][G];
  float bg, bm, bv, bw, bwt;
  __device__ __forceinline__ size_t widx(int u) const { return ((size_t)blk * G + u) * 256 + threadIdx.x; }
  __device__ __forceinline__ size_t bidx() const { return (size_t)r.N * r.Kp + (size_t)blk * 16 + threadIdx.x; }
  // everything the step on this workgroup's slice reads, requested in ONE round trip before the launch's scalars are derived
  // (the memory system is saturated by the strided pass beside it: every dependent round trip costs ~3 us here)
  __device__ __forceinline__ void request() {
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const size_t i = widx(u);
      g[u] = reinterpret_cast<const f32x4*>(a.g)[i]; m[u] = reinterpret_cast<const f32x4*>(a.m)[i];
      v[u] = reinterpret_cast<const f32x4*>(a.v)[i]; w[u] = reinterpret_cast<const f32x4*>(a.w)[i]; wt[u] = reinterpret_cast<const f32x4*>(a.wt)[i];
    }
    if (threadIdx.x < 16) { const size_t i = bidx(); bg = a.g[i]; bm = a.m[i]; bv = a.v[i]; bw = a.w[i]; bwt = a.wt[i]; }
    // ... and the first row tiles' operands of the layer (as many as the 80-register budget holds beside the step's operands)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int T = r.rows >> 4;
    const float* xq = r.X + (size_t)li * r.ldx + wave * (r.Kp >> 2) + lg * 4;
#pragma unroll
    for (int j = 0; j < NH; ++j)
#pragma unroll
      for (int kb = 0; kb < G; ++kb) qf[j][kb] = *reinterpret_cast<const f32x4*>(xq + (size_t)(j < T ? j : T - 1) * 16 * r.ldx + kb * 16);
  }
  __device__ __forceinline__ void run(float scale, float step, bool soft, bool apply) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int Kw = r.Kp >> 2, T = r.rows >> 4;
    if (apply) {
#pragma unroll
      for (int u = 0; u < G; ++u) adam_apply4(a, scale, step, soft, g[u], m[u], v[u], w[u], wt[u]);
      if (threadIdx.x < 16) adam_apply1(a, scale, step, soft, bg, bm, bv, bw, bwt);
    }
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const size_t i = widx(u);
      if (apply) {
        reinterpret_cast<f32x4*>(a.m)[i] = m[u]; reinterpret_cast<f32x4*>(a.v)[i] = v[u]; reinterpret_cast<f32x4*>(a.w)[i] = w[u];
        if (soft) reinterpret_cast<f32x4*>(a.wt)[i] = wt[u];
      }
      reinterpret_cast<f32x4*>(sW)[u * 256 + threadIdx.x] = w[u];
    }
    if (threadIdx.x < 16) {
      const size_t i = bidx();
      if (apply) { a.m[i] = bm; a.v[i] = bv; a.w[i] = bw; if (soft) a.wt[i] = bwt; }
      sB[threadIdx.x] = bw;
    }
    const float* xq = r.X + (size_t)li * r.ldx + wave * Kw + lg * 4;
#pragma unroll
    for (int j = NH; j < 4; ++j)          // (the rest of the first group: behind the step's stores, whose registers they take over)
#pragma unroll
      for (int kb = 0; kb < G; ++kb) qf[j][kb] = *reinterpret_cast<const f32x4*>(xq + (size_t)(j < T ? j : T - 1) * 16 * r.ldx + kb * 16);
    __syncthreads();
    // the layer: outputs [16 blk, +16) x every row, four row tiles per step (l0_step)
    const float* pw = sW + li * r.Kp + wave * Kw + lg * 4;
    for (int t4 = 0; t4 < T; t4 += 4) l0_step<G>(pw, xq, r.ldx, qf, t4, T, sB, true, r.Y, r.ldy, blk * 16, park, t4 == 0);
  }
};
struct ActorL0Work {
  const AdamArgs& a; const ActorL0& r; const int blk; float* sW; float* sB; float* park;
  __device__ __forceinline__ ActorL0Work(const AdamArgs& a_, const ActorL0& r_, int blk_, float* sW_, float* sB_, float* park_)
      : a(a_), r(r_), blk(blk_), sW(sW_), sB(sB_), park(park_) {}
  f32x4 g, m, v, w, wt, qs[4][1], qn[4][1];
  float bg, bm, bv, bw, bwt;
  __device__ __forceinline__ size_t widx() const { return (size_t)blk * 256 + threadIdx.x; }
  __device__ __forceinline__ size_t bidx() const { return (size_t)r.N * 64 + (size_t)blk * 16 + threadIdx.x; }
  __device__ __forceinline__ void request() {
    const size_t i = widx();
    g = reinterpret_cast<const f32x4*>(a.g)[i]; m = reinterpret_cast<const f32x4*>(a.m)[i];
    v = reinterpret_cast<const f32x4*>(a.v)[i]; w = reinterpret_cast<const f32x4*>(a.w)[i]; wt = reinterpret_cast<const f32x4*>(a.wt)[i];
    if (threadIdx.x < 16) { const size_t j = bidx(); bg = a.g[j]; bm = a.m[j]; bv = a.v[j]; bw = a.w[j]; bwt = a.wt[j]; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int T = r.rows >> 4;
    const size_t x0 = (size_t)li * r.ldx + wave * 16 + lg * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t x = x0 + (size_t)(j < T ? j : T - 1) * 16 * r.ldx;
      qs[j][0] = *reinterpret_cast<const f32x4*>(r.Xs + x);
    }
  }
  __device__ __forceinline__ void run(float scale, float step, bool soft, bool apply) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const int T = r.rows >> 4;
    if (apply) {
      adam_apply4(a, scale, step, soft, g, m, v, w, wt);
      if (threadIdx.x < 16) adam_apply1(a, scale, step, soft, bg, bm, bv, bw, bwt);
      const size_t i = widx();
      reinterpret_cast<f32x4*>(a.m)[i] = m; reinterpret_cast<f32x4*>(a.v)[i] = v; reinterpret_cast<f32x4*>(a.w)[i] = w;
      if (soft) reinterpret_cast<f32x4*>(a.wt)[i] = wt;
      if (threadIdx.x < 16) { const size_t j = bidx(); a.m[j] = bm; a.v[j] = bv; a.w[j] = bw; if (soft) a.wt[j] = bwt; }
    }
    reinterpret_cast<f32x4*>(sW)[threadIdx.x] = w; reinterpret_cast<f32x4*>(sW)[256 + threadIdx.x] = wt;
    if (threadIdx.x < 16) { sB[threadIdx.x] = bw; sB[16 + threadIdx.x] = bwt; }
    const float* xs = r.Xs + (size_t)li * r.ldx + wave * 16 + lg * 4;
    const float* xn = r.Xn + (size_t)li * r.ldx + wave * 16 + lg * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) qn[j][0] = *reinterpret_cast<const f32x4*>(xn + (size_t)(j < T ? j : T - 1) * 16 * r.ldx);   // (behind the step's stores, whose registers they take over)
    __syncthreads();
    const float* pw = sW + li * 64 + wave * 16 + lg * 4;
    for (int t4 = 0; t4 < T; t4 += 4) {      // the two nets take turns: each one's next operands are in flight under the other's step
      l0_step<1>(pw, xs, r.ldx, qs, t4, T, sB, true, r.Ys, r.ldy, blk * 16, park, t4 == 0);
      l0_step<1>(pw + 16 * 64, xn, r.ldx, qn, t4, T, sB + 16, true, r.Yn, r.ldy, blk * 16, park, false);
    }
  }
};
template <int G>
__device__ __forceinline__ void plain_l0_run(const PlainL0& p, int blk, float* park) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
  const int Kw = 16 * G, T = p.rows >> 4;
  const float* xq = p.X + (size_t)li * p.ldx + wave * Kw + lg * 4;
  f32x4 qf[4][G];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int kb = 0; kb < G; ++kb) qf[j][kb] = *reinterpret_cast<const f32x4*>(xq + (size_t)(j < T ? j : T - 1) * 16 * p.ldx + kb * 16);
  if (p.xcopy_dst != nullptr && threadIdx.x < 16) {
    const float* src = p.W + (size_t)(blk * 16 + threadIdx.x) * p.ldw + p.xcopy_col;
    for (int j = 0; j < p.xcopy_n; ++j) p.xcopy_dst[(size_t)j * p.N + blk * 16 + threadIdx.x] = src[j];
  }
  const float* pw = p.W + (size_t)(blk * 16 + li) * p.ldw + wave * Kw + lg * 4;
  const float* b16 = p.bias != nullptr ? p.bias + blk * 16 : nullptr;
  for (int t4 = 0; t4 < T; t4 += 4) l0_step<G>(pw, xq, p.ldx, qf, t4, T, b16, p.bias != nullptr, p.Y, p.ldy, blk * 16, park, t4 == 0);
}

}  // namespace dqnhip
