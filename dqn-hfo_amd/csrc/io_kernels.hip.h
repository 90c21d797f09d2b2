// io_kernels.hip.h — the kernels learner_io.hip launches: replay-ring I/O, the acting-time pack / unpack helpers, the local
// gradient reduction.  (Kernels are static: a unit that includes this embeds all of them.)
#pragma once
#include "update_bodies.hip.h"

namespace dqnhip {

// ---- replay ring (Ring: learner_args.hip.h) -------------------------------------
// DQN::AddTransitions / AddTransition (src/dqn.cpp:768-781): the eviction
// arithmetic runs on one thread and publishes (head,size); rows are scattered
// by the rest of the grid from the values BEFORE the update (old_head/old_size
// are recomputed identically by every block).
static __global__ void k_add_transitions(Ring ring, DevState* st, const float* __restrict__ s,
                                  const float* __restrict__ a, const float* __restrict__ r,
                                  const float* __restrict__ mc, const float* __restrict__ nx,
                                  const uint8_t* __restrict__ term, int n, int single_mode,
                                  int* done_counter) {
  // every block derives the same post-eviction (head,size)
  int head = st->ring_head, size = st->ring_size;
  if (single_mode == 2) {      // LoadReplayMemory: plain append, no eviction (caller checked the capacity)
  } else if (single_mode) {    // AddTransition: pop iff size == capacity
    if (size == ring.cap) { head = (head + 1) % ring.cap; size -= 1; }
  } else {                     // AddTransitions: while (size + n >= capacity) pop_front
    int pops = size + n - ring.cap + 1;
    if (pops < 0) pops = 0;
    if (pops > size) pops = size;
    head = (int)(((long long)head + pops) % ring.cap); size -= pops;
  }
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row < n) {
    const long long slot = ((long long)head + size + row) % ring.cap;
    const uint8_t t = term[row];
    for (int c = lane; c < ring.SP; c += 64) {
      ring.state[slot * ring.SP + c] = c < ring.S ? s[(size_t)row * ring.S + c] : 0.0f;
      ring.next[slot * ring.SP + c] = (c < ring.S && !t && nx != nullptr) ? nx[(size_t)row * ring.S + c] : 0.0f;
    }
    if (lane < kAP) ring.act[slot * kAP + lane] = lane < kNO ? a[(size_t)row * kNO + lane] : 0.0f;
    if (lane == 0) { ring.reward[slot] = r[row]; ring.mc[slot] = mc[row]; ring.term[slot] = t ? 1 : 0; }
  }
  // last block to finish publishes the new (head,size)
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    const int prev = atomicAdd(done_counter, 1);
    if (prev == (int)gridDim.x - 1) {
      st->ring_head = head; st->ring_size = size + n; *done_counter = 0;
      __threadfence();
    }
  }
}

static __global__ void k_read_memory(Ring ring, const DevState* st, int first, int n, float* s, float* a,
                              float* r, float* mc, float* nx, uint8_t* term) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const long long slot = ((long long)st->ring_head + first + row) % ring.cap;
  for (int c = lane; c < ring.S; c += 64) {
    if (s) s[(size_t)row * ring.S + c] = ring.state[slot * ring.SP + c];
    if (nx) nx[(size_t)row * ring.S + c] = ring.next[slot * ring.SP + c];
  }
  if (a && lane < kNO) a[(size_t)row * kNO + lane] = ring.act[slot * kAP + lane];
  if (lane == 0) {
    if (r) r[row] = ring.reward[slot];
    if (mc) mc[row] = ring.mc[slot];
    if (term) term[row] = ring.term[slot];
  }
}

// DQN::SampleStatesFromMemory (src/dqn.cpp:511-523): one wave per sampled transition, dense [n][S] out
static __global__ void k_sample_states(Ring ring, const DevState* rs, const int* __restrict__ idx_in, uint64_t key,
                                unsigned long long counter, int n, float* __restrict__ out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const int size = rs->ring_size;
  int li = idx_in ? idx_in[row] : (int)(((uint64_t)philox_u32(key, counter, (uint32_t)row) * (uint64_t)size) >> 32);
  li = li < 0 ? 0 : (li >= size ? size - 1 : li);
  const long long slot = ((long long)rs->ring_head + li) % ring.cap;
  for (int c = lane; c < ring.S; c += 64) out[(size_t)row * ring.S + c] = ring.state[slot * ring.SP + c];
}

// dqnhip_nstep_validate: the invariant n-step windows stand on — a non-terminal transition's stored next state IS the state of its
// logical successor, bit for bit over the S floats.  One wave per transition of [first, first + n), waves striding over the range; the
// ring's last transition has no successor and is exempt.  Each block folds its waves' count and smallest offending logical index in
// LDS and adds them to the two result words with one integer atomic each: whatever the order, the same two numbers.
static __global__ __launch_bounds__(256) void k_nstep_validate(NstepValidateArgs a) {
  __shared__ int s_cnt[4], s_min[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const Ring& ring = a.ring;
  const int size = a.rs->ring_size;
  const long long head = a.rs->ring_head;
  int cnt = 0, mn = 0x7FFFFFFF;
  for (long long i = (long long)blockIdx.x * 4 + wave; i < a.n; i += (long long)gridDim.x * 4) {
    const long long li = (long long)a.first + i;
    if (li >= size - 1) continue;                                  // (wave-uniform) the last transition, or beyond the memory
    const long long slot = (head + li) % ring.cap, succ = (head + li + 1) % ring.cap;
    if (ring.term[slot]) continue;
    const uint32_t* nx = reinterpret_cast<const uint32_t*>(ring.next + slot * ring.SP);
    const uint32_t* sn = reinterpret_cast<const uint32_t*>(ring.state + succ * ring.SP);
    bool bad = false;
    for (int c = lane; c < ring.S; c += 64) bad |= nx[c] != sn[c];
    if (__ballot(bad)) { cnt += 1; mn = mn < (int)li ? mn : (int)li; }
  }
  if (lane == 0) { s_cnt[wave] = cnt; s_min[wave] = mn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    const int m01 = s_min[0] < s_min[1] ? s_min[0] : s_min[1], m23 = s_min[2] < s_min[3] ? s_min[2] : s_min[3];
    if (c) { atomicAdd(a.violations, (unsigned long long)c); atomicMin(a.first_bad, m01 < m23 ? m01 : m23); }
  }
}

// ---- acting-time helpers ---------------------------------------------------------
// dense [n][S] -> padded panel [npad][SP] (pad rows/cols zero)
static __global__ void k_pack_rows(const float* __restrict__ src, int n, int S, float* __restrict__ dst,
                            int npad, int SP) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npad * SP) return;
  const int r = i / SP, c = i % SP;
  dst[i] = (r < n && c < S) ? src[(size_t)r * S + c] : 0.0f;
}
// critic input panel from dense states + dense actor outputs
static __global__ void k_pack_critic(const float* __restrict__ s, const float* __restrict__ a, int n, int S,
                              float* __restrict__ dst, int npad, int KP) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npad * KP) return;
  const int r = i / KP, c = i % KP;
  float v = 0.0f;
  if (r < n) { if (c < S) v = s[(size_t)r * S + c]; else if (c < S + kNO) v = a[(size_t)r * kNO + (c - S)]; }
  dst[i] = v;
}
// fp16 acting (dqnhip_set_act_precision): the same two panels in fp16, rounded to nearest even, [rows][k16] with k16 % 128 == 0.
// One wave per row piece of 512 columns, a lane converts 8 consecutive columns and writes them with one 16-byte store.  Pad rows
// (>= n) and pad columns are written as zero on EVERY call: the panel is reused between actor and critic passes of different
// widths, and a stale Inf / NaN in a pad column times a zero weight is NaN.
typedef __attribute__((ext_vector_type(8))) _Float16 pack_h8;
// src: [n][ld_src] fp32, the first S columns of a row are the state; act (k_pack_critic16): dense actor outputs [n][10]
struct Pack16Args { const float* src; const float* act; int n, S, ld_src; _Float16* dst; int rows, k16; };
static __global__ __launch_bounds__(256) void k_pack_rows16(const Pack16Args p) {
  const int ppr = (p.k16 + 511) / 512;                 // row pieces per row
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = gw / ppr, c = (gw % ppr) * 512 + lane * 8;
  if (r >= p.rows || c >= p.k16) return;               // (k16 % 8 == 0: c < k16 means the whole piece is inside the row)
  pack_h8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (_Float16)((r < p.n && c + e < p.S) ? p.src[(size_t)r * p.ld_src + c + e] : 0.0f);
  *reinterpret_cast<pack_h8*>(p.dst + (size_t)r * p.k16 + c) = v;
}
// critic input panel [s | a | p] from dense states [n][S] (ld_src == S) + dense actor outputs
static __global__ __launch_bounds__(256) void k_pack_critic16(const Pack16Args p) {
  const int ppr = (p.k16 + 511) / 512;
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = gw / ppr, c = (gw % ppr) * 512 + lane * 8;
  if (r >= p.rows || c >= p.k16) return;
  pack_h8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int col = c + e;
    float x = 0.0f;
    if (r < p.n) { if (col < p.S) x = p.src[(size_t)r * p.ld_src + col]; else if (col < p.S + kNO) x = p.act[(size_t)r * kNO + (col - p.S)]; }
    v[e] = (_Float16)x;
  }
  *reinterpret_cast<pack_h8*>(p.dst + (size_t)r * p.k16 + c) = v;
}
static __global__ void k_unpack_out(const float* __restrict__ out16, int n, float* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * kNO) return;
  dst[i] = out16[(size_t)(i / kNO) * kAP + (i % kNO)];
}

// Sum of up to 8 co-located gradient arenas in rank order, written back to all (dqnhip_reduce_gradients_local)
static __global__ __launch_bounds__(256) void k_local_reduce(LocalReduce a) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.n4; i += (size_t)gridDim.x * 256) {
    f32x4 s = reinterpret_cast<const f32x4*>(a.g[0])[i];
    for (int r = 1; r < a.n; ++r) { const f32x4 v = reinterpret_cast<const f32x4*>(a.g[r])[i]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
    for (int r = 0; r < a.n; ++r) reinterpret_cast<f32x4*>(a.g[r])[i] = s;
  }
}

}  // namespace dqnhip
