// per_kernels.hip.h — proportional prioritized replay (Schaul et al. 2016), the replay-side kernels: a radix-64 sum tree over the
// PHYSICAL slots of the ring, its reconciliation with the ring (k_per_sync), the stratified sampler (k_per_sample), the fill for
// explicit indices (k_per_fill) and the write-back (k_per_update).  Launched by learner_per.hip.  (Kernels are static: a unit that
// includes this embeds all of them.)  The weighted critic loss is k_head_q_train_w, head_kernels.hip.h.
//
// THE TREE.  Level 0 holds one float32 leaf per physical slot, padded with zeros to a multiple of 64; level k + 1 holds one node per
// 64 children of level k, padded with zeros to a multiple of 64 as well; the last level's node 0 is the root, `total`.  A leaf is the
// already exponentiated priority p^alpha: 0 outside the logical window [head, head + size), PerDev::p_max for a transition that was
// never sampled.  Physical slots do not move while ring_head does, so FIFO eviction only zeroes leaves.
//
// A NODE is the float32 sum of its 64 children c[0 .. 63] in ONE order, the halving tree
//     v32[i] = c[i] + c[i + 32]   (i < 32),   v16[i] = v32[i] + v32[i + 16],   v8, v4, v2 likewise,   node = v2[0] + v2[1]
// whoever computes it: a wave (node_sum_wave: one coalesced 256-B load, six __shfl_xor steps with offsets 32, 16, 8, 4, 2, 1 — lane i
// adds the value of lane i ^ off, and float addition commutes, so every lane ends with the tree's value) or one thread
// (node_sum_thread: the same pairs from registers).  Nodes are always recomputed from their children, never adjusted by a delta: the
// tree cannot drift, and tests/per_ref.py recomputes every level from the leaves bit for bit.
//
// THE DRAW of minibatch row j of B, on Philox counter c (DevState::update_counter of the update, or the caller's):
//     r_j = (float)(philox_u32(per_seed, c, j) >> 8) * 2^-24            in [0, 1), exact
//     u_j = (((float)j + r_j) * inv_B) * total                           three float32 operations, in this order; inv_B = 1.0f / (float)B
// then from the root down, per level, with c[lane] the node's 64 children:
//     p = c;  for off in 1, 2, 4, 8, 16, 32:  t = __shfl_up(p, off);  if (lane >= off) p = p + t        (inclusive Hillis-Steele scan)
//     child = the first lane with p > u and c > 0; if there is none (rounding), the last lane with c > 0
//     u = u - (child > 0 ? p[child - 1] : 0)
// (c > 0 in the first rule: the scan sums every lane's prefix in its own association, so p[i] may exceed p[i - 1] by a rounding although
// c[i] is zero — a zero-priority slot is never returned.)  The slot reached at level 0 is written as the LOGICAL index
// (slot - head + cap) % cap into the buffer the gather reads, with slot[j] and prob[j] = leaf / total (correctly rounded division).
#pragma once
#include "update_bodies.hip.h"     // philox_u32; Ring, DevState (learner_args.hip.h)

namespace dqnhip {

constexpr int kPerMaxLevels = 8;
struct PerTree {
  float* lvl[kPerMaxLevels];       // lvl[0]: leaves ... lvl[levels]: the root's level (64 floats, node 0 = total)
  int n[kPerMaxLevels];            // real nodes per level: n[0] = cap, n[k + 1] = ceil(n[k] / 64), n[levels] = 1
  int levels;                      // levels above the leaves (>= 1)
};
// device-resident scalars of the priority structure
struct PerDev {
  float p_max;                     // the largest leaf ever written (initially 1): what a new transition gets
  int head_seen, size_seen;        // (ring_head, ring_size) as the last k_per_sync left the tree
  int done;                        // arrival counter of k_per_sync, zero between launches
};

__device__ __forceinline__ float node_sum_wave(float c) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c = c + __shfl_xor(c, off, 64);
  return c;
}
__device__ __forceinline__ float node_sum_thread(const float* __restrict__ c) {
  float v[64];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const f32x4 t = reinterpret_cast<const f32x4*>(c)[i];
    v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
#pragma unroll
    for (int i = 0; i < w; ++i) v[i] = v[i] + v[i + w];
  }
  return v[0];
}
// levels first .. t.levels, every real node, by the threads of ONE workgroup (thread per node); the children must be visible
__device__ __forceinline__ void per_upper_levels(const PerTree& t, int first) {
  for (int k = first; k <= t.levels; ++k) {
    for (int i = threadIdx.x; i < t.n[k]; i += blockDim.x) t.lvl[k][i] = node_sum_thread(t.lvl[k - 1] + (size_t)i * 64);
    __threadfence();
    __syncthreads();
  }
}

// ---- k_per_sync: the tree follows the ring ------------------------------------------------------------------------------------
// From (head, size) now and as seen last: e = (head - head_seen) mod cap transitions were evicted, n = size - size_seen + e
// appended (unambiguous while fewer than cap were appended in between: the host enqueues a sync before its upper bound gets there).
// A physical slot's leaf becomes 0 outside the new window, p_max among the window's n newest, and stays otherwise.  The slots whose
// leaf may change are the e oldest of the old window and the n newest of the new one: up to four runs of consecutive slots; the
// waves of the grid stride over the level-1 nodes above those runs (a node above two runs is computed twice, to the same bits), and
// the last block to finish (done counter + __threadfence, as k_add_transitions) recomputes every node of the levels above.
// set mode (src != null; dqnhip_per_set_priorities, the tree in sync): the logical range [first, first + n_set) takes src[], p_max
// rises to the largest of them, nothing else changes.
struct PerSyncArgs {
  PerTree t; PerDev* pd; const DevState* rs; int cap;
  const float* src; int first, n_set;
};
static __global__ __launch_bounds__(256) void k_per_sync(PerSyncArgs a) {
  const int cap = a.cap;
  const int head = a.rs->ring_head, size = a.rs->ring_size;
  const int hs = a.pd->head_seen, ss = a.pd->size_seen;
  const float pmax = a.pd->p_max;
  const bool set = a.src != nullptr;
  const int e = set ? 0 : (head - hs + cap) % cap;
  int n = set ? a.n_set : size - ss + e;
  n = n < 0 ? 0 : (n > cap ? cap : n);                    // (whatever the counters hold, the runs below stay inside the ring)
  // the runs [lo, hi) of physical slots, none wrapping
  int lo[4], hi[4];
  const int z0 = hs, z1 = hs + e;                                                  // evicted
  lo[0] = z0; hi[0] = z1 < cap ? z1 : cap; lo[1] = 0; hi[1] = z1 > cap ? z1 - cap : 0;
  const int s0 = (int)(((long long)head + (set ? a.first : size - n)) % cap), s1 = s0 + n;   // appended (set mode: the range)
  lo[2] = s0; hi[2] = s1 < cap ? s1 : cap; lo[3] = 0; hi[3] = s1 > cap ? s1 - cap : 0;
  int cnt[4], total = 0;
  for (int r = 0; r < 4; ++r) { cnt[r] = hi[r] > lo[r] ? (hi[r] - 1) / 64 - lo[r] / 64 + 1 : 0; total += cnt[r]; }
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), waves = gridDim.x * 4;
  float seen_max = 0.0f;
  for (int j = wave; j < total; j += waves) {
    int r = 0, k = j;
    while (k >= cnt[r]) { k -= cnt[r]; ++r; }
    const int node = lo[r] / 64 + k;
    const int slot = node * 64 + lane;                   // (< n[0] rounded up to 64: inside the padded level)
    float c = a.t.lvl[0][slot];
    if (slot < cap) {
      const int li = (slot - head + cap) % cap;          // logical index in the new window (>= size: outside)
      float v = c;
      if (set) { if (li >= a.first && li < a.first + n) v = a.src[li - a.first]; }
      else if (li >= size) v = 0.0f;
      else if (li >= size - n) v = pmax;
      if (__builtin_bit_cast(unsigned, v) != __builtin_bit_cast(unsigned, c)) a.t.lvl[0][slot] = v;
      if (set && li >= a.first && li < a.first + n) seen_max = fmaxf(seen_max, v);
      c = v;
    }
    const float s = node_sum_wave(c);
    if (lane == 0) a.t.lvl[1][node] = s;
  }
  if (set) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) seen_max = fmaxf(seen_max, __shfl_xor(seen_max, off, 64));
    // (non-negative floats order as their bit patterns)
    if (lane == 0 && seen_max > pmax) atomicMax(reinterpret_cast<unsigned*>(&a.pd->p_max), __builtin_bit_cast(unsigned, seen_max));
  }
  __shared__ int s_last;
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    s_last = atomicAdd(&a.pd->done, 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();                                       // the other blocks' level-1 nodes
  if (a.t.levels >= 2) per_upper_levels(a.t, 2);
  if (threadIdx.x == 0) {
    if (!set) { a.pd->head_seen = head; a.pd->size_seen = size; }
    a.pd->done = 0;
  }
}

// ---- k_per_sample: one wave per minibatch row, four rows per block (as k_gather); blockIdx.y: the minibatch of a sample-only call ----
struct PerSampleArgs {
  PerTree t; const DevState* rs; const DevState* st; int cap, B; float inv_B; uint64_t seed;
  int live; unsigned long long counter;      // live: the counter is st->update_counter (inside an update); else counter + blockIdx.y
  int* idx; int* slot; float* prob; float* u;      // [gridDim.y][B] each (u may be null)
};
static __global__ __launch_bounds__(256) void k_per_sample(PerSampleArgs a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.B) return;
  const unsigned long long ctr = a.live ? a.st->update_counter : a.counter + blockIdx.y;
  const float total = a.t.lvl[a.t.levels][0];
  const float r = (float)(philox_u32(a.seed, ctr, (uint32_t)row) >> 8) * (1.0f / 16777216.0f);
  float u = (float)row + r;
  u = u * a.inv_B;
  u = u * total;
  const float u0 = u;
  int node = 0;
  float c = 0.0f;
  for (int k = a.t.levels - 1; k >= 0; --k) {
    c = a.t.lvl[k][(size_t)node * 64 + lane];
    float p = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const float t = __shfl_up(p, off, 64); if (lane >= off) p = p + t; }
    const unsigned long long nz = __ballot(c > 0.0f);
    const unsigned long long hit = __ballot(p > u && c > 0.0f);
    // (nz == 0 cannot be reached below a node > 0: a sum of non-negative floats is 0 only if all are; an empty tree is refused by the host)
    const int child = hit ? __ffsll((long long)hit) - 1 : (nz ? 63 - __clzll((long long)nz) : 0);
    const float before = __shfl(p, child > 0 ? child - 1 : 0, 64);
    if (child > 0) u = u - before;
    c = __shfl(c, child, 64);
    node = node * 64 + child;
  }
  if (lane == 0) {
    const size_t o = (size_t)blockIdx.y * a.B + row;
    const int sl = node < a.cap ? node : a.cap - 1;      // (the padding is zero and never chosen; the clamp guards the ring reads)
    a.idx[o] = (sl - a.rs->ring_head + a.cap) % a.cap;
    a.slot[o] = sl;
    a.prob[o] = __fdiv_rn(c, total);
    if (a.u != nullptr) a.u[o] = u0;
  }
}

// ---- k_per_fill: explicit indices — slot / prob of the given rows from their leaves ------------------------------------------------
static __global__ void k_per_fill(PerTree t, const DevState* rs, int cap, int B, const int* __restrict__ idx, int* slot, float* prob) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= B) return;
  const int size = rs->ring_size;
  int li = idx[row];
  li = li < 0 ? 0 : (li >= size ? size - 1 : li);        // (the gather's clamp)
  li = li < 0 ? 0 : li;
  const int sl = (int)(((long long)rs->ring_head + li) % cap);
  slot[row] = sl;
  prob[row] = __fdiv_rn(t.lvl[0][sl], t.lvl[t.levels][0]);
}

// ---- k_per_update: the write-back, after the update's last launch -------------------------------------------------------------------
// leaf[slot_row] = (td_abs_row + eps)^alpha (duplicate rows of one transition carry the same |TD error|, hence the same value; a
// non-finite td_abs leaves the old leaf in place), p_max = max(p_max, new leaf) by an atomic max on the bits of a non-negative float,
// then the touched parents level by level.  ONE workgroup, not the last-block pattern: the work is B leaves and B nodes of 256 B per
// level, the levels depend on each other, and inside one workgroup a barrier orders them — a grid would need one arrival counter per
// level for nothing to do in parallel.  Thread per row and level: node_sum_thread, the tree's one order.
struct PerUpdateArgs { PerTree t; PerDev* pd; int B; const int* slot; const float* td_abs; float eps, alpha; };
static __global__ __launch_bounds__(256) void k_per_update(PerUpdateArgs a) {
  for (int row = threadIdx.x; row < a.B; row += blockDim.x) {
    const float td = a.td_abs[row];
    if (!isfinite(td)) continue;
    const float v = a.alpha == 0.0f ? 1.0f : powf(td + a.eps, a.alpha);
    if (!isfinite(v)) continue;
    a.t.lvl[0][a.slot[row]] = v;
    atomicMax(reinterpret_cast<unsigned*>(&a.pd->p_max), __builtin_bit_cast(unsigned, v));
  }
  __threadfence();
  __syncthreads();
  long long div = 64;                                    // slots per node of level k
  for (int k = 1; k <= a.t.levels; ++k, div *= 64) {
    for (int row = threadIdx.x; row < a.B; row += blockDim.x) {
      const int node = (int)(a.slot[row] / div);
      a.t.lvl[k][node] = node_sum_thread(a.t.lvl[k - 1] + (size_t)node * 64);
    }
    __threadfence();
    __syncthreads();
  }
}

}  // namespace dqnhip
