// state_kernels.hip.h — the device side of the asynchronous learner-state save (dqnhip_save_state_async, include/dqnhip.h):
// one pass on the learner's stream freezes the file's sections, as their final bytes, in a staging buffer and checksums them there.
// Included and launched by learner_save_async.hip only; a learner that never saves asynchronously launches none of this.  The kernels READ
// the learner and write nothing but the staging buffer.  state_image.h has the structures and the CRC bodies (host and device).
//
//   k_state_pack_params  grid (x, segments + 1): slice y < segments moves one strided piece of a parameter arena (a layer's weights
//                        without their pad columns, a bias vector, a head's rows) into the dense Caffe order of dqnhip_get_params;
//                        the last slice's first thread captures the record (StateRec) from DevState and the priority tree's p_max
//   k_state_pack_ring    grid (ceil(cap / kPackRows), arrays): (ring_head, ring_size) are read from DevState here, on the device — the
//                        host's mirrors may be stale; a block owns kPackRows logical rows of one array, blocks beyond ring_size exit
//   k_state_crc          one thread per kCrcChunk bytes of every section, slice-by-4 tables built in LDS: raw() of the chunk
// 16-byte loads where width, pitch and both addresses allow (PackSeg::vec / RingArr::vec, decided on the host), 4-byte (term: 1-byte)
// elements otherwise; the stores are plain vector stores.  No atomics, no floating-point arithmetic: a copy and an integer reduction.
#pragma once
#include "learner_args.hip.h"       // DevState
#include "state_image.h"

namespace dqnhip {

using dqnhip_state::CrcArgs;
using dqnhip_state::CrcSection;
using dqnhip_state::PackSeg;
using dqnhip_state::RingArr;
using dqnhip_state::RingPackArgs;
using dqnhip_state::StateRec;

__global__ __launch_bounds__(256) void k_state_pack_params(const PackSeg* __restrict__ segs, int n_seg, const DevState* __restrict__ st,
                                                           const float* __restrict__ p_max, StateRec* __restrict__ rec) {
  const int y = blockIdx.y;
  if (y >= n_seg) {                                // the record
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    StateRec r{};
    r.ring_head = st->ring_head; r.ring_size = st->ring_size; r.actor_iter = st->actor_iter; r.critic_iter = st->critic_iter;
    r.update_counter = st->update_counter; r.critic_loss = st->critic_loss; r.avg_q = st->avg_q;
    r.flags = st->flags; r.skipped_steps = st->skipped_steps;
    for (int i = 0; i < 2; ++i) {
      r.ls_mult[i] = st->ls_mult[i][0]; r.ls_good[i] = st->ls_good[i]; r.ls_backoffs[i] = st->ls_backoffs[i]; r.ls_growths[i] = st->ls_growths[i];
    }
    r.p_max = p_max ? *p_max : 0.0f;
    *rec = r;
    return;
  }
  const PackSeg s = segs[y];
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  if (s.vec) {
    const int w4 = s.width >> 2;
    const size_t n4 = (size_t)s.rows * w4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      const size_t row = i / w4; const int c = (int)(i - row * w4);
      reinterpret_cast<f32x4*>(s.dst)[i] = reinterpret_cast<const f32x4*>(s.src + row * s.pitch)[c];
    }
  } else {
    const size_t n = (size_t)s.rows * s.width;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const size_t row = i / s.width; const int c = (int)(i - row * s.width);
      s.dst[i] = s.src[row * s.pitch + c];
    }
  }
}

__global__ __launch_bounds__(256) void k_state_pack_ring(RingPackArgs a) {
  const DevState* st = (const DevState*)a.st;
  const int head = st->ring_head, size = min(st->ring_size, a.cap);
  const int r0 = blockIdx.x * dqnhip_state::kPackRows;
  if (r0 >= size || head < 0 || head >= a.cap) return;      // (a head outside the ring: nothing is read; the writer refuses the record)
  const int rows = min(dqnhip_state::kPackRows, size - r0);
  const RingArr arr = a.arr[blockIdx.y];
  if (arr.vec) {
    const int w4 = arr.width >> 2;
    const f32x4* src = (const f32x4*)arr.src; f32x4* dst = (f32x4*)arr.dst;
    for (int e = threadIdx.x; e < rows * w4; e += blockDim.x) {
      const int i = r0 + e / w4, c = e % w4;
      int phys = head + i; if (phys >= a.cap) phys -= a.cap;
      dst[(size_t)i * w4 + c] = src[(size_t)phys * (arr.pitch >> 2) + c];
    }
  } else if (arr.elem == 4) {
    const float* src = (const float*)arr.src; float* dst = (float*)arr.dst;
    for (int e = threadIdx.x; e < rows * arr.width; e += blockDim.x) {
      const int i = r0 + e / arr.width, c = e % arr.width;
      int phys = head + i; if (phys >= a.cap) phys -= a.cap;
      dst[(size_t)i * arr.width + c] = src[(size_t)phys * arr.pitch + c];
    }
  } else {
    const uint8_t* src = (const uint8_t*)arr.src; uint8_t* dst = (uint8_t*)arr.dst;
    for (int e = threadIdx.x; e < rows * arr.width; e += blockDim.x) {
      const int i = r0 + e / arr.width, c = e % arr.width;
      int phys = head + i; if (phys >= a.cap) phys -= a.cap;
      dst[(size_t)i * arr.width + c] = src[(size_t)phys * arr.pitch + c];
    }
  }
}

__global__ __launch_bounds__(256) void k_state_crc(CrcArgs a) {
  __shared__ uint32_t tab[dqnhip_state::kCrcTableWords];
  __shared__ CrcSection sec[dqnhip_state::kMaxCrcSections];
  for (int k = 0; k < 4; ++k) tab[k * 256 + threadIdx.x] = dqnhip_state::crc_table_entry(k, threadIdx.x);
  if ((int)threadIdx.x < a.n) sec[threadIdx.x] = a.sec[threadIdx.x];
  __syncthreads();
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.total_chunks) return;
  int s = a.n - 1;
  while (s > 0 && sec[s].chunk0 > g) --s;
  const uint64_t rows = a.rec ? (uint64_t)min(max(a.rec->ring_size, 0), a.max_rows) : 0;
  const uint64_t len = sec[s].row_bytes ? rows * sec[s].row_bytes : sec[s].fixed_bytes;
  const uint64_t start = (uint64_t)(g - sec[s].chunk0) * dqnhip_state::kCrcChunk;
  if (start >= len) return;
  const uint64_t n = min((uint64_t)dqnhip_state::kCrcChunk, len - start);
  a.out[g] = dqnhip_state::crc_chunk_raw(tab, a.base + sec[s].off + start, (size_t)n);
}

}  // namespace dqnhip
