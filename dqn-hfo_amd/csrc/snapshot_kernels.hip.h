// snapshot_kernels.hip.h — the device side of the asynchronous Caffe snapshot (dqnhip_snapshot_async, include/dqnhip.h):
// the replay memory as the uncompressed `.replaymemory` stream, in its final bytes, in the snapshot's staging buffer.  Included and
// launched by learner_save_async.hip only; a learner that never snapshots asynchronously launches none of this.  The parameters and the
// record (k_state_pack_params) and the stream's CRC-32 (k_state_crc) are the learner-state save's kernels, unchanged.
//
//   k_snap_pack_replay   a workgroup owns K records (K a multiple of 16, so their bytes are whole 16-byte pieces; snapshot_stream.h
//                        has the layout and the byte-selection body, which the host test runs too), stages them in LDS — a wave
//                        per record, its lanes on consecutive words of the ring rows — and streams them out as aligned 16-byte
//                        stores, one division per piece.  (ring_head, ring_size) are read from DevState here, on the device — an
//                        env front-end appends there, the host's mirrors may be stale; the count in the stream's first dword is
//                        that ring_size.  The piece that holds the stream's last (zero-filled) dword is stored dword by dword and
//                        blocks behind it exit: nothing behind that dword is written.
// Measured against the form with one thread per output dword (scripts/snap_pack_forms.hip keeps that one; profiles/snapshot_async_ab.md):
// 285 us against 552 us at 1 M records of S = 58, K = 64; K = 128 and 256 are slower (the staging loop is a chain of dependent loads).
// Integer copies only, no atomics; the kernel writes nothing but the staging buffer.
#pragma once
#include "learner_args.hip.h"       // DevState, Ring, kNO, kAP
#include "snapshot_stream.h"

namespace dqnhip {

static_assert(dqnhip_snap::kActOut == kNO && dqnhip_snap::kActPitch == kAP, "snapshot_stream.h restates the ring's actor-output row");

// out: the stream's first dword, the count; out + 1, the first record, is 16-byte aligned; max_dwords: stream_dwords(S, cap), the
// room at out; dynamic LDS: K snap_lds_row_words(S) words
__global__ __launch_bounds__(256) void k_snap_pack_replay(Ring ring, const DevState* __restrict__ st, uint32_t* __restrict__ out, uint64_t max_dwords, int K) {
  extern __shared__ uint32_t snap_rows[];
  const int head = st->ring_head, n = min(max(st->ring_size, 0), ring.cap);
  if (head < 0 || head >= ring.cap) return;                 // (nothing is read; the writer refuses the record)
  if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = (uint32_t)n;
  const int64_t rec0 = (int64_t)blockIdx.x * K;             // the record staged as row 0
  if (rec0 >= n) return;                                    // (the whole block: its records are behind the stream)
  const int W = dqnhip_snap::snap_lds_row_words(ring.S);
  const uint32_t R = (uint32_t)dqnhip_snap::record_bytes(ring.S);
  dqnhip_snap::SnapSrc s{(const uint32_t*)ring.state, (const uint32_t*)ring.act, (const uint32_t*)ring.reward, (const uint32_t*)ring.mc, ring.term,
                         ring.S, ring.SP, ring.cap, head, n};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 4
  for (int l = wave; l < K; l += 4)
    for (int j = lane; j < W; j += 64) snap_rows[l * W + j] = dqnhip_snap::snap_lds_word(s, rec0 + l, j);
  __syncthreads();
  const uint64_t total = min(max_dwords, dqnhip_snap::stream_dwords(ring.S, (uint64_t)n));
  const uint32_t pieces = (uint32_t)K / 16u * R;            // 16-byte pieces of a block: K R / 16
  const uint64_t d0 = 1ull + (uint64_t)blockIdx.x * pieces * 4u;      // the block's first dword
  for (uint32_t p = threadIdx.x; p < pieces; p += 256) {
    const uint64_t d = d0 + 4ull * p;
    if (d >= total) break;
    const uint32_t t = 16u * p;                             // the piece's first byte, counted from row 0
    uint32_t l = t / R, o = t - l * R, v[4];
    for (int k = 0; k < 4; ++k) {
      v[k] = dqnhip_snap::snap_lds_dword(snap_rows, W, R, l, o);
      o += 4; if (o >= R) { o -= R; l += 1; }
    }
    if (d + 4 <= total) *(uint4*)(out + d) = make_uint4(v[0], v[1], v[2], v[3]);
    else for (int k = 0; k < 4 && d + k < total; ++k) out[d + k] = v[k];
  }
}

}  // namespace dqnhip
