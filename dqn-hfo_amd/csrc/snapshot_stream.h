// snapshot_stream.h — the uncompressed `.replaymemory` stream (reference src/dqn.cpp:1146-1178) as the asynchronous Caffe snapshot
// (dqnhip_snapshot_async) assembles it: what k_snap_pack_replay (snapshot_kernels.hip.h, launched from learner_save_async.hip) runs, its host
// side (learner_save_async.hip) and the host test (tests/cpp/snapshot_stream_host.cpp) share.  Plain C++: no HIP header is needed.
//
// The stream:  i32 n, then n records of R = 4 S + 49 bytes in logical order (logical i <- physical slot (head + i) % cap):
//     S x f32 state | 10 x f32 actor output (the first 10 of act[cap][16]) | f32 reward | f32 on-policy target | u8 terminal (0 / 1)
// R = 1 (mod 4): record r starts at byte 4 + r R, 4-byte phase r mod 4, and the stream's length is no multiple of 4 when n is odd.
// The stream is produced one aligned output dword at a time: snap_dword(d) is bytes [4 d, 4 d + 4) of the stream, bytes past its end
// zero.  Inside a record every field but the last byte is a 4-byte word at a 4-byte offset, so a dword that lies inside one record's
// words is two source words funnelled by the record's phase; the (at most two per record) dwords that touch a terminal byte or the
// count are put together byte by byte.  Integer copies only.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SNAP_HD __host__ __device__ inline
#else
#define SNAP_HD inline
#endif

namespace dqnhip_snap {

constexpr int kActOut = 10;                   // floats of the actor output a record holds ...
constexpr int kActPitch = 16;                 // ... out of a ring row of this many
constexpr int kGuardWords = 64;               // the band behind the stream's upper bound that nothing may write
constexpr uint32_t kGuardWord = 0x5AFEC0DEu;

SNAP_HD uint64_t record_bytes(int S) { return 4ull * (uint64_t)S + 4ull * kActOut + 9ull; }
SNAP_HD uint64_t stream_bytes(int S, uint64_t n) { return 4ull + n * record_bytes(S); }
SNAP_HD uint64_t stream_dwords(int S, uint64_t n) { return (stream_bytes(S, n) + 3ull) / 4ull; }

// the ring as the pack reads it: the float arrays as 32-bit words (bit copies), rows of SP / kActPitch / 1 words
struct SnapSrc {
  const uint32_t* state; const uint32_t* act; const uint32_t* reward; const uint32_t* mc; const uint8_t* term;
  int32_t S, SP, cap, head, n;                // n: records in the stream (0 ... cap), head in [0, cap)
};

SNAP_HD int64_t snap_slot(const SnapSrc& s, uint64_t rec) {
  int64_t p = (int64_t)s.head + (int64_t)rec;
  return p >= s.cap ? p - s.cap : p;
}
// word j (0 ... S + 11) of the record in physical slot `slot`
SNAP_HD uint32_t snap_word(const SnapSrc& s, int64_t slot, int j) {
  if (j < s.S) return s.state[slot * s.SP + j];
  j -= s.S;
  if (j < kActOut) return s.act[slot * kActPitch + j];
  return j == kActOut ? s.reward[slot] : s.mc[slot];
}
// byte q of the stream (any q; 0 past the end)
SNAP_HD uint32_t snap_byte(const SnapSrc& s, uint64_t q) {
  if (q < 4) return ((uint32_t)s.n >> (8 * (unsigned)q)) & 0xffu;
  const uint64_t R = record_bytes(s.S), rec = (q - 4) / R, o = (q - 4) - rec * R;
  if (rec >= (uint64_t)s.n) return 0;
  const int64_t slot = snap_slot(s, rec);
  if (o == R - 1) return s.term[slot] ? 1u : 0u;
  return (snap_word(s, slot, (int)(o >> 2)) >> (8 * (unsigned)(o & 3))) & 0xffu;
}
// output dword d of the stream: bytes [4 d, 4 d + 4), little endian
SNAP_HD uint32_t snap_dword(const SnapSrc& s, uint64_t d) {
  const uint64_t q = 4 * d;
  if (q >= 4) {
    const uint64_t R = record_bytes(s.S), rec = (q - 4) / R, o = (q - 4) - rec * R;
    if (rec >= (uint64_t)s.n) return 0;
    if (o + 4 <= R - 1) {                     // inside the words of one record
      const int64_t slot = snap_slot(s, rec);
      const int j = (int)(o >> 2); const unsigned sh = 8 * (unsigned)(o & 3);
      const uint32_t lo = snap_word(s, slot, j);
      if (sh == 0) return lo;
      return (lo >> sh) | (snap_word(s, slot, j + 1) << (32 - sh));      // (o + 4 <= R - 1 and sh != 0: word j + 1 exists)
    }
  }
  return snap_byte(s, q) | snap_byte(s, q + 1) << 8 | snap_byte(s, q + 2) << 16 | snap_byte(s, q + 3) << 24;
}

// ---- the workgroup form, which k_snap_pack_replay runs: a block owns K records, K a multiple of 16, so their K R bytes are whole
// 16-byte pieces, and the launcher places the stream so that its first record (byte 4) lies on a 16-byte boundary.  The block stages
// its records as rows of S + 13 words: the record's S + 12 words, then the terminal byte as a word.  Byte o of a record is then byte o
// of its row for every o (R - 1 = 4 (S + 12)).  Records from n on are rows of zeros.  The count is block 0's to store.
SNAP_HD int snap_lds_row_words(int S) { return S + kActOut + 3; }
// word j (0 ... S + 12) of the staged row of record `rec`
SNAP_HD uint32_t snap_lds_word(const SnapSrc& s, int64_t rec, int j) {
  const int last = s.S + kActOut + 1;           // the record's last whole word; the terminal byte's word follows it
  if (rec >= (int64_t)s.n) return 0u;
  const int64_t slot = snap_slot(s, (uint64_t)rec);
  return j <= last ? snap_word(s, slot, j) : (s.term[slot] ? 1u : 0u);
}
// four bytes of the staged rows from byte o (< R) of row l on, little endian; they may run into row l + 1
SNAP_HD uint32_t snap_lds_dword(const uint32_t* rows, int W, uint32_t R, uint32_t l, uint32_t o) {
  if (o + 4 <= R - 1) {                       // inside the words of one record
    const uint32_t* w = rows + (size_t)l * W + (o >> 2); const unsigned sh = 8 * (o & 3);
    return sh == 0 ? w[0] : (w[0] >> sh) | (w[1] << (32 - sh));
  }
  uint32_t v = 0;
  for (unsigned k = 0; k < 4; ++k) {
    uint32_t ll = l, oo = o + k;
    if (oo >= R) { oo -= R; ll += 1; }
    v |= ((rows[(size_t)ll * W + (oo >> 2)] >> (8 * (oo & 3))) & 0xffu) << (8 * k);
  }
  return v;
}

}  // namespace dqnhip_snap
