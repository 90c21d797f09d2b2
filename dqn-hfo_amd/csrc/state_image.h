// state_image.h — what the asynchronous learner-state save (dqnhip_save_state_async) shares between its kernels
// (state_kernels.hip.h), the unit that launches them and holds its host side (learner_save_async.hip) and the host test
// (tests/cpp/state_stream_host.cpp): the device record, the CRC section table, and zlib's CRC-32 as bodies that compile for the
// device and for the host.  Plain C++: no HIP header is needed to include it.
//
// CRC-32 (reflected polynomial 0xEDB88320, register starts at ~0, result inverted).  The register update is linear over GF(2) in
// (register, data), so for a message A || B
//     reg(A || B, r0) = Z_|B|(reg(A, r0)) ^ raw(B),     raw(B) = reg(B, 0),   Z_n = "append n zero bytes" (a 32 x 32 bit matrix).
// The device computes raw() of each kCrcChunk-byte chunk of a section (one thread per chunk, slice-by-4 tables in LDS); the chunks
// are folded left to right with Z_kCrcChunk (Z of the remainder for a short last chunk): integers only, exact by construction.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define STATE_HD __host__ __device__ inline
#else
#define STATE_HD inline
#endif

namespace dqnhip_state {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcChunk = 1024;          // bytes per chunk CRC: one thread's stream
constexpr int kCrcTableWords = 4 * 256;       // slice-by-4: t[k][b] = the register after byte b and k zero bytes

STATE_HD uint32_t crc_table_entry(int k, uint32_t b) {
  uint32_t c = b;
  for (int i = 0; i < 8 * (k + 1); ++i) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
  return c;
}
STATE_HD uint32_t crc_byte(const uint32_t* t, uint32_t c, uint8_t b) { return t[(c ^ b) & 0xffu] ^ (c >> 8); }
STATE_HD uint32_t crc_word(const uint32_t* t, uint32_t c, uint32_t w) {      // four bytes, little endian
  c ^= w;
  return t[768 + (c & 0xffu)] ^ t[512 + ((c >> 8) & 0xffu)] ^ t[256 + ((c >> 16) & 0xffu)] ^ t[c >> 24];
}

struct CrcWord4 { uint32_t x, y, z, w; };
// 16 bytes at a 16-byte boundary: one global_load_dwordx4 on the device
STATE_HD CrcWord4 crc_load16(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *reinterpret_cast<const CrcWord4*>(__builtin_assume_aligned(p, 16));
#else
  CrcWord4 v; memcpy(&v, p, sizeof v); return v;
#endif
}

// raw(): the register, started at 0, after the n bytes at p.  Any n, any alignment of p: single bytes up to the first 16-byte
// boundary, 16-byte loads, single bytes for what is left.
STATE_HD uint32_t crc_chunk_raw(const uint32_t* t, const uint8_t* p, size_t n) {
  uint32_t c = 0;
  for (; n > 0 && ((uintptr_t)p & 15u) != 0; ++p, --n) c = crc_byte(t, c, *p);
  for (; n >= 16; p += 16, n -= 16) {
    const CrcWord4 v = crc_load16(p);
    c = crc_word(t, c, v.x); c = crc_word(t, c, v.y); c = crc_word(t, c, v.z); c = crc_word(t, c, v.w);
  }
  for (; n > 0; ++p, --n) c = crc_byte(t, c, *p);
  return c;
}

// ---- the combine step: 32 x 32 matrices over GF(2), column i = the image of bit i ----
STATE_HD uint32_t gf2_times(const uint32_t* mat, uint32_t v) {
  uint32_t s = 0;
  for (int i = 0; v != 0; v >>= 1, ++i) if (v & 1u) s ^= mat[i];
  return s;
}
STATE_HD void gf2_square(uint32_t* m) {
  uint32_t sq[32];
  for (int i = 0; i < 32; ++i) sq[i] = gf2_times(m, m[i]);
  for (int i = 0; i < 32; ++i) m[i] = sq[i];
}
// op = Z_n: appending n zero bytes to a message takes the register r to gf2_times(op, r)
STATE_HD void crc_zeros_op(uint32_t* op, uint64_t n) {
  uint32_t pw[32];                            // Z of 1, 2, 4, ... bytes
  pw[0] = kCrcPoly;                           // one zero BIT: bit 0 falls out and feeds the polynomial back, the others move down
  for (int i = 1; i < 32; ++i) pw[i] = 1u << (i - 1);
  gf2_square(pw); gf2_square(pw); gf2_square(pw);
  for (int i = 0; i < 32; ++i) op[i] = 1u << i;
  for (; n != 0; n >>= 1) {
    if (n & 1u) for (int i = 0; i < 32; ++i) op[i] = gf2_times(pw, op[i]);
    if (n >> 1) gf2_square(pw);
  }
}
// the same operator by bytes of the register: tab[k][b] = op (b << 8k); four lookups per application
STATE_HD void crc_op_table(uint32_t* tab, const uint32_t* op) {
  for (int k = 0; k < 4; ++k)
    for (uint32_t b = 0; b < 256; ++b) tab[k * 256 + b] = gf2_times(op, b << (8 * k));
}
STATE_HD uint32_t crc_op_apply(const uint32_t* tab, uint32_t r) {
  return tab[r & 0xffu] ^ tab[256 + ((r >> 8) & 0xffu)] ^ tab[512 + ((r >> 16) & 0xffu)] ^ tab[768 + (r >> 24)];
}
// The CRC-32 of `bytes` bytes from the raw() of their chunks (ceil(bytes / kCrcChunk) of them, the last one short if bytes is no
// multiple).  chunk_tab: crc_op_table of Z_kCrcChunk.  0 bytes: no chunk, the CRC of the empty message.
STATE_HD uint32_t crc_fold_chunks(const uint32_t* raws, uint64_t bytes, const uint32_t* chunk_tab) {
  uint32_t r = 0xffffffffu;
  const uint64_t full = bytes / kCrcChunk, rest = bytes % kCrcChunk;
  for (uint64_t k = 0; k < full; ++k) r = crc_op_apply(chunk_tab, r) ^ raws[k];
  if (rest) {
    uint32_t op[32];
    crc_zeros_op(op, rest);
    r = gf2_times(op, r) ^ raws[full];
  }
  return ~r;
}

// ---- the image the pack kernels leave in the staging buffer ----
// What DEVS, LSCL, RING, PERC and the header need of the device, captured in stream order by the pack (k_state_pack_params' last
// slice).  It lies at the front of the staging buffer.
struct StateRec {
  int32_t ring_head, ring_size, actor_iter, critic_iter;
  uint64_t update_counter;
  float critic_loss, avg_q;
  int32_t flags, skipped_steps;
  float ls_mult[2];
  int32_t ls_good[2], ls_backoffs[2], ls_growths[2];
  float p_max;
  int32_t reserved[5];
};
static_assert(sizeof(StateRec) == 96, "six 16-byte lines");

// One strided piece of a parameter section: rows x width floats at a pitch of `pitch` floats -> dense floats at dst.  vec: width,
// pitch and both addresses are whole 16-byte units, the piece moves as float4.
struct PackSeg { const float* src; float* dst; int32_t rows, width, pitch, vec; };
// One array of the ring: logical row i of the window <- physical slot (head + i) % cap; `width` elements of `elem` bytes (4 or 1)
// of a row of `pitch` elements.  vec (elem 4 only): as in PackSeg.
constexpr int kRingArrays = 7;                // state, next, act, reward, mc, term, priority leaves
constexpr int kPackRows = 256;                // logical rows per block of k_state_pack_ring
struct RingArr { const void* src; void* dst; int32_t width, pitch, elem, vec; };
struct RingPackArgs { const void* st; int32_t cap, n_arr; RingArr arr[kRingArrays]; };   // st: the DevState that holds (ring_head, ring_size)

// One section whose bytes the device checksums.  row_bytes 0: fixed_bytes long; else ring_size (StateRec) x row_bytes long.
// Its chunk CRCs are out[chunk0 ...], room for the longest it can be.
constexpr int kMaxCrcSections = 16;
struct CrcSection { uint64_t off, fixed_bytes; uint32_t row_bytes, chunk0; };
struct CrcArgs {
  const uint8_t* base;          // sec[].off counts from here
  const StateRec* rec;          // null: no section's length depends on the ring
  uint32_t* out;
  int32_t n;                    // sections
  int32_t max_rows;             // the ring's capacity: what a ring_size outside [0, max_rows] is clamped to
  uint32_t total_chunks;        // = the grid's threads that have work
  uint32_t reserved;
  CrcSection sec[kMaxCrcSections];
};

}  // namespace dqnhip_state
