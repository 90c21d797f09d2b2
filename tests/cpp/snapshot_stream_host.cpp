// The host-compilable parts of the asynchronous Caffe snapshot (dqnhip_snapshot_async), without a GPU (built and run by
// tests/test_snapshot_stream_host.py: plain, under the address + undefined-behaviour sanitizers, and under the thread sanitizer):
//   * the pack body (dqn-hfo_amd/csrc/snapshot_stream.h: the dword-by-dword reference and what k_snap_pack_replay runs per workgroup) against the memcpy loop of
//     dqnhip_snapshot_replay_memory, over state sizes, memory sizes and ring heads, with the bytes behind the stream checked untouched;
//   * the parallel gzip writer (gzip_parallel.cpp) against gzread: worker counts, stream lengths around the chunk size, the trailer,
//     a wrong CRC, a missing directory.
// usage: snapshot_stream_host <directory>   — leaves <directory>/member_w<workers>.gz + payload.bin for the Python side to read back
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gzip_parallel.h"
#include "snapshot_stream.h"

using namespace dqnhip_snap;
using dqnhip_state::GzipParallelWriter;

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail = 1; } \
  } while (0)

static bool exists(const std::string& p) { struct stat sb; return stat(p.c_str(), &sb) == 0; }
static std::vector<uint8_t> slurp(const std::string& p) {
  std::vector<uint8_t> v;
  FILE* f = fopen(p.c_str(), "rb");
  if (!f) return v;
  uint8_t buf[4096];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}
static uint32_t rnd(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

// ---- the pack body ----
// a ring as the learner holds it: padded rows, every word distinct (pad columns too: a pad word in the stream would show)
struct HostRing {
  int S, SP, cap;
  std::vector<uint32_t> state, act, reward, mc;
  std::vector<uint8_t> term;
  HostRing(int S_, int cap_, uint64_t seed) : S(S_), SP((S_ + 63) / 64 * 64), cap(cap_) {
    state.resize((size_t)cap * SP); act.resize((size_t)cap * kActPitch); reward.resize(cap); mc.resize(cap); term.resize(cap);
    for (auto& x : state) x = rnd(seed) | 1u;
    for (auto& x : act) x = rnd(seed) | 1u;
    for (auto& x : reward) x = rnd(seed) | 1u;
    for (auto& x : mc) x = rnd(seed) | 1u;
    for (auto& x : term) { const uint32_t r = rnd(seed) % 3; x = r == 0 ? 0 : r == 1 ? 1 : (uint8_t)(2 + rnd(seed) % 250); }   // (any non-zero byte is "terminal")
  }
};

// the synchronous snapshot's loop (learner_io.hip, dqnhip_snapshot_replay_memory): logical order, field by field
static std::vector<uint8_t> reference_stream(const HostRing& g, int head, int n) {
  std::vector<uint8_t> out(4 + (size_t)n * record_bytes(g.S));
  const int32_t count = n;
  memcpy(out.data(), &count, 4);
  uint8_t* p = out.data() + 4;
  for (int i = 0; i < n; ++i) {
    const size_t slot = (size_t)((head + i) % g.cap);
    memcpy(p, &g.state[slot * g.SP], (size_t)g.S * 4); p += (size_t)g.S * 4;
    memcpy(p, &g.act[slot * kActPitch], kActOut * 4); p += kActOut * 4;
    memcpy(p, &g.reward[slot], 4); p += 4;
    memcpy(p, &g.mc[slot], 4); p += 4;
    *p++ = g.term[slot] ? 1 : 0;
  }
  return out;
}

static void test_pack(int S, int cap, int head, int n) {
  const HostRing g(S, cap, (uint64_t)S * 1000003u + (uint64_t)cap * 101u + (uint64_t)head * 7u + (uint64_t)n);
  const std::vector<uint8_t> ref = reference_stream(g, head, n);
  CHECK(ref.size() == stream_bytes(S, (uint64_t)n));
  const SnapSrc src{g.state.data(), g.act.data(), g.reward.data(), g.mc.data(), g.term.data(), S, g.SP, cap, head, n};
  // the staging buffer as the launcher lays it out: room for a full ring, the guard band behind it, sentinels everywhere
  const uint64_t max_dwords = stream_dwords(S, (uint64_t)cap), dwords = stream_dwords(S, (uint64_t)n);
  std::vector<uint32_t> stage(max_dwords + kGuardWords, kGuardWord);
  // the dword-by-dword form: one thread per dword of a grid, those past the stream's last dword write nothing
  for (uint64_t d = 0; d < (max_dwords + 255) / 256 * 256; ++d) {
    if (d >= max_dwords || d >= dwords) continue;
    stage[d] = snap_dword(src, d);
  }
  const uint8_t* got = (const uint8_t*)stage.data();
  CHECK(memcmp(got, ref.data(), ref.size()) == 0);
  for (size_t b = ref.size(); b < 4 * dwords; ++b) CHECK(got[b] == 0);                      // the last partial dword is zero-filled
  for (uint64_t d = dwords; d < stage.size(); ++d) CHECK(stage[d] == kGuardWord);            // nothing behind it is written
  // the workgroup form, as k_snap_pack_replay runs it: per block the staged rows (a vector of exactly the kernel's LDS size), then
  // its 16-byte pieces; K = 64 is the launcher's
  for (int K : {16, 64, 256}) {
    std::vector<uint32_t> stage2(max_dwords + kGuardWords, kGuardWord);
    const int W = snap_lds_row_words(S);
    const uint32_t R = (uint32_t)record_bytes(S), pieces = (uint32_t)K / 16u * R;
    const uint64_t blocks = ((uint64_t)cap + K - 1) / K, total = std::min(max_dwords, dwords);
    std::vector<uint32_t> rows((size_t)K * W);
    for (uint64_t b = 0; b < blocks; ++b) {
      if (b == 0) stage2[0] = (uint32_t)n;
      const int64_t rec0 = (int64_t)b * K;
      if (rec0 >= n) continue;
      for (int l = 0; l < K; ++l)
        for (int j = 0; j < W; ++j) rows[(size_t)l * W + j] = snap_lds_word(src, rec0 + l, j);
      for (uint32_t p = 0; p < pieces; ++p) {
        const uint64_t d = 1 + b * pieces * 4u + 4ull * p;
        if (d >= total) break;
        const uint32_t t = 16u * p;
        uint32_t l = t / R, o = t - l * R;
        for (int k = 0; k < 4; ++k) {
          CHECK(l < (uint32_t)K);
          const uint32_t v = snap_lds_dword(rows.data(), W, R, l, o);
          o += 4; if (o >= R) { o -= R; l += 1; }
          if (d + k < total) stage2[d + k] = v;
        }
      }
    }
    CHECK(stage2 == stage);
  }
  // every byte on its own, and the bytes past the end
  for (uint64_t q = 0; q < ref.size(); q += (q < 700 ? 1 : 97)) CHECK(snap_byte(src, q) == ref[q]);
  for (uint64_t q = ref.size(); q < ref.size() + 8; ++q) CHECK(snap_byte(src, q) == 0);
  if (g_fail) printf("  (pack: S %d cap %d head %d n %d)\n", S, cap, head, n);
}

// ---- the parallel writer ----
static std::vector<uint8_t> payload(size_t n, int salt) {      // compressible, like rows of floats, with an incompressible stretch
  std::vector<uint8_t> v(n);
  uint64_t s = 77 + (uint64_t)salt;
  for (size_t j = 0; j < n; ++j) v[j] = (j / 4096) % 3 == 2 ? (uint8_t)rnd(s) : (uint8_t)(salt * 7 + (j % 232) * 13 + (j >> 10));
  return v;
}
static uint32_t crc_of(const std::vector<uint8_t>& v) { return (uint32_t)crc32(crc32(0L, Z_NULL, 0), v.data(), (uInt)v.size()); }

// -> 0 and *out = the member's payload; 1: gzread / gzclose reported an error
static int read_member(const std::string& path, std::vector<uint8_t>* out) {
  gzFile f = gzopen(path.c_str(), "rb");
  if (!f) return 1;
  out->clear();
  std::vector<uint8_t> buf(1 << 16);
  int k, bad = 0;
  while ((k = gzread(f, buf.data(), (unsigned)buf.size())) > 0) out->insert(out->end(), buf.begin(), buf.begin() + k);
  if (k < 0) bad = 1;
  int errnum = Z_OK;
  gzerror(f, &errnum);
  if (errnum != Z_OK && errnum != Z_STREAM_END) bad = 1;
  if (gzclose(f) != Z_OK) bad = 1;
  return bad;
}

static void test_writer(const std::string& dir, int workers, size_t chunk, size_t n, int piece) {
  const std::vector<uint8_t> data = payload(n, workers + (int)(n % 11));
  const std::string fn = dir + "/w" + std::to_string(workers) + "_" + std::to_string(n) + ".gz";
  std::string err;
  GzipParallelWriter w;
  CHECK(w.open(fn.c_str(), workers, chunk, &err) == 0);
  CHECK(exists(fn + ".tmp") && !exists(fn));
  for (size_t at = 0; at < n;) {                                 // pieces that do not line up with the chunks
    const size_t k = std::min(n - at, (size_t)piece + at % 7);
    CHECK(w.append(data.data() + at, k, &err) == 0);
    at += k;
  }
  CHECK(w.finish(crc_of(data), &err) == 0);
  CHECK(exists(fn) && !exists(fn + ".tmp"));
  CHECK(w.payload_bytes() == n);
  const std::vector<uint8_t> file = slurp(fn);
  CHECK(file.size() == w.file_bytes() && file.size() >= 20);
  // the trailer holds the CRC it was given and the length
  uint32_t crc = 0, isize = 0;
  memcpy(&crc, file.data() + file.size() - 8, 4); memcpy(&isize, file.data() + file.size() - 4, 4);
  CHECK(crc == crc_of(data) && isize == (uint32_t)n);
  static const uint8_t head[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
  CHECK(memcmp(file.data(), head, 10) == 0);
  std::vector<uint8_t> back;
  CHECK(read_member(fn, &back) == 0);
  CHECK(back == data);
  if (g_fail) printf("  (writer: workers %d chunk %zu n %zu: %s)\n", workers, chunk, n, err.c_str());
  remove(fn.c_str());
}

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: %s <directory>\n", argv[0]); return 2; }
  const std::string dir = argv[1];

  // R = 1 (mod 4) for every S
  for (int S = 1; S < 200; ++S) CHECK(record_bytes(S) % 4 == 1 && record_bytes(S) == (uint64_t)(4 * S + 49));
  // the pack body: sizes 1 ... 5 put every alignment phase of a record and both parities of n under test; heads that make the window
  // straddle the ring's end
  const int cap = 300;
  for (int S : {58, 59, 77, 1, 64}) {
    for (int n : {0, 1, 2, 3, 4, 5, 255, 256, 257, cap - 1, cap}) {
      for (int head : {0, 1, cap - 3, cap - 1, 123}) test_pack(S, cap, head, n);
    }
  }
  test_pack(58, 1, 0, 1);
  test_pack(58, 1, 0, 0);

  // the parallel writer: chunks small enough that every length class is cheap
  const size_t chunk = 1 << 15;
  for (int workers : {1, 2, 8})
    for (size_t n : {(size_t)0, (size_t)1, chunk - 1, chunk, chunk + 1, 2 * chunk, 5 * chunk + 12345, 19 * chunk + 1})
      test_writer(dir, workers, chunk, n, 10007);
  test_writer(dir, 3, 1, 5, 2);                                   // one-byte chunks
  test_writer(dir, 8, GzipParallelWriter::kDefaultChunk, 3 * GzipParallelWriter::kDefaultChunk + 281, 1 << 23);      // the product's chunk size

  // a wrong CRC in the trailer makes gzread fail: the check is live
  {
    const std::vector<uint8_t> data = payload(3 * chunk + 5, 3);
    const std::string fn = dir + "/wrongcrc.gz";
    std::string err;
    GzipParallelWriter w;
    CHECK(w.open(fn.c_str(), 2, chunk, &err) == 0 && w.append(data.data(), data.size(), &err) == 0 && w.finish(crc_of(data) ^ 0x10u, &err) == 0);
    std::vector<uint8_t> back;
    CHECK(read_member(fn, &back) != 0);
    remove(fn.c_str());
  }
  // a missing directory fails cleanly, a writer dropped before finish leaves nothing
  {
    std::string err;
    GzipParallelWriter w;
    CHECK(w.open((dir + "/no/such/dir/x.gz").c_str(), 4, chunk, &err) != 0 && !err.empty());
    CHECK(w.append("abc", 3, &err) != 0 && w.finish(0, &err) != 0);
    const std::vector<uint8_t> data = payload(4 * chunk, 9);
    const std::string fn = dir + "/dropped.gz";
    {
      GzipParallelWriter d;
      CHECK(d.open(fn.c_str(), 4, chunk, &err) == 0 && d.append(data.data(), data.size(), &err) == 0);
    }
    CHECK(!exists(fn) && !exists(fn + ".tmp"));
    CHECK(w.open(fn.c_str(), 0, chunk, &err) != 0);              // no workers
    CHECK(!exists(fn + ".tmp"));
  }
  // files for the Python side: gzip.decompress must return payload.bin
  {
    const std::vector<uint8_t> data = payload(7 * chunk + 333, 5);
    FILE* f = fopen((dir + "/payload.bin").c_str(), "wb");
    CHECK(f && fwrite(data.data(), 1, data.size(), f) == data.size());
    if (f) fclose(f);
    for (int workers : {1, 8}) {
      std::string err;
      GzipParallelWriter w;
      CHECK(w.open((dir + "/member_w" + std::to_string(workers) + ".gz").c_str(), workers, chunk, &err) == 0 &&
            w.append(data.data(), data.size(), &err) == 0 && w.finish(crc_of(data), &err) == 0);
    }
  }
  if (g_fail) { printf("snapshot stream host FAILED\n"); return 1; }
  printf("snapshot stream host OK\n");
  return 0;
}
