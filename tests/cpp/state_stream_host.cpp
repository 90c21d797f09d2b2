// The host-compilable parts of the asynchronous learner-state save, without a GPU (built and run by tests/test_state_stream_host.py,
// once plain and once under the address + undefined-behaviour sanitizers):
//   * the chunk CRC and the combine step (dqn-hfo_amd/csrc/state_image.h: the bodies k_state_crc and the writer thread run) against
//     zlib's crc32 and crc32_combine;
//   * the streaming writer (state_codec.cpp: StreamWriter) against write_file, byte for byte, and what a failed append leaves.
// usage: state_stream_host <directory>   — leaves <directory>/whole.bin, stream.bin, many.bin for the Python side to read back
#include <signal.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "state_codec.h"
#include "state_image.h"

using namespace dqnhip_state;

extern "C" int dqnhip_internal_set_error(const char*) { return 1; }      // (state_codec.cpp's C entry points report through the library)

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail = 1; } \
  } while (0)

static uint32_t g_tab[kCrcTableWords], g_chunk_tab[kCrcTableWords];

// the save's path: raw() of every chunk, folded
static uint32_t crc_by_chunks(const uint8_t* p, size_t n) {
  std::vector<uint32_t> raws;
  for (size_t at = 0; at < n; at += kCrcChunk) raws.push_back(crc_chunk_raw(g_tab, p + at, n - at < kCrcChunk ? n - at : kCrcChunk));
  return crc_fold_chunks(raws.data(), n, g_chunk_tab);
}

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

struct Sec { uint32_t tag; std::vector<uint8_t> data; };
static std::vector<uint8_t> pattern(size_t n, int salt) {
  std::vector<uint8_t> v(n);
  for (size_t j = 0; j < n; ++j) v[j] = (uint8_t)(salt * 7 + j * 13 + (j >> 8));
  return v;
}
static dqnhip_state_info_t some_info() {
  dqnhip_state_info_t in{};
  in.struct_size = (int32_t)sizeof in; in.version = 1; in.precision = 1; in.minibatch = 128; in.state_size = 58; in.num_hidden = 2;
  in.hidden[0] = 64; in.hidden[1] = 128; in.replay_capacity = 96; in.memory_size = 95; in.actor_iter = 3; in.critic_iter = 4;
  in.has_memory = 1; in.seed = 0xFEDCBA9876543210ull; in.update_counter = (1ull << 40) + 7;
  return in;
}
static int write_whole(const std::string& fn, const std::vector<Sec>& secs, std::string* err) {
  std::vector<Section> s;
  for (const Sec& x : secs) s.push_back({x.tag, x.data.data(), x.data.size()});
  return write_file(fn.c_str(), some_info(), s, err);
}
// the same sections through the streaming writer, the payload cut into pieces that ignore the section boundaries
static int write_stream(const std::string& fn, const std::vector<Sec>& secs, std::string* err) {
  std::vector<StreamEntry> e;
  std::vector<uint8_t> payload;
  for (const Sec& x : secs) {
    e.push_back({x.tag, crc_by_chunks(x.data.data(), x.data.size()), x.data.size()});
    payload.insert(payload.end(), x.data.begin(), x.data.end());
  }
  StreamWriter w;
  if (w.open(fn.c_str(), some_info(), e, err)) return 1;
  static const size_t kPieces[] = {0, 1, 7, 1000, 4096, 3, 65536, 12345};
  size_t at = 0;
  for (int i = 0; at < payload.size(); ++i) {
    const size_t k = std::min(kPieces[i % 8], payload.size() - at);
    if (w.append(payload.data() + at, k, err)) return 1;
    at += k;
  }
  return w.finish(err);
}

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: %s <directory>\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  for (int k = 0; k < 4; ++k) for (uint32_t b = 0; b < 256; ++b) g_tab[k * 256 + b] = crc_table_entry(k, b);
  { uint32_t op[32]; crc_zeros_op(op, kCrcChunk); crc_op_table(g_chunk_tab, op); }
  CHECK(memcmp(g_tab, get_crc_table(), 256 * sizeof(uint32_t)) == 0);      // slice 0 is zlib's own table

  // ---- chunk CRC + fold against zlib's crc32 ----
  const size_t lens[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, kCrcChunk - 1, kCrcChunk, kCrcChunk + 1, 2 * kCrcChunk + 7, (1u << 20) + 13};
  const size_t max_len = (1u << 20) + 13;
  uint8_t* raw = (uint8_t*)aligned_alloc(16, ((max_len + 4 + 15) / 16) * 16);
  uint64_t lcg = 0x1234567ull;
  int cases = 0;
  for (int content = 0; content < 3; ++content)
    for (size_t len : lens)
      for (size_t off = 0; off < 4; ++off) {
        uint8_t* p = raw + off;
        if (content == 0) memset(p, 0, len);
        else if (content == 1) memset(p, 0xff, len);
        else for (size_t j = 0; j < len; ++j) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; p[j] = (uint8_t)(lcg >> 56); }
        const uint32_t want = (uint32_t)crc32(crc32(0L, Z_NULL, 0), p, (uInt)len), got = crc_by_chunks(p, len);
        if (want != got) printf("content %d len %zu offset %zu: %08x, zlib %08x\n", content, len, off, got, want);
        CHECK(want == got);
        ++cases;
      }
  CHECK(cases == 3 * 14 * 4);
  // ---- the combine step against zlib's crc32_combine: crc(A || B) from crc(A), raw(B), |B| ----
  for (size_t la : {(size_t)0, (size_t)1, (size_t)777, (size_t)kCrcChunk})
    for (size_t lb : {(size_t)0, (size_t)1, (size_t)5, (size_t)kCrcChunk, (size_t)100000}) {
      const uint8_t *a = raw, *b = raw + la;
      const uint32_t ca = (uint32_t)crc32(0L, a, (uInt)la), cb = (uint32_t)crc32(0L, b, (uInt)lb);
      uint32_t op[32];
      crc_zeros_op(op, lb);
      // raw(B) in pieces as well: raw is itself foldable from register 0
      uint32_t rb = 0;
      for (size_t at = 0; at < lb; at += kCrcChunk) {
        const size_t k = lb - at < kCrcChunk ? lb - at : kCrcChunk;
        uint32_t o[32]; crc_zeros_op(o, k);
        rb = gf2_times(o, rb) ^ crc_chunk_raw(g_tab, b + at, k);
      }
      const uint32_t got = ~(gf2_times(op, ~ca) ^ rb);
      CHECK(got == (uint32_t)crc32_combine(ca, cb, (z_off_t)lb));
      CHECK(got == (uint32_t)crc32(0L, a, (uInt)(la + lb)));
    }
  free(raw);

  // ---- the streaming writer against write_file ----
  std::string err;
  std::vector<Sec> secs;
  secs.push_back({kTagW[0], pattern(4 * 1001, 1)});
  secs.push_back({kTagDev, pattern(32, 2)});
  secs.push_back({kTagHost, {}});                                  // a zero-length section in the middle
  secs.push_back({kTagStates, pattern(95 * 58 * 4, 3)});
  secs.push_back({kTagTerm, pattern(95, 4)});                      // odd length
  secs.push_back({kTagPerLeaves, {}});
  secs.push_back({kTagUser, pattern(4097, 5)});                    // odd length, last
  CHECK(write_whole(dir + "/whole.bin", secs, &err) == 0);
  CHECK(write_stream(dir + "/stream.bin", secs, &err) == 0);
  CHECK(!slurp(dir + "/whole.bin").empty() && slurp(dir + "/whole.bin") == slurp(dir + "/stream.bin"));
  CHECK(!exists(dir + "/whole.bin.tmp") && !exists(dir + "/stream.bin.tmp"));
  // the 64-section limit: 64 pass, 65 are refused by both and leave nothing
  std::vector<Sec> many;
  for (int i = 0; i < 64; ++i) many.push_back({tag4('S', 'C', (char)('0' + i / 10), (char)('0' + i % 10)), pattern((size_t)(i * 37) % 300, i)});
  CHECK(write_whole(dir + "/many_whole.bin", many, &err) == 0);
  CHECK(write_stream(dir + "/many.bin", many, &err) == 0);
  CHECK(slurp(dir + "/many_whole.bin") == slurp(dir + "/many.bin"));
  many.push_back({tag4('S', 'C', '6', '4'), pattern(5, 64)});
  CHECK(write_whole(dir + "/toomany.bin", many, &err) != 0 && err.find("too many sections") != std::string::npos);
  err.clear();
  CHECK(write_stream(dir + "/toomany.bin", many, &err) != 0 && err.find("too many sections") != std::string::npos);
  CHECK(!exists(dir + "/toomany.bin") && !exists(dir + "/toomany.bin.tmp"));
  // no sections at all
  CHECK(write_whole(dir + "/none_whole.bin", {}, &err) == 0 && write_stream(dir + "/none.bin", {}, &err) == 0);
  CHECK(slurp(dir + "/none_whole.bin") == slurp(dir + "/none.bin") && slurp(dir + "/none.bin").size() == kHeaderBytes);

  // ---- failures leave no file and no .tmp, and an existing file alone ----
  {
    const std::vector<uint8_t> big = pattern(1 << 20, 9);
    const std::vector<StreamEntry> e = {{kTagUser, crc_by_chunks(big.data(), big.size()), big.size()}};
    const std::string fn = dir + "/fail.bin";
    {   // more bytes than declared
      StreamWriter w; err.clear();
      CHECK(w.open(fn.c_str(), some_info(), e, &err) == 0 && exists(fn + ".tmp"));
      CHECK(w.append(big.data(), big.size(), &err) == 0);
      CHECK(w.append(big.data(), 1, &err) != 0 && err.find("more payload bytes") != std::string::npos);
      CHECK(!exists(fn) && !exists(fn + ".tmp"));
      CHECK(w.finish(&err) != 0);
    }
    {   // fewer bytes than declared
      StreamWriter w; err.clear();
      CHECK(w.open(fn.c_str(), some_info(), e, &err) == 0);
      CHECK(w.append(big.data(), 100, &err) == 0);
      CHECK(w.finish(&err) != 0 && err.find("fewer payload bytes") != std::string::npos);
      CHECK(!exists(fn) && !exists(fn + ".tmp"));
    }
    {   // a writer dropped half way
      StreamWriter w;
      CHECK(w.open(fn.c_str(), some_info(), e, &err) == 0 && w.append(big.data(), 100, &err) == 0);
    }
    CHECK(!exists(fn) && !exists(fn + ".tmp"));
    {   // the write itself fails (the file-size limit stands in for a full disk); the complete file from before stays
      CHECK(write_stream(fn, secs, &err) == 0);
      const std::vector<uint8_t> before = slurp(fn);
      struct rlimit old{}, lim{};
      getrlimit(RLIMIT_FSIZE, &old);
      signal(SIGXFSZ, SIG_IGN);
      lim = old; lim.rlim_cur = 8192;
      CHECK(setrlimit(RLIMIT_FSIZE, &lim) == 0);
      StreamWriter w; err.clear();
      int rc = w.open(fn.c_str(), some_info(), e, &err);
      CHECK(rc == 0);
      rc = rc || w.append(big.data(), big.size(), &err) || w.finish(&err);
      setrlimit(RLIMIT_FSIZE, &old);
      CHECK(rc != 0 && err.find("short write to " + fn + ".tmp") != std::string::npos);
      CHECK(!exists(fn + ".tmp") && slurp(fn) == before);
      remove(fn.c_str());
    }
    {   // a directory that does not exist
      StreamWriter w; err.clear();
      CHECK(w.open((dir + "/no/such/dir/x.bin").c_str(), some_info(), e, &err) != 0 && err.find("cannot open") != std::string::npos);
    }
  }
  if (g_fail) return 1;
  printf("state stream host OK\n");
  return 0;
}
