// state_codec.cpp — the container of the native learner-state file (dqnhip_save_state / dqnhip_load_state): header, section
// table, CRC-32 of everything, and the two entry points that need no GPU (dqnhip_state_info, dqnhip_state_read_user).
// DESIGN.md 9 has the byte layout; tests/state_ref.py is an independent reader / writer of it.  No device code here.
#include "state_codec.h"

#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <cerrno>
#include <cstddef>
#include <cstdio>
#include <cstring>

extern "C" int dqnhip_internal_set_error(const char* msg);

namespace dqnhip_state {

namespace {

const char kMagic[8] = {'D', 'Q', 'N', 'H', 'I', 'P', 'S', 'T'};

// little-endian fields at fixed offsets (the hosts this library runs on are little endian: memcpy is the codec)
template <class T> void put(uint8_t* p, size_t off, T v) { memcpy(p + off, &v, sizeof v); }
template <class T> T get(const uint8_t* p, size_t off) { T v; memcpy(&v, p + off, sizeof v); return v; }

uint32_t crc_of(const void* p, uint64_t n) {
  uint32_t c = (uint32_t)crc32(0L, Z_NULL, 0);
  const uint8_t* b = (const uint8_t*)p;
  while (n > 0) {                                   // (zlib's length is 32 bits)
    const uInt k = (uInt)(n > (1u << 30) ? (1u << 30) : n);
    c = (uint32_t)crc32(c, b, k); b += k; n -= k;
  }
  return c;
}

// header offsets
enum : size_t { oMagic = 0, oVersion = 8, oHeaderBytes = 12, oFlags = 16, oPrecision = 20, oMinibatch = 24, oStateSize = 28, oNumHidden = 32,
                oHidden = 36, oCapacity = 68, oMemorySize = 72, oActorIter = 76, oCriticIter = 80, oHasMemory = 84, oHasPer = 88,
                oHasLossScale = 92, oSections = 96, oReserved = 100, oSeed = 104, oUpdateCounter = 112, oUserBytes = 120, oFileBytes = 128 };
// ... and the two CRCs close the header
constexpr size_t oTableCrc = 136, oHeaderCrc = 140, kHeaderTotal = kHeaderBytes;

int set(std::string* err, const std::string& m) { if (err) *err = m; return 1; }

}  // namespace

std::string tag_name(uint32_t tag) {
  std::string s(4, '?');
  for (int i = 0; i < 4; ++i) { const char c = (char)(tag >> (8 * i)); s[i] = (c >= 32 && c < 127) ? c : '?'; }
  return s;
}

namespace {

// header + section table of a file whose sections are `e` (tag, crc, bytes), packed back to back behind the table
std::vector<uint8_t> build_head(const dqnhip_state_info_t& info, const std::vector<StreamEntry>& e) {
  const uint32_t n = (uint32_t)e.size();
  std::vector<uint8_t> head(kHeaderTotal + (size_t)n * kEntryBytes, 0);
  uint64_t off = head.size(), user_bytes = 0;
  for (uint32_t i = 0; i < n; ++i) {
    uint8_t* t = head.data() + kHeaderTotal + (size_t)i * kEntryBytes;
    put<uint32_t>(t, 0, e[i].tag); put<uint32_t>(t, 4, e[i].crc);
    put<uint64_t>(t, 8, off); put<uint64_t>(t, 16, e[i].bytes);
    off += e[i].bytes;
    if (e[i].tag == kTagUser) user_bytes = e[i].bytes;
  }
  uint8_t* h = head.data();
  memcpy(h + oMagic, kMagic, 8);
  put<uint32_t>(h, oVersion, kVersion); put<uint32_t>(h, oHeaderBytes, (uint32_t)kHeaderTotal);
  put<int32_t>(h, oFlags, info.flags); put<int32_t>(h, oPrecision, info.precision); put<int32_t>(h, oMinibatch, info.minibatch);
  put<int32_t>(h, oStateSize, info.state_size); put<int32_t>(h, oNumHidden, info.num_hidden);
  for (int i = 0; i < DQNHIP_MAX_HIDDEN; ++i) put<int32_t>(h, oHidden + 4 * i, info.hidden[i]);
  put<int32_t>(h, oCapacity, info.replay_capacity); put<int32_t>(h, oMemorySize, info.memory_size);
  put<int32_t>(h, oActorIter, info.actor_iter); put<int32_t>(h, oCriticIter, info.critic_iter);
  put<int32_t>(h, oHasMemory, info.has_memory); put<int32_t>(h, oHasPer, info.has_per); put<int32_t>(h, oHasLossScale, info.has_loss_scale);
  put<uint32_t>(h, oSections, n); put<uint32_t>(h, oReserved, 0);
  put<uint64_t>(h, oSeed, info.seed); put<uint64_t>(h, oUpdateCounter, info.update_counter);
  put<uint64_t>(h, oUserBytes, user_bytes); put<uint64_t>(h, oFileBytes, off);
  put<uint32_t>(h, oTableCrc, crc_of(h + kHeaderTotal, (uint64_t)n * kEntryBytes));
  put<uint32_t>(h, oHeaderCrc, crc_of(h, oHeaderCrc));
  return head;
}

}  // namespace

uint32_t crc32_of(const void* p, uint64_t n) { return crc_of(p, n); }

std::vector<ManifestEntry> manifest(const StateShape& s) {
  std::vector<ManifestEntry> m;
  for (int i = 0; i < kParSections; ++i) m.push_back({kTagPar[i], s.dense[par_net(i)] * sizeof(float), Src::Par, i});
  // a learner whose solver is not Adam says so, and so does one with an lr policy or a weight decay: without either, the file is
  // byte for byte what it was before those existed
  if (s.has_solver) m.push_back({kTagSolver, sizeof(SolverSection), Src::Solver, 0});
  if (s.has_lr) m.push_back({kTagLrSched, sizeof(LrSection), Src::Lr, 0});
  m.push_back({kTagDev, sizeof(DevSection), Src::Dev, 0});
  if (s.has_loss_scale) m.push_back({kTagLossScale, sizeof(LossScaleSection), Src::LossScale, 0});
  m.push_back({kTagHost, sizeof(HostSection), Src::Host, 0});
  if (s.with_memory) {
    m.push_back({kTagRing, sizeof(RingSection), Src::Ring, 0});
    for (int i = 0; i < ring_arrays(s.has_per); ++i) {
      if (kRingArray[i].tag == kTagPerLeaves) m.push_back({kTagPerCfg, sizeof(PerSection), Src::PerCfg, 0});      // the leaves follow their PERC
      m.push_back({kRingArray[i].tag, (uint64_t)s.ring_size * ring_row_bytes(i, s.state_size), Src::RingArray, i});
    }
  }
  if (s.user_bytes) m.push_back({kTagUser, s.user_bytes, Src::User, 0});
  return m;
}

const void* FixedSections::of(Src s) const {
  const void* const by_src[] = {nullptr, nullptr, &solver, &lr, &dev, &ls, &host, &ring, &per, user};      // Src's order; Par, RingArray: the saver's own bytes
  return by_src[(int)s];
}

dqnhip_state_info_t info_of(const dqnhip_config& c, int32_t flags, const StateShape& s, int32_t actor_iter, int32_t critic_iter, uint64_t update_counter) {
  dqnhip_state_info_t info{};
  info.struct_size = (int32_t)sizeof info; info.version = (int32_t)kVersion; info.flags = flags;
  info.precision = c.precision; info.minibatch = c.minibatch; info.state_size = c.state_size; info.num_hidden = c.num_hidden;
  for (int i = 0; i < c.num_hidden; ++i) info.hidden[i] = c.hidden[i];
  info.replay_capacity = c.replay_capacity; info.memory_size = s.with_memory ? s.ring_size : 0;
  info.actor_iter = actor_iter; info.critic_iter = critic_iter;
  info.has_memory = s.with_memory; info.has_per = s.with_memory && s.has_per; info.has_loss_scale = s.has_loss_scale;
  info.seed = c.seed; info.update_counter = update_counter;
  return info;
}

std::string ring_range_error(int head, int size, int cap) {
  if (head >= 0 && head < cap && size >= 0 && size <= cap) return "";
  return "the ring's (head, size) = (" + std::to_string(head) + ", " + std::to_string(size) + ") is outside its capacity " + std::to_string(cap);
}

int write_file(const char* filename, const dqnhip_state_info_t& info, const std::vector<Section>& sections, std::string* err) {
  if (sections.size() > kMaxSections) return set(err, std::string(filename) + ": too many sections");
  std::vector<StreamEntry> e;
  for (const Section& s : sections) e.push_back({s.tag, crc_of(s.data, s.bytes), s.bytes});
  StreamWriter w;
  if (w.open(filename, info, e, err)) return 1;
  for (const Section& s : sections)
    if (w.append(s.data, s.bytes, err)) return 1;
  return w.finish(err);
}

int StreamWriter::open(const char* filename, const dqnhip_state_info_t& info, const std::vector<StreamEntry>& entries, std::string* err) {
  abort();
  fn_ = filename; tmp_ = fn_ + ".tmp";
  if (entries.size() > kMaxSections) return set(err, fn_ + ": too many sections");
  const std::vector<uint8_t> head = build_head(info, entries);
  left_ = 0;
  for (const StreamEntry& e : entries) left_ += e.bytes;
  f_ = fopen(tmp_.c_str(), "wb");
  if (!f_) return set(err, "cannot open " + tmp_ + " for writing: " + strerror(errno));
  if (fwrite(head.data(), 1, head.size(), f_) != head.size()) { const std::string why = strerror(errno); abort(); return set(err, "short write to " + tmp_ + ": " + why); }
  return 0;
}

int StreamWriter::append(const void* data, uint64_t bytes, std::string* err) {
  if (!f_) return set(err, fn_ + ": append without an open file");
  if (bytes > left_) { abort(); return set(err, fn_ + ": more payload bytes than the section table declares"); }
  if (bytes && fwrite(data, 1, bytes, f_) != bytes) { const std::string why = strerror(errno); abort(); return set(err, "short write to " + tmp_ + ": " + why); }
  left_ -= bytes;
  return 0;
}

int StreamWriter::finish(std::string* err) {
  if (!f_) return set(err, fn_ + ": finish without an open file");
  if (left_) { abort(); return set(err, fn_ + ": fewer payload bytes than the section table declares"); }
  bool ok = fflush(f_) == 0;
  ok = fsync(fileno(f_)) == 0 && ok;                // (the rename below must not overtake the data on its way to the disk)
  ok = fclose(f_) == 0 && ok;
  f_ = nullptr;
  if (!ok) { const std::string why = strerror(errno); remove(tmp_.c_str()); return set(err, "short write to " + tmp_ + ": " + why); }
  if (rename(tmp_.c_str(), fn_.c_str()) != 0) { const std::string why = strerror(errno); remove(tmp_.c_str()); return set(err, "rename " + tmp_ + " -> " + fn_ + " failed: " + why); }
  return 0;
}

void StreamWriter::abort() {
  if (!f_) return;
  fclose(f_); f_ = nullptr;
  remove(tmp_.c_str());
}

// the SOLV section -> the info's solver fields (a file without one is an Adam learner's: both stay 0)
static int solver_of(const uint8_t* p, uint64_t bytes, dqnhip_state_info_t* in, const std::string& fn, std::string* err) {
  SolverSection s;
  if (bytes != sizeof s) return set(err, fn + ": section SOLV holds " + std::to_string(bytes) + " bytes, expected " + std::to_string(sizeof s));
  memcpy(&s, p, sizeof s);
  if (s.solver_type <= DQNHIP_SOLVER_ADAM || s.solver_type > DQNHIP_SOLVER_ADADELTA)
    return set(err, fn + ": section SOLV names solver " + std::to_string(s.solver_type) + " (an Adam learner writes no SOLV section; the others are 1 .. 5)");
  in->solver_type = s.solver_type; in->rms_decay = s.rms_decay;
  return 0;
}

int read_file(const char* filename, Parsed* out, bool keep, std::string* err) {
  const std::string fn(filename);
  FILE* f = fopen(filename, "rb");
  if (!f) return set(err, fn + ": cannot open: " + strerror(errno));
  struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
  struct stat sb;
  if (fstat(fileno(f), &sb) != 0 || !S_ISREG(sb.st_mode)) return set(err, fn + ": not a regular file");
  const uint64_t size = (uint64_t)sb.st_size;
  uint8_t h[kHeaderTotal];
  const size_t got = fread(h, 1, sizeof h, f);
  if (got < 8 || memcmp(h, kMagic, 8) != 0) return set(err, fn + ": bad magic (not a learner-state file)");
  if (got < 12) return set(err, fn + ": truncated inside the header (" + std::to_string(size) + " bytes)");
  const uint32_t version = get<uint32_t>(h, oVersion);
  if (version != kVersion) return set(err, fn + ": unknown format version " + std::to_string(version) + " (this library reads version " + std::to_string(kVersion) + ")");
  if (got < sizeof h) return set(err, fn + ": truncated inside the header (" + std::to_string(size) + " bytes)");
  if (get<uint32_t>(h, oHeaderCrc) != crc_of(h, oHeaderCrc)) return set(err, fn + ": header CRC mismatch");
  const uint32_t n = get<uint32_t>(h, oSections);
  if (get<uint32_t>(h, oHeaderBytes) != kHeaderTotal || n > kMaxSections) return set(err, fn + ": bad header (header size / section count)");
  dqnhip_state_info_t& in = out->info;
  memset(&in, 0, sizeof in);
  in.struct_size = (int32_t)sizeof in; in.version = (int32_t)version;
  in.flags = get<int32_t>(h, oFlags); in.precision = get<int32_t>(h, oPrecision); in.minibatch = get<int32_t>(h, oMinibatch);
  in.state_size = get<int32_t>(h, oStateSize); in.num_hidden = get<int32_t>(h, oNumHidden);
  for (int i = 0; i < DQNHIP_MAX_HIDDEN; ++i) in.hidden[i] = get<int32_t>(h, oHidden + 4 * i);
  in.replay_capacity = get<int32_t>(h, oCapacity); in.memory_size = get<int32_t>(h, oMemorySize);
  in.actor_iter = get<int32_t>(h, oActorIter); in.critic_iter = get<int32_t>(h, oCriticIter);
  in.has_memory = get<int32_t>(h, oHasMemory); in.has_per = get<int32_t>(h, oHasPer); in.has_loss_scale = get<int32_t>(h, oHasLossScale);
  in.seed = get<uint64_t>(h, oSeed); in.update_counter = get<uint64_t>(h, oUpdateCounter);
  in.user_bytes = get<uint64_t>(h, oUserBytes); in.file_bytes = get<uint64_t>(h, oFileBytes);
  // the table
  const uint64_t table_bytes = (uint64_t)n * kEntryBytes;
  if (size < kHeaderTotal + table_bytes) return set(err, fn + ": truncated inside the section table (" + std::to_string(size) + " bytes)");
  std::vector<uint8_t> tb(table_bytes);
  if (table_bytes && fread(tb.data(), 1, table_bytes, f) != table_bytes) return set(err, fn + ": truncated inside the section table");
  if (get<uint32_t>(h, oTableCrc) != crc_of(tb.data(), table_bytes)) return set(err, fn + ": section table CRC mismatch");
  out->table.resize(n);
  uint64_t expect = kHeaderTotal + table_bytes;
  for (uint32_t i = 0; i < n; ++i) {
    Entry& e = out->table[i];
    const uint8_t* p = tb.data() + (size_t)i * kEntryBytes;
    e.tag = get<uint32_t>(p, 0); e.crc = get<uint32_t>(p, 4); e.offset = get<uint64_t>(p, 8); e.bytes = get<uint64_t>(p, 16);
    for (uint32_t j = 0; j < i; ++j) if (out->table[j].tag == e.tag) return set(err, fn + ": section " + tag_name(e.tag) + " appears twice");
    if (e.offset > in.file_bytes || e.bytes > in.file_bytes - e.offset)
      return set(err, fn + ": section " + tag_name(e.tag) + " runs past the end of the file (offset " + std::to_string(e.offset) + " + " +
                      std::to_string(e.bytes) + " bytes > " + std::to_string(in.file_bytes) + ")");
    if (e.offset != expect) return set(err, fn + ": section " + tag_name(e.tag) + " does not follow its predecessor (offset " + std::to_string(e.offset) +
                                            ", expected " + std::to_string(expect) + ")");
    expect += e.bytes;
  }
  if (expect != in.file_bytes) return set(err, fn + ": bad header (file_bytes " + std::to_string(in.file_bytes) + " != end of the last section " + std::to_string(expect) + ")");
  if (size != in.file_bytes) return set(err, fn + ": " + (size < in.file_bytes ? "truncated" : "trailing bytes") + " (" + std::to_string(size) +
                                             " bytes, the header says " + std::to_string(in.file_bytes) + ")");
  // the sections
  if (keep) {
    out->file.resize(size);
    memcpy(out->file.data(), h, sizeof h);
    if (table_bytes) memcpy(out->file.data() + kHeaderTotal, tb.data(), table_bytes);
    const uint64_t rest = size - (kHeaderTotal + table_bytes);
    if (rest && fread(out->file.data() + kHeaderTotal + table_bytes, 1, rest, f) != rest) return set(err, fn + ": truncated (short read)");
    for (const Entry& e : out->table)
      if (crc_of(out->file.data() + e.offset, e.bytes) != e.crc) return set(err, fn + ": section " + tag_name(e.tag) + " CRC mismatch");
    if (const Entry* sv = out->find(kTagSolver))
      if (solver_of(out->file.data() + sv->offset, sv->bytes, &in, fn, err)) return 1;
  } else {
    std::vector<uint8_t> buf(1 << 20);
    for (const Entry& e : out->table) {                     // (contiguous, in table order: one pass)
      uint32_t c = (uint32_t)crc32(0L, Z_NULL, 0);
      for (uint64_t left = e.bytes; left > 0;) {
        const size_t k = (size_t)(left < buf.size() ? left : buf.size());
        if (fread(buf.data(), 1, k, f) != k) return set(err, fn + ": truncated (short read in section " + tag_name(e.tag) + ")");
        c = (uint32_t)crc32(c, buf.data(), (uInt)k); left -= k;
      }
      if (c != e.crc) return set(err, fn + ": section " + tag_name(e.tag) + " CRC mismatch");
      if (e.tag == kTagSolver && solver_of(buf.data(), e.bytes, &in, fn, err)) return 1;      // (16 bytes: the one piece just read)
    }
  }
  const Entry* u = out->find(kTagUser);
  if ((u ? u->bytes : 0) != in.user_bytes) return set(err, fn + ": bad header (user_bytes does not match the USER section)");
  return 0;
}

}  // namespace dqnhip_state

using namespace dqnhip_state;

extern "C" {

int dqnhip_state_info(const char* filename, dqnhip_state_info_t* out) {
  if (!filename || !out) return dqnhip_internal_set_error("dqnhip_state_info: null argument");
  // the struct as it is, or as it was before solver_type / rms_decay were appended (a caller compiled against that header: it gets
  // the fields it knows, under its own struct_size)
  const int32_t asked = out->struct_size;
  const int32_t before_solver = (int32_t)offsetof(dqnhip_state_info_t, solver_type);
  if (asked != (int32_t)sizeof(dqnhip_state_info_t) && asked != before_solver)
    return dqnhip_internal_set_error(("dqnhip_state_info_t.struct_size " + std::to_string(out->struct_size) + " != " + std::to_string(sizeof(dqnhip_state_info_t)) + " (ABI mismatch)").c_str());
  Parsed p; std::string err;
  if (read_file(filename, &p, false, &err)) return dqnhip_internal_set_error(err.c_str());
  memcpy(out, &p.info, (size_t)asked);
  out->struct_size = asked;
  return 0;
}

int dqnhip_state_read_user(const char* filename, void* buf, size_t cap, size_t* n_out) {
  if (!filename || !n_out || (!buf && cap)) return dqnhip_internal_set_error("dqnhip_state_read_user: null argument");
  *n_out = 0;
  Parsed p; std::string err;
  if (read_file(filename, &p, false, &err)) return dqnhip_internal_set_error(err.c_str());
  const Entry* u = p.find(kTagUser);
  if (!u || u->bytes == 0) return 0;
  *n_out = (size_t)u->bytes;
  if (u->bytes > cap) return dqnhip_internal_set_error((std::string(filename) + ": the user section holds " + std::to_string(u->bytes) + " bytes, the buffer " + std::to_string(cap)).c_str());
  FILE* f = fopen(filename, "rb");
  if (!f) return dqnhip_internal_set_error((std::string(filename) + ": cannot open").c_str());
  const bool ok = fseeko(f, (off_t)u->offset, SEEK_SET) == 0 && fread(buf, 1, u->bytes, f) == u->bytes;
  fclose(f);
  if (!ok || (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)buf, (uInt)u->bytes) != u->crc)
    return dqnhip_internal_set_error((std::string(filename) + ": section USER CRC mismatch").c_str());
  return 0;
}

}  // extern "C"
