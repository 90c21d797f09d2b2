// state_codec.h — the learner-state file's container (DESIGN.md 9 has the byte layout): what learner_state.hip needs of
// state_codec.cpp.  Host code only; not installed, not part of the C-ABI.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/dqnhip.h"

namespace dqnhip_state {

constexpr uint32_t kVersion = 1;
constexpr size_t kHeaderBytes = 144, kEntryBytes = 24;
constexpr uint32_t kMaxSections = 64;

constexpr uint32_t tag4(char a, char b, char c, char d) {
  return (uint32_t)(uint8_t)a | (uint32_t)(uint8_t)b << 8 | (uint32_t)(uint8_t)c << 16 | (uint32_t)(uint8_t)d << 24;
}
// parameter sections: dense Caffe order (dqnhip_get_params), float32.  WGT<net>, ADM<net> (history 1: Adam's m), ADV<net> (history 2: Adam's v)
constexpr uint32_t kTagW[4] = {tag4('W', 'G', 'T', '0'), tag4('W', 'G', 'T', '1'), tag4('W', 'G', 'T', '2'), tag4('W', 'G', 'T', '3')};
constexpr uint32_t kTagM[2] = {tag4('A', 'D', 'M', '0'), tag4('A', 'D', 'M', '1')};
constexpr uint32_t kTagV[2] = {tag4('A', 'D', 'V', '0'), tag4('A', 'D', 'V', '1')};
constexpr uint32_t kTagDev = tag4('D', 'E', 'V', 'S'), kTagLossScale = tag4('L', 'S', 'C', 'L'), kTagHost = tag4('H', 'O', 'S', 'T');
constexpr uint32_t kTagRing = tag4('R', 'I', 'N', 'G'), kTagStates = tag4('R', 'S', 'T', 'A'), kTagNext = tag4('R', 'N', 'X', 'T'),
                   kTagAct = tag4('R', 'A', 'C', 'T'), kTagReward = tag4('R', 'R', 'E', 'W'), kTagMc = tag4('R', 'M', 'C', 'T'),
                   kTagTerm = tag4('R', 'T', 'R', 'M');
constexpr uint32_t kTagSolver = tag4('S', 'O', 'L', 'V');      // written by a learner whose solver is not Adam, right behind ADV1
constexpr uint32_t kTagLrSched = tag4('L', 'R', 'S', 'C');     // written by a learner with an lr policy or a weight decay, behind ADV1 / SOLV
constexpr uint32_t kTagPerCfg = tag4('P', 'E', 'R', 'C'), kTagPerLeaves = tag4('P', 'E', 'R', 'L'), kTagUser = tag4('U', 'S', 'E', 'R');

// the fixed-size sections, as they lie in the file (little endian, no padding inside)
struct DevSection { int32_t actor_iter, critic_iter; uint64_t update_counter; float critic_loss, avg_q; int32_t flags, skipped_steps; };
struct LossScaleSection { float mult[2]; int32_t good[2], backoffs[2], growths[2]; };      // [actor, critic]
struct HostSection { uint64_t sample_states_calls, seed; };
struct SolverSection { int32_t solver_type; float rms_decay; int32_t reserved[2]; };
// the words of LrSchedule (lr_schedule.hip.h), then the decay and its kind
struct LrSection { int32_t policy; float base_lr[2]; float gamma, power; int32_t stepsize, max_iter, n_stepvalue; int32_t stepvalue[16];
                   float weight_decay; int32_t regularization_type; };
struct RingSection { int32_t ring_head, ring_size; };
struct PerSection { float alpha, beta0; int32_t beta_anneal_iters; float eps; uint64_t seed; float p_max; int32_t reserved; int64_t syncs; };
static_assert(sizeof(SolverSection) == 16, "SOLV is 16 bytes");
static_assert(sizeof(LrSection) == 104, "LRSC is 104 bytes");
static_assert(sizeof(DevSection) == 32 && sizeof(LossScaleSection) == 32 && sizeof(HostSection) == 16 && sizeof(RingSection) == 8 &&
              sizeof(PerSection) == 40, "the sections have no padding");

struct Section { uint32_t tag; const void* data; uint64_t bytes; };
struct Entry { uint32_t tag, crc; uint64_t offset, bytes; };

std::string tag_name(uint32_t tag);

// Writes header, table and the sections back to back into filename + ".tmp" and renames it over filename.  info: every field the
// header stores except user_bytes and file_bytes, which are derived here.  On failure *err says why and filename is untouched.
int write_file(const char* filename, const dqnhip_state_info_t& info, const std::vector<Section>& sections, std::string* err);

// The same file, streamed: header and table first — every section's CRC and size are known before its bytes arrive — then the
// payload in table order, in pieces of any size, then the flush and rename of write_file.  open/append/finish return 0 or set *err;
// a failure (and a writer dropped before finish) removes the ".tmp" and leaves filename untouched.  write_file is built on it.
struct StreamEntry { uint32_t tag, crc; uint64_t bytes; };
class StreamWriter {
 public:
  StreamWriter() = default;
  StreamWriter(const StreamWriter&) = delete;
  StreamWriter& operator=(const StreamWriter&) = delete;
  ~StreamWriter() { abort(); }
  int open(const char* filename, const dqnhip_state_info_t& info, const std::vector<StreamEntry>& entries, std::string* err);
  int append(const void* data, uint64_t bytes, std::string* err);
  int finish(std::string* err);
  void abort();
 private:
  std::string fn_, tmp_;
  FILE* f_ = nullptr;
  uint64_t left_ = 0;            // payload bytes the table declares and append has not seen yet
};
uint32_t crc32_of(const void* p, uint64_t n);      // zlib's, over any length

struct Parsed {
  dqnhip_state_info_t info{};
  std::vector<Entry> table;
  std::vector<uint8_t> file;       // the whole file (keep = true)
  const Entry* find(uint32_t tag) const { for (const Entry& e : table) if (e.tag == tag) return &e; return nullptr; }
  const uint8_t* at(const Entry* e) const { return file.data() + e->offset; }
};
// Reads and validates: magic, version, header CRC; the table's CRC and the section bounds; every section's CRC.  keep: the file
// stays in out->file (dqnhip_load_state); else the sections are streamed through the CRC only.
int read_file(const char* filename, Parsed* out, bool keep, std::string* err);

}  // namespace dqnhip_state
