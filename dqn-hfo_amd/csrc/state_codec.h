// state_codec.h — the learner-state file's container and its manifest, the ordered list of a file's sections (DESIGN.md 9 has the
// byte layout): what learner_state.hip and learner_save_async.hip need of state_codec.cpp.  Host code only; not installed, not
// part of the C-ABI.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/dqnhip.h"
#include "state_image.h"          // kRingArrays

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

// ---- the manifest: which sections a learner's file holds, in which order, each of how many bytes.  The one description of the
// file's composition in the code: both savers walk it, the load takes every expected size from it ----
// the eight parameter sections, in file order: W of the four nets, then (history 1, history 2) of each online net
constexpr int kParSections = 8;
constexpr uint32_t kTagPar[kParSections] = {kTagW[0], kTagW[1], kTagW[2], kTagW[3], kTagM[0], kTagV[0], kTagM[1], kTagV[1]};
constexpr int par_net(int i) { return i < 4 ? i : (i - 4) / 2; }
constexpr int par_kind(int i) { return i < 4 ? DQNHIP_KIND_W : (i - 4) % 2 ? DQNHIP_KIND_V : DQNHIP_KIND_M; }
// the ring's arrays (state_image.h: kRingArrays), logical order, dense rows.  per_row 0: state_size elements
struct RingArrayDesc { uint32_t tag, elem_bytes; int32_t per_row; };
constexpr RingArrayDesc kRingArray[kRingArrays] = {{kTagStates, 4, 0}, {kTagNext, 4, 0}, {kTagAct, 4, DQNHIP_ACTOR_OUT}, {kTagReward, 4, 1},
                                                   {kTagMc, 4, 1}, {kTagTerm, 1, 1}, {kTagPerLeaves, 4, 1}};
constexpr int ring_arrays(bool has_per) { return has_per ? kRingArrays : kRingArrays - 1; }      // the leaves: a prioritized learner's
constexpr uint32_t ring_width(int i, int state_size) { return (uint32_t)(kRingArray[i].per_row ? kRingArray[i].per_row : state_size); }
constexpr uint32_t ring_row_bytes(int i, int state_size) { return ring_width(i, state_size) * kRingArray[i].elem_bytes; }

// what a learner's file contains
struct StateShape {
  uint64_t dense[4] = {0, 0, 0, 0};      // float count of each net's dense parameters
  int32_t state_size = 0;
  bool has_solver = false, has_lr = false, has_loss_scale = false, with_memory = false, has_per = false;   // has_per: only with_memory
  int32_t ring_size = 0;
  uint64_t user_bytes = 0;
};
// where a section's bytes come from: parameter section `index`, ring array `index`, or one of the fixed structs
enum class Src { Par, RingArray, Solver, Lr, Dev, LossScale, Host, Ring, PerCfg, User };
struct ManifestEntry { uint32_t tag; uint64_t bytes; Src src; int index; };
std::vector<ManifestEntry> manifest(const StateShape& s);
// the fixed structs of one save (and the caller's user bytes), by source
struct FixedSections {
  SolverSection solver{}; LrSection lr{}; DevSection dev{}; LossScaleSection ls{}; HostSection host{}; RingSection ring{}; PerSection per{};
  const void* user = nullptr;
  const void* of(Src s) const;
};
// the header of a learner's file: its config, and the three values only the device knows
dqnhip_state_info_t info_of(const dqnhip_config& c, int32_t flags, const StateShape& s, int32_t actor_iter, int32_t critic_iter, uint64_t update_counter);
// empty, or why (head, size) is no window of a ring of `cap` slots
std::string ring_range_error(int head, int size, int cap);

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
