// learner_state.hip — dqnhip_save_state / dqnhip_load_state: the native learner-state file (include/dqnhip.h; DESIGN.md 9 has the
// byte layout, state_codec.cpp the container).  Host only: copies between the learner's device state and the file's sections, no
// kernel of its own — the one launch a load may need, the priority tree's set pass, goes through per_restore (learner_io.hip).
// dqnhip_save_state_async: the same file behind training.  The caller's thread enqueues the pack and the chunk CRCs on the learner's
// stream (state_kernels.hip.h, launched from learner_io.hip) and hands a job to the learner's writer thread, which waits for the
// event, folds the CRCs, and streams the staging buffer to the file through two pinned chunks.
// dqnhip_snapshot_async: the Caffe snapshot's files behind training, a second kind of job for the same writer thread.  The caller's
// thread enqueues the parameter pack, the `.replaymemory` stream (snapshot_kernels.hip.h) and its CRC into a staging buffer of the
// snapshot's own; the writer builds the protobuf files with snapshot.cpp's builders and hands the stream to GzipParallelWriter.
#include <condition_variable>
#include <memory>

#include "learner_internal.hip.h"
#include "gzip_parallel.h"
#include "snapshot_codec.h"
#include "snapshot_stream.h"
#include "state_codec.h"

using namespace dqnhip_state;

namespace {

// v1's limits, the same for save and load
int state_refuse(const H* h, const char* what) {
  if (h->ring_owner || h->ring_shared) return fail("%s: a learner that shares a replay memory (dqnhip_share_replay_memory) is not supported in this version", what);
  if (h->w_owner || h->sharers) return fail("%s: a learner that shares parameters or is shared from (dqnhip_share_parameters) is not supported in this version", what);
  if (h->cfg.dp_world > 1 || h->comm || h->dp_half || h->dp_shard) return fail("%s: a data-parallel learner (dp_world > 1, dqnhip_dp_init) is not supported in this version", what);
  if (h->next_phase != 0) return fail("%s: a phased update is in progress (next phase %d)", what, h->next_phase);
  if (h->timing) return fail("%s: kernel timing is on (dqnhip_set_kernel_timing)", what);
  return 0;
}

// the LRSC section of a learner: its schedule's words (only the stepvalues in use: what lies behind them is not the learner's), decay, kind
LrSection lr_section_of(const dqnhip_config& c) {
  const LrSchedule s = schedule_of(c);
  LrSection o{};
  o.policy = s.policy; o.base_lr[0] = s.base_lr[0]; o.base_lr[1] = s.base_lr[1]; o.gamma = s.gamma; o.power = s.power;
  o.stepsize = s.stepsize; o.max_iter = s.max_iter; o.n_stepvalue = s.n_stepvalue;
  for (int i = 0; i < s.n_stepvalue && i < kLrMaxStepvalues; ++i) o.stepvalue[i] = s.stepvalue[i];
  o.weight_decay = c.weight_decay; o.regularization_type = c.regularization_type;
  return o;
}

// the window [head, head + size) of a ring array with rows of `width` bytes at a pitch of `pitch` bytes <-> dense host rows, logical order
int window_copy(const H* h, void* dev, size_t pitch, void* host, size_t width, int head, int size, bool to_host) {
  const int cap = h->ring.cap;
  const int n0 = std::min(size, cap - head);
  for (int piece = 0; piece < 2; ++piece) {
    const int first = piece ? 0 : head, rows = piece ? size - n0 : n0, done = piece ? n0 : 0;
    if (rows <= 0) continue;
    char* d = (char*)dev + (size_t)first * pitch; char* s = (char*)host + (size_t)done * width;
    if (pitch == width) {                          // dense on both sides: one linear copy
      if (to_host) HIPCHK(hipMemcpy(s, d, (size_t)rows * width, hipMemcpyDeviceToHost));
      else HIPCHK(hipMemcpy(d, s, (size_t)rows * width, hipMemcpyHostToDevice));
    }
    else if (to_host) HIPCHK(hipMemcpy2D(s, width, d, pitch, width, (size_t)rows, hipMemcpyDeviceToHost));
    else HIPCHK(hipMemcpy2D(d, pitch, s, width, width, (size_t)rows, hipMemcpyHostToDevice));
  }
  return 0;
}

}  // namespace

// ---- the asynchronous save ------------------------------------------------------------------------------------------------------
namespace dqnhip_host {

constexpr size_t kPinnedChunk = (size_t)8 << 20;       // the pinned ring: two of these

// what one save needs besides the staging buffer: fixed on the caller's thread, read by the writer
struct StateJob {
  std::string filename;
  int32_t flags = 0;
  bool with_mem = false, has_per = false, has_ls = false;
  std::vector<uint8_t> user;
  HostSection host{};
  bool has_solver = false; SolverSection solver{};      // a learner whose solver is not Adam
  bool has_lr = false; LrSection lr{};                  // a learner with an lr policy or a weight decay
  PerSection per{};                      // p_max comes from the record
  dqnhip_state_info_t info{};            // the config's share; the record fills the rest
  int device = 0, cap = 0;
};

// what one asynchronous snapshot needs besides its staging buffer
struct SnapJob {
  std::string save_path, prefix;
  bool remove_old = false, with_mem = false, two = false;   // two: the solver keeps a second history set
  int workers = 8;
  dqnhip_config cfg{};
  int device = 0, cap = 0, S = 0;
};
constexpr int kSnapPar = 6;              // W actor, W critic, history 1 / 2 of the actor, history 1 / 2 of the critic
struct SnapAsync {
  // device side, allocated by the first asynchronous snapshot and kept until dqnhip_destroy: the snapshot's own staging buffer
  uint8_t* stage = nullptr; size_t stage_bytes = 0;
  hipEvent_t ev = nullptr;
  // its map: the record, the segment table, the chunk CRCs of the records, the dense parameters, the stream (its records start on a
  // 16-byte boundary: the count sits in the 4 bytes before one), the guard band behind the stream's upper bound
  size_t off_rec = 0, off_segs = 0, off_crc = 0, off_par[kSnapPar] = {0}, off_stream = 0, off_guard = 0;
  size_t par_bytes[kSnapPar] = {0};
  int n_seg = 0;
  std::vector<PackSeg> segs;
  SnapJob job;
  int32_t actor_iter = 0, critic_iter = 0;       // of the last job that wrote its files
};

enum JobKind { kJobState = 0, kJobSnapshot = 1, kJobKinds = 2 };
const char* const kJobWhat[kJobKinds] = {"save", "snapshot"};

struct StateAsync {
  // the learner-state save's device side, allocated by the first asynchronous save and kept until dqnhip_destroy (null: this learner
  // has only snapshotted asynchronously)
  uint8_t* stage = nullptr; size_t stage_bytes = 0;
  hipEvent_t ev = nullptr;
  // what both kinds of job share, allocated with the writer thread by whichever comes first
  uint8_t* pinned = nullptr;
  hipStream_t copy_stream = nullptr;
  SnapAsync* snap = nullptr;             // dqnhip_snapshot_async's side, allocated by the first asynchronous snapshot
  // the staging buffer's map (byte offsets, every section on a 16-byte boundary)
  size_t off_rec = 0, off_segs = 0, off_crc = 0, off_par[8] = {0}, off_ring[kRingArrays] = {0};
  size_t par_bytes[8] = {0};
  uint32_t ring_row_bytes[kRingArrays] = {0};
  int n_seg = 0;
  std::vector<PackSeg> segs;             // (host copy of the table at off_segs: its upload reads it)
  CrcArgs crc{};                         // the launch of the save in flight (the writer reads chunk0 / the offsets)
  uint32_t chunk_tab[kCrcTableWords];    // crc_op_table of Z_kCrcChunk
  // the writer thread
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<int> queue;                 // the kinds of the jobs that wait for the thread, first in first out
  bool busy[kJobKinds] = {false, false}; // a job of this kind is in flight (waiting or being written): at most one of each
  bool quit = false;
  StateJob job;
  bool failed[kJobKinds] = {false, false}; std::string err[kJobKinds];   // of the last finished job of each kind, until a join reports it
};

}  // namespace dqnhip_host

namespace {

std::string hip_msg(const char* what, hipError_t e) { return std::string(what) + " failed: " + hipGetErrorString(e); }
#define WCHK(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { *err = hip_msg(#expr, e__); return 1; } } while (0)

// `bytes` bytes of a staging buffer at src -> dst (host memory of any kind), through the pinned ring
int fetch_dev(StateAsync* a, const uint8_t* src, size_t bytes, void* dst, std::string* err) {
  for (size_t done = 0; done < bytes;) {
    const size_t k = std::min(bytes - done, kPinnedChunk);
    WCHK(hipMemcpyAsync(a->pinned, src + done, k, hipMemcpyDeviceToHost, a->copy_stream));
    WCHK(hipStreamSynchronize(a->copy_stream));
    memcpy((char*)dst + done, a->pinned, k);
    done += k;
  }
  return 0;
}
// ... -> the file (StreamWriter, GzipParallelWriter): the copy of chunk k + 1 runs while chunk k is written
template <class Writer>
int stream_dev(StateAsync* a, const uint8_t* src, size_t bytes, Writer* w, std::string* err) {
  if (!bytes) return 0;
  int b = 0;
  size_t k = std::min(bytes, kPinnedChunk);
  WCHK(hipMemcpyAsync(a->pinned, src, k, hipMemcpyDeviceToHost, a->copy_stream));
  for (size_t done = 0; done < bytes;) {
    WCHK(hipStreamSynchronize(a->copy_stream));
    const size_t next = done + k, k_next = std::min(bytes - next, kPinnedChunk);
    if (k_next) WCHK(hipMemcpyAsync(a->pinned + (size_t)(b ^ 1) * kPinnedChunk, src + next, k_next, hipMemcpyDeviceToHost, a->copy_stream));
    if (w->append(a->pinned + (size_t)b * kPinnedChunk, k, err)) return 1;
    done = next; k = k_next; b ^= 1;
  }
  return 0;
}

// The writer thread's share of one save.  Nothing here allocates through HIP or touches the learner: the staging buffer, the job
// and the launch's CrcArgs are all it reads, its own copy stream all it waits for.
int write_job(StateAsync* a, std::string* err) {
  const StateJob& j = a->job;
  WCHK(hipSetDevice(j.device));
  // (the copy stream already waits for the save's event — dqnhip_save_state_async enqueued that wait: every copy below is behind the
  // pack and the CRC, and this thread touches neither the learner's stream nor an event recorded on it, which may be capturing by now)
  StateRec rec{};
  if (fetch_dev(a, a->stage + a->off_rec, sizeof rec, &rec, err)) return 1;
  const int head = rec.ring_head, size = rec.ring_size;
  if (j.with_mem && (head < 0 || head >= j.cap || size < 0 || size > j.cap)) {
    *err = "the ring's (head, size) = (" + std::to_string(head) + ", " + std::to_string(size) + ") is outside its capacity " + std::to_string(j.cap);
    return 1;
  }
  // the device-checksummed sections, in the launch's order: eight parameter sections, then the ring's arrays
  struct DevSec { size_t off; uint64_t bytes; uint32_t crc; };
  std::vector<DevSec> dev;
  std::vector<uint32_t> raws;
  for (int s = 0; s < a->crc.n; ++s) {
    const CrcSection& c = a->crc.sec[s];
    const uint64_t bytes = c.row_bytes ? (uint64_t)size * c.row_bytes : c.fixed_bytes;
    const size_t chunks = (size_t)((bytes + kCrcChunk - 1) / kCrcChunk);
    raws.resize(chunks);
    if (fetch_dev(a, a->stage + a->off_crc + (size_t)c.chunk0 * sizeof(uint32_t), chunks * sizeof(uint32_t), raws.data(), err)) return 1;
    dev.push_back({(size_t)c.off, bytes, crc_fold_chunks(raws.data(), bytes, a->chunk_tab)});
  }
  // the host-built sections
  const DevSection devs{rec.actor_iter, rec.critic_iter, rec.update_counter, rec.critic_loss, rec.avg_q, rec.flags, rec.skipped_steps};
  const LossScaleSection ls{{rec.ls_mult[0], rec.ls_mult[1]}, {rec.ls_good[0], rec.ls_good[1]}, {rec.ls_backoffs[0], rec.ls_backoffs[1]},
                            {rec.ls_growths[0], rec.ls_growths[1]}};
  const RingSection ring{head, size};
  PerSection per = j.per; per.p_max = rec.p_max;
  // the file's sections in dqnhip_save_state's order; dev_ix >= 0: the bytes are in the staging buffer
  struct Out { uint32_t tag; int dev_ix; const void* host; uint64_t bytes; };
  std::vector<Out> out;
  for (int net = 0; net < 4; ++net) out.push_back({kTagW[net], net, nullptr, 0});
  for (int net = 0; net < 2; ++net) { out.push_back({kTagM[net], 4 + 2 * net, nullptr, 0}); out.push_back({kTagV[net], 5 + 2 * net, nullptr, 0}); }
  if (j.has_solver) out.push_back({kTagSolver, -1, &j.solver, sizeof j.solver});
  if (j.has_lr) out.push_back({kTagLrSched, -1, &j.lr, sizeof j.lr});
  out.push_back({kTagDev, -1, &devs, sizeof devs});
  if (j.has_ls) out.push_back({kTagLossScale, -1, &ls, sizeof ls});
  out.push_back({kTagHost, -1, &j.host, sizeof j.host});
  if (j.with_mem) {
    static const uint32_t kRingTags[6] = {kTagStates, kTagNext, kTagAct, kTagReward, kTagMc, kTagTerm};
    out.push_back({kTagRing, -1, &ring, sizeof ring});
    for (int i = 0; i < 6; ++i) out.push_back({kRingTags[i], 8 + i, nullptr, 0});
    if (j.has_per) { out.push_back({kTagPerCfg, -1, &per, sizeof per}); out.push_back({kTagPerLeaves, 14, nullptr, 0}); }
  }
  if (!j.user.empty()) out.push_back({kTagUser, -1, j.user.data(), j.user.size()});
  std::vector<StreamEntry> entries;
  for (const Out& o : out) {
    if (o.dev_ix >= 0) entries.push_back({o.tag, dev[o.dev_ix].crc, dev[o.dev_ix].bytes});
    else entries.push_back({o.tag, crc32_of(o.host, o.bytes), o.bytes});
  }
  dqnhip_state_info_t info = j.info;
  info.memory_size = j.with_mem ? size : 0;
  info.actor_iter = rec.actor_iter; info.critic_iter = rec.critic_iter; info.update_counter = rec.update_counter;
  StreamWriter w;
  if (w.open(j.filename.c_str(), info, entries, err)) return 1;
  for (const Out& o : out) {
    if (o.dev_ix >= 0) { if (stream_dev(a, a->stage + dev[o.dev_ix].off, (size_t)dev[o.dev_ix].bytes, &w, err)) return 1; }
    else if (w.append(o.host, o.bytes, err)) return 1;
  }
  return w.finish(err);
}

// The writer thread's share of one asynchronous snapshot, under the same rule: the snapshot's staging buffer, its job and its
// launch's CrcArgs are all it reads.  Order and names are dqnhip_snapshot's; every file appears under a name only when it is complete.
int snap_write_job(StateAsync* a, std::string* err) {
  SnapAsync* sn = a->snap;
  const SnapJob& j = sn->job;
  WCHK(hipSetDevice(j.device));
  StateRec rec{};
  if (fetch_dev(a, sn->stage + sn->off_rec, sizeof rec, &rec, err)) return 1;
  const int head = rec.ring_head, size = rec.ring_size;
  if (j.with_mem) {
    if (head < 0 || head >= j.cap || size < 0 || size > j.cap) {
      *err = "the ring's (head, size) = (" + std::to_string(head) + ", " + std::to_string(size) + ") is outside its capacity " + std::to_string(j.cap);
      return 1;
    }
    uint32_t guard[dqnhip_snap::kGuardWords];
    if (fetch_dev(a, sn->stage + sn->off_guard, sizeof guard, guard, err)) return 1;
    for (int i = 0; i < dqnhip_snap::kGuardWords; ++i)
      if (guard[i] != dqnhip_snap::kGuardWord) { *err = "guard word " + std::to_string(i) + " behind the replay-memory stream was overwritten; no file was written"; return 1; }
  }
  // ---- the four protobuf files, from the staged dense arrays ----
  std::vector<float> par[kSnapPar];
  for (int i = 0; i < kSnapPar; ++i) {
    par[i].resize(sn->par_bytes[i] / sizeof(float));
    if (fetch_dev(a, sn->stage + sn->off_par[i], sn->par_bytes[i], par[i].data(), err)) return 1;
  }
  const int iters[2] = {rec.actor_iter, rec.critic_iter};
  static const char* const kNet[2] = {"_actor", "_critic"};
  std::string to[2];
  for (int net = 0; net < 2; ++net) {
    const std::string from = j.save_path + kNet[net] + "_iter_" + std::to_string(iters[net]);      // Solver::SnapshotFilename
    to[net] = j.prefix + kNet[net] + "_iter_" + std::to_string(iters[net]);
    if (dqnhip_snap::publish_file(from + ".caffemodel", dqnhip_snap::caffemodel_bytes(j.cfg, net, par[net].data()), err)) return 1;
    const float* h2 = j.two ? par[3 + 2 * net].data() : nullptr;
    if (dqnhip_snap::publish_file(from + ".solverstate", dqnhip_snap::solverstate_bytes(j.cfg, net, iters[net], from + ".caffemodel", par[2 + 2 * net].data(), h2), err)) return 1;
  }
  for (int net = 0; net < 2; ++net) {
    const std::string from = j.save_path + kNet[net] + "_iter_" + std::to_string(iters[net]);
    if (dqnhip_snap::move_file(from + ".caffemodel", to[net] + ".caffemodel", err) || dqnhip_snap::move_file(from + ".solverstate", to[net] + ".solverstate", err)) return 1;
  }
  // ---- the replay memory: one gzip member, the trailer's CRC from the device ----
  if (j.with_mem) {
    const uint64_t rec_bytes = (uint64_t)size * dqnhip_snap::record_bytes(j.S);
    std::vector<uint32_t> raws((size_t)((rec_bytes + kCrcChunk - 1) / kCrcChunk));
    if (fetch_dev(a, sn->stage + sn->off_crc, raws.size() * sizeof(uint32_t), raws.data(), err)) return 1;
    // k_state_crc checksums the records; the count in front is four bytes the host knows: crc(A || B) = Z_|B|(crc(A)) ^ crc(B),
    // zlib's crc32_combine
    const int32_t count = size;
    const uint32_t crc = (uint32_t)crc32_combine(crc32_of(&count, sizeof count), crc_fold_chunks(raws.data(), rec_bytes, a->chunk_tab), (z_off_t)rec_bytes);
    const std::string mem = j.prefix + "_iter_" + std::to_string(std::max(iters[0], iters[1])) + ".replaymemory";
    GzipParallelWriter w;
    if (w.open(mem.c_str(), j.workers, GzipParallelWriter::kDefaultChunk, err)) return 1;
    if (stream_dev(a, sn->stage + sn->off_stream, (size_t)(4 + rec_bytes), &w, err)) return 1;
    if (w.finish(crc, err)) return 1;
  }
  if (j.remove_old) dqnhip_snap::remove_old_snapshots(j.prefix, iters[0], iters[1]);      // only now: all of this job's files are in place
  sn->actor_iter = iters[0]; sn->critic_iter = iters[1];
  return 0;
}

void writer_main(StateAsync* a) {
  // the learner captures its graphs in thread-local mode; this thread's copies and waits are checked against its own captures (none)
  hipStreamCaptureMode mode = hipStreamCaptureModeThreadLocal;
  (void)hipThreadExchangeStreamCaptureMode(&mode);
  std::unique_lock<std::mutex> lk(a->mu);
  for (;;) {
    a->cv.wait(lk, [a] { return !a->queue.empty() || a->quit; });
    if (a->queue.empty()) return;        // quit, and nothing left to write
    const int kind = a->queue.front();
    a->queue.pop_front();
    lk.unlock();
    std::string err;
    const int rc = kind == kJobState ? write_job(a, &err) : snap_write_job(a, &err);
    lk.lock();
    a->failed[kind] = rc != 0; a->err[kind] = err;
    a->busy[kind] = false;
    a->cv.notify_all();
  }
}

// one parameter arena -> the pieces of its dense image at dst
int arena_segs(const NetLayout& l, const float* base, float* dst, std::vector<PackSeg>* segs) {
  size_t d = 0;
  auto piece = [&](size_t src_off, int rows, int width, int pitch) {
    const float* s = base + src_off; float* t = dst + d;
    const bool vec = width % 4 == 0 && pitch % 4 == 0 && (uintptr_t)s % 16 == 0 && (uintptr_t)t % 16 == 0;
    segs->push_back(PackSeg{s, t, rows, width, pitch, vec ? 1 : 0});
    d += (size_t)rows * width;
  };
  for (int i = 0; i < l.L; ++i) {
    piece(l.w_off[i], l.dims[i + 1], l.dims[i], l.kp[i]);          // the pad columns of a row stay behind
    piece(l.b_off[i], 1, l.dims[i + 1], l.dims[i + 1]);
  }
  const int Hh = l.dims[l.L];
  if (l.NH == kNO) {                     // action_layer.W[4,H] .b[4] actionpara_layer.W[6,H] .b[6] (arena_to_dense)
    piece(l.hw_off, 1, kNA * Hh, kNA * Hh); piece(l.hb_off, 1, kNA, kNA);
    piece(l.hw_off + (size_t)kNA * Hh, 1, kNP * Hh, kNP * Hh); piece(l.hb_off + kNA, 1, kNP, kNP);
  } else {
    piece(l.hw_off, 1, Hh, Hh); piece(l.hb_off, 1, 1, 1);
  }
  return d == l.dense ? 0 : fail("dqnhip_save_state_async: the dense image of a net has %zu floats, expected %zu", d, l.dense);
}

// first use of either kind of job: what they share — the pinned ring, the copy stream, the combine table, the writer thread
int writer_init(H* h) {
  if (h->sasync) return 0;
  std::unique_ptr<StateAsync> up(new StateAsync);
  StateAsync* a = up.get();
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipHostMalloc((void**)&a->pinned, 2 * kPinnedChunk, hipHostMallocDefault));
  const hipError_t e = hipStreamCreateWithFlags(&a->copy_stream, hipStreamNonBlocking);
  if (e != hipSuccess) { hipHostFree(a->pinned); return fail("hipStreamCreateWithFlags failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__); }
  uint32_t op[32];
  crc_zeros_op(op, kCrcChunk);
  crc_op_table(a->chunk_tab, op);
  a->th = std::thread(writer_main, a);
  h->sasync = up.release();
  return 0;
}

// first asynchronous save: the staging buffer's map, the buffer, its event, the segment table
int state_async_init(H* h) {
  RC(writer_init(h));
  StateAsync* a = h->sasync;
  if (a->stage) return 0;
  const size_t cap = (size_t)h->ring.cap;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off = round_up_z(off + bytes, 16); return at; };
  a->off_rec = take(sizeof(StateRec));
  for (int net = 0; net < 4; ++net) a->par_bytes[net] = layout_of(h, net).dense * sizeof(float);
  for (int net = 0; net < 2; ++net) a->par_bytes[4 + 2 * net] = a->par_bytes[5 + 2 * net] = layout_of(h, net).dense * sizeof(float);
  const uint32_t row_bytes[kRingArrays] = {(uint32_t)h->S * 4u, (uint32_t)h->S * 4u, (uint32_t)kNO * 4u, 4u, 4u, 1u, 4u};
  uint64_t chunks = 0;
  for (int i = 0; i < 8; ++i) chunks += (a->par_bytes[i] + kCrcChunk - 1) / kCrcChunk;
  for (int i = 0; i < kRingArrays; ++i) { a->ring_row_bytes[i] = row_bytes[i]; chunks += (cap * row_bytes[i] + kCrcChunk - 1) / kCrcChunk; }
  if (chunks > 0x7fffffffull) return fail("dqnhip_save_state_async: this learner's file is too large for the chunk table");
  const int max_segs = 8 * (2 * kMaxL + 4);
  a->off_segs = take((size_t)max_segs * sizeof(PackSeg));
  a->off_crc = take((size_t)chunks * sizeof(uint32_t));
  for (int i = 0; i < 8; ++i) a->off_par[i] = take(a->par_bytes[i]);
  for (int i = 0; i < kRingArrays; ++i) a->off_ring[i] = take(cap * row_bytes[i]);
  a->stage_bytes = off;
  HIPCHK(hipSetDevice(h->cfg.device));
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, a->stage_bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail("dqnhip_save_state_async: cannot allocate the device staging buffer of %zu bytes (%s); the learner is untouched and "
                "dqnhip_save_state, which needs none, still works", a->stage_bytes, hipGetErrorString(e));
  }
  uint8_t* stage = (uint8_t*)p;
  hipEvent_t ev = nullptr;
  auto bail = [&](int rc) {
    if (ev) hipEventDestroy(ev);
    hipFree(stage);
    a->segs.clear();
    return rc;
  };
#define ICHK(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return bail(fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__)); } while (0)
  ICHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  // the segment table: W of the four nets, then (m, v) of the two online nets — the order of the parameter sections
  const float* arenas[8] = {h->w[0], h->w[1], h->w[2], h->w[3], h->m[0], h->v[0], h->m[1], h->v[1]};
  for (int i = 0; i < 8; ++i) {
    const int net = i < 4 ? i : (i - 4) / 2;
    if (arena_segs(layout_of(h, net), arenas[i], (float*)(stage + a->off_par[i]), &a->segs)) return bail(1);
  }
  a->n_seg = (int)a->segs.size();
  if (a->n_seg > max_segs) return bail(fail("dqnhip_save_state_async: %d parameter pieces, room for %d", a->n_seg, max_segs));
  ICHK(hipMemcpyAsync(stage + a->off_segs, a->segs.data(), a->segs.size() * sizeof(PackSeg), hipMemcpyHostToDevice, h->stream));
  ICHK(hipStreamSynchronize(h->stream));
#undef ICHK
  a->stage = stage; a->ev = ev;
  return 0;
}

// first asynchronous snapshot: the same for the snapshot's own staging buffer — the two kinds of job can be in flight together
int snap_async_init(H* h) {
  RC(writer_init(h));
  StateAsync* a = h->sasync;
  if (a->snap) return 0;
  std::unique_ptr<SnapAsync> up(new SnapAsync);
  SnapAsync* sn = up.get();
  const bool two = h->cfg.solver_type == DQNHIP_SOLVER_ADAM || h->cfg.solver_type == DQNHIP_SOLVER_ADADELTA;
  const uint64_t cap = (uint64_t)h->ring.cap, R = dqnhip_snap::record_bytes(h->S);
  const uint64_t chunks = (cap * R + kCrcChunk - 1) / kCrcChunk;
  if (chunks > 0x7fffffffull) return fail("dqnhip_snapshot_async: this learner's replay memory is too large for the chunk table");
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off = round_up_z(off + bytes, 16); return at; };
  sn->off_rec = take(sizeof(StateRec));
  // W of actor and critic, then (history 1, history 2) of each; a single-history solver has no second set
  for (int i = 0; i < kSnapPar; ++i) {
    const int net = i < 2 ? i : (i - 2) / 2;
    const bool second = i >= 2 && (i - 2) % 2 == 1;
    sn->par_bytes[i] = second && !two ? 0 : layout_of(h, net).dense * sizeof(float);
    // the builders of snapshot.cpp index these arrays by their own blob table: the two must describe the same dense array
    if (dqnhip_snap::dense_count(h->cfg, net) != (size_t)layout_of(h, net).dense)
      return fail("dqnhip_snapshot_async: the snapshot codec counts %zu dense parameters in net %d, the learner %zu", dqnhip_snap::dense_count(h->cfg, net), net,
                  (size_t)layout_of(h, net).dense);
  }
  const int max_segs = kSnapPar * (2 * kMaxL + 4);
  sn->off_segs = take((size_t)max_segs * sizeof(PackSeg));
  sn->off_crc = take((size_t)chunks * sizeof(uint32_t));
  for (int i = 0; i < kSnapPar; ++i) sn->off_par[i] = take(sn->par_bytes[i]);
  const size_t max_dwords = (size_t)dqnhip_snap::stream_dwords(h->S, cap);
  sn->off_stream = take(16) + 12;                  // the count's four bytes end on a 16-byte boundary: k_snap_pack_replay stores whole 16-byte pieces of records, their CRC reads whole lines
  off = sn->off_stream + 4 * max_dwords;
  sn->off_guard = off;
  off += dqnhip_snap::kGuardWords * sizeof(uint32_t);
  sn->stage_bytes = round_up_z(off, 16);
  HIPCHK(hipSetDevice(h->cfg.device));
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, sn->stage_bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail("dqnhip_snapshot_async: the asynchronous snapshot cannot allocate its device staging buffer of %zu bytes (%s); the learner is "
                "untouched and dqnhip_snapshot, which needs none, still works", sn->stage_bytes, hipGetErrorString(e));
  }
  sn->stage = (uint8_t*)p;
  auto bail = [&](int rc) {
    if (sn->ev) hipEventDestroy(sn->ev);
    hipFree(sn->stage);
    return rc;
  };
#define ICHK(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return bail(fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__)); } while (0)
  ICHK(hipEventCreateWithFlags(&sn->ev, hipEventDisableTiming));
  const float* arenas[kSnapPar] = {h->w[0], h->w[1], h->m[0], h->v[0], h->m[1], h->v[1]};
  for (int i = 0; i < kSnapPar; ++i) {
    if (!sn->par_bytes[i]) continue;
    const int net = i < 2 ? i : (i - 2) / 2;
    if (arena_segs(layout_of(h, net), arenas[i], (float*)(sn->stage + sn->off_par[i]), &sn->segs)) return bail(1);
  }
  sn->n_seg = (int)sn->segs.size();
  if (sn->n_seg > max_segs) return bail(fail("dqnhip_snapshot_async: %d parameter pieces, room for %d", sn->n_seg, max_segs));
  ICHK(hipMemcpyAsync(sn->stage + sn->off_segs, sn->segs.data(), sn->segs.size() * sizeof(PackSeg), hipMemcpyHostToDevice, h->stream));
  ICHK(hipStreamSynchronize(h->stream));
#undef ICHK
  a->snap = up.release();
  return 0;
}

// waits for the job of `kind` in flight; its failure, once, as `what`'s
int job_join(H* h, int kind, const char* what) {
  StateAsync* a = h->sasync;
  if (!a) return 0;
  std::unique_lock<std::mutex> lk(a->mu);
  a->cv.wait(lk, [a, kind] { return !a->busy[kind]; });
  if (!a->failed[kind]) return 0;
  a->failed[kind] = false;
  if (kind == kJobState) return fail("%s: the asynchronous save of %s failed: %s", what, a->job.filename.c_str(), a->err[kind].c_str());
  return fail("%s: the asynchronous snapshot to %s failed: %s", what, a->snap->job.prefix.c_str(), a->err[kind].c_str());
}

}  // namespace

namespace dqnhip_host {

int state_async_join(H* h, const char* what) { return job_join(h, kJobState, what); }
int snapshot_async_join(H* h, const char* what) { return job_join(h, kJobSnapshot, what); }

void state_async_free(H* h) {
  StateAsync* a = h->sasync;
  if (!a) return;
  {
    std::unique_lock<std::mutex> lk(a->mu);
    a->cv.wait(lk, [a] { return !a->busy[kJobState] && !a->busy[kJobSnapshot]; });
    a->quit = true;
    a->cv.notify_all();
  }
  a->th.join();
  if (a->snap) { hipEventDestroy(a->snap->ev); hipFree(a->snap->stage); delete a->snap; }
  if (a->stage) { hipEventDestroy(a->ev); hipFree(a->stage); }
  hipStreamDestroy(a->copy_stream); hipHostFree(a->pinned);
  delete a;
  h->sasync = nullptr;
}

}  // namespace dqnhip_host

// what snapshot.cpp (a client of the C-ABI, without the learner's definition) needs of the above
extern "C" int dqnhip_internal_snapshot_join(dqnhip_handle h, const char* what) { return h ? snapshot_async_join(h, what) : 0; }

extern "C" {

int dqnhip_save_state_async(dqnhip_handle h, const char* filename, int32_t flags, const void* user, size_t user_bytes) {
  if (!h || !filename) return fail("dqnhip_save_state_async: null argument");
  if (flags & ~DQNHIP_STATE_NO_MEMORY) return fail("dqnhip_save_state_async: unknown flags %d", flags);
  if (!user && user_bytes) return fail("dqnhip_save_state_async: user is null but user_bytes is %zu", user_bytes);
  RC(state_refuse(h, "dqnhip_save_state_async"));
  RC(state_async_join(h, "dqnhip_save_state_async"));      // one save in flight per learner
  const bool with_mem = !(flags & DQNHIP_STATE_NO_MEMORY);
  HIPCHK(hipSetDevice(h->cfg.device));
  RC(per_sync_if_needed(h));
  RC(state_async_init(h));
  StateAsync* a = h->sasync;
  // ---- the learner's stream: pack, checksum, event ----
  RC(state_pack_params_launch(h, (const PackSeg*)(a->stage + a->off_segs), a->n_seg, (StateRec*)(a->stage + a->off_rec)));
  const bool has_per = with_mem && h->per;
  const int n_arr = !with_mem ? 0 : has_per ? 7 : 6;
  if (with_mem) {
    const Ring& g = h->ring;
    RingPackArgs r{};
    r.st = h->st; r.cap = g.cap; r.n_arr = n_arr;
    const bool vecS = h->S % 4 == 0 && g.SP % 4 == 0;
    r.arr[0] = RingArr{g.state, a->stage + a->off_ring[0], h->S, g.SP, 4, vecS};
    r.arr[1] = RingArr{g.next, a->stage + a->off_ring[1], h->S, g.SP, 4, vecS};
    r.arr[2] = RingArr{g.act, a->stage + a->off_ring[2], kNO, kAP, 4, 0};
    r.arr[3] = RingArr{g.reward, a->stage + a->off_ring[3], 1, 1, 4, 0};
    r.arr[4] = RingArr{g.mc, a->stage + a->off_ring[4], 1, 1, 4, 0};
    r.arr[5] = RingArr{g.term, a->stage + a->off_ring[5], 1, 1, 1, 0};
    if (has_per) r.arr[6] = RingArr{h->per->tree.lvl[0], a->stage + a->off_ring[6], 1, 1, 4, 0};
    RC(state_pack_ring_launch(h, r));
  }
  CrcArgs c{};
  c.base = a->stage; c.rec = (const StateRec*)(a->stage + a->off_rec); c.out = (uint32_t*)(a->stage + a->off_crc);
  c.max_rows = h->ring.cap;
  uint32_t chunk0 = 0;
  for (int i = 0; i < 8; ++i) {
    c.sec[c.n++] = CrcSection{a->off_par[i], a->par_bytes[i], 0u, chunk0};
    chunk0 += (uint32_t)((a->par_bytes[i] + kCrcChunk - 1) / kCrcChunk);
  }
  for (int i = 0; i < n_arr; ++i) {
    c.sec[c.n++] = CrcSection{a->off_ring[i], 0, a->ring_row_bytes[i], chunk0};
    chunk0 += (uint32_t)(((uint64_t)h->ring.cap * a->ring_row_bytes[i] + kCrcChunk - 1) / kCrcChunk);
  }
  c.total_chunks = chunk0;
  RC(state_crc_launch(h, c));
  HIPCHK(hipEventRecord(a->ev, h->stream));
  HIPCHK(hipStreamWaitEvent(a->copy_stream, a->ev, 0));    // the writer's copies are ordered behind the image by its own stream
  // ---- the job: everything the writer needs of the host, as it is now ----
  std::unique_lock<std::mutex> lk(a->mu);
  a->crc = c;
  StateJob& j = a->job;
  j = StateJob{};
  j.filename = filename; j.flags = flags; j.with_mem = with_mem; j.has_per = has_per; j.has_ls = h->ls_dynamic;
  if (user_bytes) j.user.assign((const uint8_t*)user, (const uint8_t*)user + user_bytes);
  j.host = HostSection{h->sample_states_calls, h->cfg.seed};
  j.has_solver = h->cfg.solver_type != DQNHIP_SOLVER_ADAM;
  j.solver = SolverSection{h->cfg.solver_type, h->cfg.rms_decay, {0, 0}};
  j.has_lr = has_policy(h) || has_decay(h);
  j.lr = lr_section_of(h->cfg);
  if (has_per) {
    const dqnhip_per_config& pc = h->per->cfg;
    j.per = PerSection{pc.alpha, pc.beta0, pc.beta_anneal_iters, pc.eps, pc.seed, 0.0f, 0, (int64_t)h->per->syncs};
  }
  dqnhip_state_info_t& info = j.info;
  info.struct_size = (int32_t)sizeof info; info.version = (int32_t)kVersion; info.flags = flags;
  info.precision = h->cfg.precision; info.minibatch = h->cfg.minibatch; info.state_size = h->cfg.state_size; info.num_hidden = h->cfg.num_hidden;
  for (int i = 0; i < h->cfg.num_hidden; ++i) info.hidden[i] = h->cfg.hidden[i];
  info.replay_capacity = h->cfg.replay_capacity;
  info.has_memory = with_mem; info.has_per = has_per; info.has_loss_scale = h->ls_dynamic;
  info.seed = h->cfg.seed;
  j.device = h->cfg.device; j.cap = h->ring.cap;
  a->failed[kJobState] = false; a->err[kJobState].clear();
  a->queue.push_back(kJobState); a->busy[kJobState] = true;
  a->cv.notify_all();
  return 0;
}

int dqnhip_save_state_wait(dqnhip_handle h) {
  if (!h) return fail("dqnhip_save_state_wait: null argument");
  return state_async_join(h, "dqnhip_save_state_wait");
}

int dqnhip_save_state_poll(dqnhip_handle h, int32_t* done) {
  if (!h || !done) return fail("dqnhip_save_state_poll: null argument");
  StateAsync* a = h->sasync;
  if (!a) { *done = 1; return 0; }
  std::lock_guard<std::mutex> lk(a->mu);
  *done = a->busy[kJobState] ? 0 : 1;
  return 0;
}

int dqnhip_snapshot_async(dqnhip_handle h, const char* save_path, const char* snapshot_prefix, int32_t remove_old, int32_t snapshot_memory,
                          int32_t compress_threads) {
  if (!h || !save_path || !snapshot_prefix) return fail("dqnhip_snapshot_async: null argument");
  if (compress_threads < 0 || compress_threads > 64) return fail("dqnhip_snapshot_async: compress_threads %d is outside 0 ... 64 (0: the default, 8)", compress_threads);
  RC(state_refuse(h, "dqnhip_snapshot_async: the asynchronous snapshot"));
  RC(snapshot_async_join(h, "dqnhip_snapshot_async"));      // one snapshot in flight per learner
  HIPCHK(hipSetDevice(h->cfg.device));
  RC(snap_async_init(h));
  StateAsync* a = h->sasync;
  SnapAsync* sn = a->snap;
  // ---- the learner's stream: parameters and record, the stream, its checksum, event ----
  RC(state_pack_params_launch(h, (const PackSeg*)(sn->stage + sn->off_segs), sn->n_seg, (StateRec*)(sn->stage + sn->off_rec)));
  CrcArgs c{};
  if (snapshot_memory) {
    RC(snap_pack_replay_launch(h, sn->stage + sn->off_stream));
    c.base = sn->stage; c.rec = (const StateRec*)(sn->stage + sn->off_rec); c.out = (uint32_t*)(sn->stage + sn->off_crc);
    c.max_rows = h->ring.cap; c.n = 1;
    const uint32_t R = (uint32_t)dqnhip_snap::record_bytes(h->S);
    c.sec[0] = CrcSection{sn->off_stream + 4, 0, R, 0u};       // the records; the count in front of them is the host's to add
    c.total_chunks = (uint32_t)(((uint64_t)h->ring.cap * R + kCrcChunk - 1) / kCrcChunk);
    RC(state_crc_launch(h, c));
  }
  HIPCHK(hipEventRecord(sn->ev, h->stream));
  HIPCHK(hipStreamWaitEvent(a->copy_stream, sn->ev, 0));   // the writer's copies are ordered behind the image by its own stream
  // ---- the job ----
  std::unique_lock<std::mutex> lk(a->mu);
  SnapJob& j = sn->job;
  j = SnapJob{};
  j.save_path = save_path; j.prefix = snapshot_prefix; j.remove_old = remove_old != 0; j.with_mem = snapshot_memory != 0;
  j.two = h->cfg.solver_type == DQNHIP_SOLVER_ADAM || h->cfg.solver_type == DQNHIP_SOLVER_ADADELTA;
  j.workers = compress_threads ? compress_threads : 8;       // (never derived from the machine's CPU count: a container may grant fewer)
  j.cfg = h->cfg; j.device = h->cfg.device; j.cap = h->ring.cap; j.S = h->S;
  a->failed[kJobSnapshot] = false; a->err[kJobSnapshot].clear();
  a->queue.push_back(kJobSnapshot); a->busy[kJobSnapshot] = true;
  a->cv.notify_all();
  return 0;
}

int dqnhip_snapshot_wait(dqnhip_handle h, int32_t* actor_iter, int32_t* critic_iter) {
  if (!h) return fail("dqnhip_snapshot_wait: null argument");
  RC(snapshot_async_join(h, "dqnhip_snapshot_wait"));
  const SnapAsync* sn = h->sasync ? h->sasync->snap : nullptr;
  if (actor_iter) *actor_iter = sn ? sn->actor_iter : 0;
  if (critic_iter) *critic_iter = sn ? sn->critic_iter : 0;
  return 0;
}

int dqnhip_snapshot_poll(dqnhip_handle h, int32_t* done) {
  if (!h || !done) return fail("dqnhip_snapshot_poll: null argument");
  StateAsync* a = h->sasync;
  if (!a) { *done = 1; return 0; }
  std::lock_guard<std::mutex> lk(a->mu);
  *done = a->busy[kJobSnapshot] ? 0 : 1;
  return 0;
}

int dqnhip_save_state(dqnhip_handle h, const char* filename, int32_t flags, const void* user, size_t user_bytes) {
  if (!h || !filename) return fail("dqnhip_save_state: null argument");
  if (flags & ~DQNHIP_STATE_NO_MEMORY) return fail("dqnhip_save_state: unknown flags %d", flags);
  if (!user && user_bytes) return fail("dqnhip_save_state: user is null but user_bytes is %zu", user_bytes);
  RC(state_refuse(h, "dqnhip_save_state"));
  RC(state_async_join(h, "dqnhip_save_state"));    // (an asynchronous save in flight finishes first)
  const bool with_mem = !(flags & DQNHIP_STATE_NO_MEMORY);
  HIPCHK(hipSetDevice(h->cfg.device));
  RC(per_sync_if_needed(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  RC(ix_harvest_all(h));                           // (indexed updates: their scalars stay collectable, they are not part of the file)
  DevState st{};
  HIPCHK(hipMemcpy(&st, h->st, sizeof st, hipMemcpyDeviceToHost));
  h->h_head = st.ring_head; h->h_size = st.ring_size; h->ring_stale = false;     // (refresh_ring, from the copy at hand)

  std::vector<float> par[8];
  std::vector<Section> sec;
  for (int net = 0; net < 4; ++net) {
    par[net].resize(layout_of(h, net).dense);
    RC(dqnhip_get_params(h, net, DQNHIP_KIND_W, par[net].data(), par[net].size()));
    sec.push_back({kTagW[net], par[net].data(), par[net].size() * sizeof(float)});
  }
  for (int net = 0; net < 2; ++net) {
    std::vector<float>&m = par[4 + net], &v = par[6 + net];
    m.resize(layout_of(h, net).dense); v.resize(m.size());
    RC(dqnhip_get_params(h, net, DQNHIP_KIND_M, m.data(), m.size()));
    RC(dqnhip_get_params(h, net, DQNHIP_KIND_V, v.data(), v.size()));
    sec.push_back({kTagM[net], m.data(), m.size() * sizeof(float)});
    sec.push_back({kTagV[net], v.data(), v.size() * sizeof(float)});
  }
  // a learner whose solver is not Adam says so; an Adam learner's file is what it was before the other solvers existed
  const SolverSection solver{h->cfg.solver_type, h->cfg.rms_decay, {0, 0}};
  if (h->cfg.solver_type != DQNHIP_SOLVER_ADAM) sec.push_back({kTagSolver, &solver, sizeof solver});
  // ... and so does a learner with an lr policy or a weight decay (SOLV's rules: without either, the file is byte for byte what it was)
  const LrSection lrs = lr_section_of(h->cfg);
  if (has_policy(h) || has_decay(h)) sec.push_back({kTagLrSched, &lrs, sizeof lrs});
  const DevSection dev{st.actor_iter, st.critic_iter, st.update_counter, st.critic_loss, st.avg_q, st.flags, st.skipped_steps};
  sec.push_back({kTagDev, &dev, sizeof dev});
  const LossScaleSection ls{{st.ls_mult[0][0], st.ls_mult[1][0]}, {st.ls_good[0], st.ls_good[1]}, {st.ls_backoffs[0], st.ls_backoffs[1]},
                            {st.ls_growths[0], st.ls_growths[1]}};
  if (h->ls_dynamic) sec.push_back({kTagLossScale, &ls, sizeof ls});
  const HostSection host{h->sample_states_calls, h->cfg.seed};
  sec.push_back({kTagHost, &host, sizeof host});

  const int head = st.ring_head, size = st.ring_size, S = h->S;
  const RingSection ring{head, size};
  std::vector<float> s, nx, a, r, mc, leaves;
  std::vector<uint8_t> term;
  PerSection per{};
  if (with_mem) {
    if (head < 0 || head >= h->ring.cap || size < 0 || size > h->ring.cap) return fail("dqnhip_save_state: the ring's (head, size) = (%d, %d) is outside its capacity %d", head, size, h->ring.cap);
    s.resize((size_t)size * S); nx.resize((size_t)size * S); a.resize((size_t)size * kNO); r.resize(size); mc.resize(size); term.resize(size);
    const Ring& g = h->ring;
    RC(window_copy(h, g.state, (size_t)g.SP * 4, s.data(), (size_t)S * 4, head, size, true));
    RC(window_copy(h, g.next, (size_t)g.SP * 4, nx.data(), (size_t)S * 4, head, size, true));
    RC(window_copy(h, g.act, (size_t)kAP * 4, a.data(), (size_t)kNO * 4, head, size, true));
    RC(window_copy(h, g.reward, 4, r.data(), 4, head, size, true));
    RC(window_copy(h, g.mc, 4, mc.data(), 4, head, size, true));
    RC(window_copy(h, g.term, 1, term.data(), 1, head, size, true));
    sec.push_back({kTagRing, &ring, sizeof ring});
    sec.push_back({kTagStates, s.data(), s.size() * 4}); sec.push_back({kTagNext, nx.data(), nx.size() * 4});
    sec.push_back({kTagAct, a.data(), a.size() * 4}); sec.push_back({kTagReward, r.data(), r.size() * 4});
    sec.push_back({kTagMc, mc.data(), mc.size() * 4}); sec.push_back({kTagTerm, term.data(), term.size()});
    if (h->per) {
      const dqnhip_per_config& c = h->per->cfg;
      float p_max = 0.0f;
      RC(per_read_p_max(h, &p_max));
      per = PerSection{c.alpha, c.beta0, c.beta_anneal_iters, c.eps, c.seed, p_max, 0, (int64_t)h->per->syncs};
      leaves.resize(size);
      RC(window_copy(h, h->per->tree.lvl[0], 4, leaves.data(), 4, head, size, true));
      sec.push_back({kTagPerCfg, &per, sizeof per});
      sec.push_back({kTagPerLeaves, leaves.data(), leaves.size() * 4});
    }
  }
  if (user_bytes) sec.push_back({kTagUser, user, user_bytes});

  dqnhip_state_info_t info{};
  info.struct_size = (int32_t)sizeof info; info.version = (int32_t)kVersion; info.flags = flags;
  info.precision = h->cfg.precision; info.minibatch = h->cfg.minibatch; info.state_size = h->cfg.state_size; info.num_hidden = h->cfg.num_hidden;
  for (int i = 0; i < h->cfg.num_hidden; ++i) info.hidden[i] = h->cfg.hidden[i];
  info.replay_capacity = h->cfg.replay_capacity; info.memory_size = with_mem ? size : 0;
  info.actor_iter = st.actor_iter; info.critic_iter = st.critic_iter;
  info.has_memory = with_mem; info.has_per = with_mem && h->per; info.has_loss_scale = h->ls_dynamic;
  info.seed = h->cfg.seed; info.update_counter = st.update_counter;
  std::string err;
  if (write_file(filename, info, sec, &err)) return fail("dqnhip_save_state: %s", err.c_str());
  return 0;
}

int dqnhip_load_state(dqnhip_handle h, const char* filename) {
  if (!h || !filename) return fail("dqnhip_load_state: null argument");
  RC(state_refuse(h, (std::string("dqnhip_load_state: ") + filename).c_str()));
  RC(state_async_join(h, "dqnhip_load_state"));
  RC(snapshot_async_join(h, "dqnhip_load_state"));
  // ---- everything that can fail for the file's sake, before the learner is touched ----
  Parsed p; std::string err;
  if (read_file(filename, &p, true, &err)) return fail("dqnhip_load_state: %s", err.c_str());
  const dqnhip_state_info_t& in = p.info;
  const int S = h->S;
  bool same = in.state_size == h->cfg.state_size && in.num_hidden == h->cfg.num_hidden;
  for (int i = 0; same && i < h->cfg.num_hidden; ++i) same = in.hidden[i] == h->cfg.hidden[i];
  if (!same) {
    std::string a, b;
    for (int i = 0; i < std::min(std::max(in.num_hidden, 0), kMaxL); ++i) a += (i ? "," : "") + std::to_string(in.hidden[i]);
    for (int i = 0; i < h->cfg.num_hidden; ++i) b += (i ? "," : "") + std::to_string(h->cfg.hidden[i]);
    return fail("dqnhip_load_state: %s: the file's nets (state_size %d, hidden %s) are not this learner's (state_size %d, hidden %s)", filename,
                in.state_size, a.c_str(), h->cfg.state_size, b.c_str());
  }
  if (in.solver_type != h->cfg.solver_type)
    return fail("dqnhip_load_state: %s: the file was written by a learner with the %s solver, this learner's solver is %s (the histories mean something else)", filename,
                dqnhip_solver_name(in.solver_type), dqnhip_solver_name(h->cfg.solver_type));
  // the schedule and the decay: both sides must agree, in either direction (the rate of every later step depends on them)
  {
    const Entry* e = p.find(kTagLrSched);
    const bool mine = has_policy(h) || has_decay(h);
    if (e && e->bytes != sizeof(LrSection))
      return fail("dqnhip_load_state: %s: section LRSC holds %llu bytes, expected %zu", filename, (unsigned long long)e->bytes, sizeof(LrSection));
    LrSection theirs{};
    if (e) memcpy(&theirs, p.at(e), sizeof theirs);
    const LrSection ours = lr_section_of(h->cfg);
    if ((e != nullptr) != mine || (e && memcmp(&theirs, &ours, sizeof ours) != 0)) {
      const char* tn = e ? dqnhip_lr_policy_name(theirs.policy) : "fixed";
      return fail("dqnhip_load_state: %s: the file was written by a learner with lr_policy %s / weight_decay %g, this learner has lr_policy %s / weight_decay %g "
                  "(or another parameter of the schedule, the base rates or the kind of decay differs)", filename, tn ? tn : "?", e ? (double)theirs.weight_decay : 0.0,
                  dqnhip_lr_policy_name(h->cfg.lr_policy), (double)h->cfg.weight_decay);
    }
  }
  const bool with_mem = in.has_memory != 0;
  // a section of exactly `bytes` bytes
  auto need = [&](uint32_t tag, uint64_t bytes, const uint8_t** out) -> int {
    const Entry* e = p.find(tag);
    if (!e) return fail("dqnhip_load_state: %s: section %s is missing", filename, tag_name(tag).c_str());
    if (e->bytes != bytes) return fail("dqnhip_load_state: %s: section %s holds %llu bytes, expected %llu", filename, tag_name(tag).c_str(),
                                       (unsigned long long)e->bytes, (unsigned long long)bytes);
    *out = p.at(e);
    return 0;
  };
  const uint8_t *q_ring = nullptr, *q_s = nullptr, *q_nx = nullptr, *q_a = nullptr, *q_r = nullptr, *q_mc = nullptr, *q_t = nullptr, *q_pc = nullptr, *q_pl = nullptr;
  RingSection ring{}; PerSection per{};
  if (with_mem) {
    if (in.replay_capacity != h->ring.cap) return fail("dqnhip_load_state: %s: the file's replay capacity %d is not this learner's %d", filename, in.replay_capacity, h->ring.cap);
    if ((in.has_per != 0) != (h->per != nullptr))
      return fail(in.has_per ? "dqnhip_load_state: %s: the file holds priorities, this learner samples uniformly (dqnhip_per_enable first, or save with DQNHIP_STATE_NO_MEMORY)"
                             : "dqnhip_load_state: %s: the file holds no priorities, this learner has prioritized replay enabled", filename);
    if (in.has_per) {
      RC(need(kTagPerCfg, sizeof per, &q_pc));
      memcpy(&per, q_pc, sizeof per);
      if (__builtin_bit_cast(uint32_t, per.alpha) != __builtin_bit_cast(uint32_t, h->per->cfg.alpha))
        return fail("dqnhip_load_state: %s: the file's priorities were stored with alpha %g, this learner's alpha is %g", filename, (double)per.alpha, (double)h->per->cfg.alpha);
    }
    RC(need(kTagRing, sizeof ring, &q_ring));
    memcpy(&ring, q_ring, sizeof ring);
    const int cap = h->ring.cap;
    if (ring.ring_size < 0 || ring.ring_size > cap || ring.ring_head < 0 || ring.ring_head >= cap || ring.ring_size != in.memory_size)
      return fail("dqnhip_load_state: %s: (ring_head, ring_size) = (%d, %d) does not fit the capacity %d / the header's memory_size %d", filename,
                  ring.ring_head, ring.ring_size, cap, in.memory_size);
    const uint64_t n = (uint64_t)ring.ring_size;
    RC(need(kTagStates, n * S * 4, &q_s)); RC(need(kTagNext, n * S * 4, &q_nx)); RC(need(kTagAct, n * kNO * 4, &q_a));
    RC(need(kTagReward, n * 4, &q_r)); RC(need(kTagMc, n * 4, &q_mc)); RC(need(kTagTerm, n, &q_t));
    if (in.has_per) {
      RC(need(kTagPerLeaves, n * 4, &q_pl));
      if (!(per.p_max >= 0.0f) || !std::isfinite(per.p_max) || !(per.beta0 >= 0.0f && per.beta0 <= 1.0f) || per.beta_anneal_iters < 0 || !(per.eps >= 0.0f) || !std::isfinite(per.eps))
        return fail("dqnhip_load_state: %s: section PERC holds values outside their ranges", filename);
      for (uint64_t i = 0; i < n; ++i) {
        float v; memcpy(&v, q_pl + 4 * i, 4);
        if (!std::isfinite(v) || v < 0.0f) return fail("dqnhip_load_state: %s: priority %llu = %g is not finite and >= 0", filename, (unsigned long long)i, (double)v);
      }
    }
  }
  const uint8_t* q_par[8] = {nullptr};
  for (int net = 0; net < 4; ++net) RC(need(kTagW[net], (uint64_t)layout_of(h, net).dense * 4, &q_par[net]));
  for (int net = 0; net < 2; ++net) {
    RC(need(kTagM[net], (uint64_t)layout_of(h, net).dense * 4, &q_par[4 + net]));
    RC(need(kTagV[net], (uint64_t)layout_of(h, net).dense * 4, &q_par[6 + net]));
  }
  const uint8_t *q_dev = nullptr, *q_host = nullptr, *q_ls = nullptr;
  DevSection dev{}; HostSection host{}; LossScaleSection ls{};
  RC(need(kTagDev, sizeof dev, &q_dev)); memcpy(&dev, q_dev, sizeof dev);
  RC(need(kTagHost, sizeof host, &q_host)); memcpy(&host, q_host, sizeof host);
  if (dev.actor_iter != in.actor_iter || dev.critic_iter != in.critic_iter || dev.update_counter != in.update_counter || host.seed != in.seed)
    return fail("dqnhip_load_state: %s: the header and the DEVS / HOST sections disagree", filename);
  const bool apply_ls = in.has_loss_scale && h->ls_dynamic;
  if (in.has_loss_scale) { RC(need(kTagLossScale, sizeof ls, &q_ls)); memcpy(&ls, q_ls, sizeof ls); }
  if (apply_ls)
    for (int i = 0; i < 2; ++i) {
      if (!is_pow2(ls.mult[i])) return fail("dqnhip_load_state: %s: loss-scale multiplier %g is not a power of two", filename, (double)ls.mult[i]);
      if (ls.mult[i] < h->cfg.loss_scale_min_mult || ls.mult[i] > h->cfg.loss_scale_max_mult)
        return fail("dqnhip_load_state: %s: loss-scale multiplier %g is outside this learner's [loss_scale_min_mult, loss_scale_max_mult] = [%g, %g]", filename,
                    (double)ls.mult[i], (double)h->cfg.loss_scale_min_mult, (double)h->cfg.loss_scale_max_mult);
    }

  // ---- the learner ----
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  RC(ix_harvest_all(h));
  h->epoch += 1;                                   // a chain ends here
  h->chain_valid = false;
  std::vector<float> tmp;
  auto put_params = [&](int net, int kind, const uint8_t* q) -> int {
    tmp.resize(layout_of(h, net).dense);
    memcpy(tmp.data(), q, tmp.size() * 4);         // (the sections are packed back to back: not aligned)
    return dqnhip_set_params(h, net, kind, tmp.data(), tmp.size());     // W: marks the net's fp16 mirror dirty
  };
  for (int net = 0; net < 4; ++net) RC(put_params(net, DQNHIP_KIND_W, q_par[net]));
  for (int net = 0; net < 2; ++net) { RC(put_params(net, DQNHIP_KIND_M, q_par[4 + net])); RC(put_params(net, DQNHIP_KIND_V, q_par[6 + net])); }
  DevState st{};
  HIPCHK(hipMemcpy(&st, h->st, sizeof st, hipMemcpyDeviceToHost));      // (adam_corr, soft_now, gbase_*: per-update scratch, left as they are)
  st.actor_iter = dev.actor_iter; st.critic_iter = dev.critic_iter; st.update_counter = dev.update_counter;
  st.critic_loss = dev.critic_loss; st.avg_q = dev.avg_q; st.flags = dev.flags; st.skipped_steps = dev.skipped_steps;
  if (apply_ls)
    for (int i = 0; i < 2; ++i) {
      st.ls_mult[i][0] = ls.mult[i]; st.ls_mult[i][1] = 1.0f / ls.mult[i];
      st.ls_good[i] = ls.good[i]; st.ls_backoffs[i] = ls.backoffs[i]; st.ls_growths[i] = ls.growths[i];
    }
  if (with_mem) { st.ring_head = ring.ring_head; st.ring_size = ring.ring_size; }
  HIPCHK(hipMemcpy(h->st, &st, sizeof st, hipMemcpyHostToDevice));
  h->h_actor_iter = dev.actor_iter; h->h_critic_iter = dev.critic_iter;
  h->h_head = st.ring_head; h->h_size = st.ring_size; h->ring_stale = false;
  h->sample_states_calls = host.sample_states_calls;
  h->cfg.seed = host.seed;
  // what dqnhip_read_stats reads: the last update's pair and the sticky flags, as the device now holds them
  h->pinned_stats[0] = dev.critic_loss; h->pinned_stats[1] = dev.avg_q; memcpy(&h->pinned_stats[2], &dev.flags, sizeof dev.flags);
  h->ix_prev_flags = dev.flags;
  if (with_mem) {
    const int head = ring.ring_head, size = ring.ring_size;
    const Ring& g = h->ring;
    // (pad columns of the ring's rows are zero from create on and no writer touches them: only the S / 10 real columns move)
    RC(window_copy(h, g.state, (size_t)g.SP * 4, (void*)q_s, (size_t)S * 4, head, size, false));
    RC(window_copy(h, g.next, (size_t)g.SP * 4, (void*)q_nx, (size_t)S * 4, head, size, false));
    RC(window_copy(h, g.act, (size_t)kAP * 4, (void*)q_a, (size_t)kNO * 4, head, size, false));
    RC(window_copy(h, g.reward, 4, (void*)q_r, 4, head, size, false));
    RC(window_copy(h, g.mc, 4, (void*)q_mc, 4, head, size, false));
    RC(window_copy(h, g.term, 1, (void*)q_t, 1, head, size, false));
    if (h->per) {
      dqnhip_per_config& c = h->per->cfg;
      c.beta0 = per.beta0; c.beta_anneal_iters = per.beta_anneal_iters; c.eps = per.eps; c.seed = per.seed;
      tmp.resize((size_t)size);
      if (size) memcpy(tmp.data(), q_pl, (size_t)size * 4);
      RC(per_restore(h, tmp.data(), head, size, per.p_max, (long long)per.syncs));
    }
  }
  drop_graphs(h);
  return 0;
}

}  // extern "C"
