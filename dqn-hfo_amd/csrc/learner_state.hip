// learner_state.hip — dqnhip_save_state / dqnhip_load_state: the native learner-state file (include/dqnhip.h; DESIGN.md 9 has the
// byte layout, state_codec.cpp the container).  Host only: copies between the learner's device state and the file's sections, no
// kernel of its own — the one launch a load may need, the priority tree's set pass, goes through per_restore (learner_io.hip).
// dqnhip_save_state_async: the same file behind training.  The caller's thread enqueues the pack and the chunk CRCs on the learner's
// stream (state_kernels.hip.h, launched from learner_io.hip) and hands a job to the learner's writer thread, which waits for the
// event, folds the CRCs, and streams the staging buffer to the file through two pinned chunks.
#include <condition_variable>
#include <memory>

#include "learner_internal.hip.h"
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
  PerSection per{};                      // p_max comes from the record
  dqnhip_state_info_t info{};            // the config's share; the record fills the rest
  int device = 0, cap = 0;
};

struct StateAsync {
  // device side, allocated by the first asynchronous save and kept until dqnhip_destroy
  uint8_t* stage = nullptr; size_t stage_bytes = 0;
  uint8_t* pinned = nullptr;
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev = nullptr;
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
  bool pending = false, busy = false, quit = false;   // pending: a job waits for the thread; busy: a save is in flight
  StateJob job;
  bool failed = false; std::string err;  // of the last finished save, until a join reports it
};

}  // namespace dqnhip_host

namespace {

std::string hip_msg(const char* what, hipError_t e) { return std::string(what) + " failed: " + hipGetErrorString(e); }
#define WCHK(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { *err = hip_msg(#expr, e__); return 1; } } while (0)

// bytes [off, off + bytes) of the staging buffer -> dst (host memory of any kind), through the pinned ring
int fetch_dev(StateAsync* a, size_t off, size_t bytes, void* dst, std::string* err) {
  for (size_t done = 0; done < bytes;) {
    const size_t k = std::min(bytes - done, kPinnedChunk);
    WCHK(hipMemcpyAsync(a->pinned, a->stage + off + done, k, hipMemcpyDeviceToHost, a->copy_stream));
    WCHK(hipStreamSynchronize(a->copy_stream));
    memcpy((char*)dst + done, a->pinned, k);
    done += k;
  }
  return 0;
}
// ... -> the file: the copy of chunk k + 1 runs while chunk k is written
int stream_dev(StateAsync* a, size_t off, size_t bytes, StreamWriter* w, std::string* err) {
  if (!bytes) return 0;
  int b = 0;
  size_t k = std::min(bytes, kPinnedChunk);
  WCHK(hipMemcpyAsync(a->pinned, a->stage + off, k, hipMemcpyDeviceToHost, a->copy_stream));
  for (size_t done = 0; done < bytes;) {
    WCHK(hipStreamSynchronize(a->copy_stream));
    const size_t next = done + k, k_next = std::min(bytes - next, kPinnedChunk);
    if (k_next) WCHK(hipMemcpyAsync(a->pinned + (size_t)(b ^ 1) * kPinnedChunk, a->stage + off + next, k_next, hipMemcpyDeviceToHost, a->copy_stream));
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
  if (fetch_dev(a, a->off_rec, sizeof rec, &rec, err)) return 1;
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
    if (fetch_dev(a, a->off_crc + (size_t)c.chunk0 * sizeof(uint32_t), chunks * sizeof(uint32_t), raws.data(), err)) return 1;
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
    if (o.dev_ix >= 0) { if (stream_dev(a, dev[o.dev_ix].off, (size_t)dev[o.dev_ix].bytes, &w, err)) return 1; }
    else if (w.append(o.host, o.bytes, err)) return 1;
  }
  return w.finish(err);
}

void writer_main(StateAsync* a) {
  // the learner captures its graphs in thread-local mode; this thread's copies and waits are checked against its own captures (none)
  hipStreamCaptureMode mode = hipStreamCaptureModeThreadLocal;
  (void)hipThreadExchangeStreamCaptureMode(&mode);
  std::unique_lock<std::mutex> lk(a->mu);
  for (;;) {
    a->cv.wait(lk, [a] { return a->pending || a->quit; });
    if (!a->pending) return;             // quit, and nothing left to write
    a->pending = false;
    lk.unlock();
    std::string err;
    const int rc = write_job(a, &err);
    lk.lock();
    a->failed = rc != 0; a->err = err;
    a->busy = false;
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

// first use: the staging buffer's map, the four HIP objects, the segment table, the writer thread
int state_async_init(H* h) {
  if (h->sasync) return 0;
  std::unique_ptr<StateAsync> up(new StateAsync);
  StateAsync* a = up.get();
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
  a->stage = (uint8_t*)p;
  auto bail = [&](int rc) {
    if (a->ev) hipEventDestroy(a->ev);
    if (a->copy_stream) hipStreamDestroy(a->copy_stream);
    if (a->pinned) hipHostFree(a->pinned);
    hipFree(a->stage);
    return rc;
  };
#define ICHK(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return bail(fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__)); } while (0)
  ICHK(hipHostMalloc((void**)&a->pinned, 2 * kPinnedChunk, hipHostMallocDefault));
  ICHK(hipStreamCreateWithFlags(&a->copy_stream, hipStreamNonBlocking));
  ICHK(hipEventCreateWithFlags(&a->ev, hipEventDisableTiming));
  // the segment table: W of the four nets, then (m, v) of the two online nets — the order of the parameter sections
  const float* arenas[8] = {h->w[0], h->w[1], h->w[2], h->w[3], h->m[0], h->v[0], h->m[1], h->v[1]};
  for (int i = 0; i < 8; ++i) {
    const int net = i < 4 ? i : (i - 4) / 2;
    if (arena_segs(layout_of(h, net), arenas[i], (float*)(a->stage + a->off_par[i]), &a->segs)) return bail(1);
  }
  a->n_seg = (int)a->segs.size();
  if (a->n_seg > max_segs) return bail(fail("dqnhip_save_state_async: %d parameter pieces, room for %d", a->n_seg, max_segs));
  ICHK(hipMemcpyAsync(a->stage + a->off_segs, a->segs.data(), a->segs.size() * sizeof(PackSeg), hipMemcpyHostToDevice, h->stream));
  ICHK(hipStreamSynchronize(h->stream));
#undef ICHK
  uint32_t op[32];
  crc_zeros_op(op, kCrcChunk);
  crc_op_table(a->chunk_tab, op);
  a->th = std::thread(writer_main, a);
  h->sasync = up.release();
  return 0;
}

}  // namespace

namespace dqnhip_host {

int state_async_join(H* h, const char* what) {
  StateAsync* a = h->sasync;
  if (!a) return 0;
  std::unique_lock<std::mutex> lk(a->mu);
  a->cv.wait(lk, [a] { return !a->busy; });
  if (!a->failed) return 0;
  a->failed = false;
  return fail("%s: the asynchronous save of %s failed: %s", what, a->job.filename.c_str(), a->err.c_str());
}

void state_async_free(H* h) {
  StateAsync* a = h->sasync;
  if (!a) return;
  {
    std::unique_lock<std::mutex> lk(a->mu);
    a->cv.wait(lk, [a] { return !a->busy; });
    a->quit = true;
    a->cv.notify_all();
  }
  a->th.join();
  hipEventDestroy(a->ev); hipStreamDestroy(a->copy_stream); hipHostFree(a->pinned); hipFree(a->stage);
  delete a;
  h->sasync = nullptr;
}

}  // namespace dqnhip_host

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
  a->failed = false; a->err.clear();
  a->pending = true; a->busy = true;
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
  *done = a->busy ? 0 : 1;
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
