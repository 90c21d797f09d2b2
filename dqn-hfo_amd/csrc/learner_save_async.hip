// learner_save_async.hip — the two saves that run behind training: their pack and checksum launches (state_kernels.hip.h,
// snapshot_kernels.hip.h), their host side, and the writer thread they share.
// dqnhip_save_state_async: the file of dqnhip_save_state (learner_state.hip; the same manifest, state_codec.h).  The caller's thread
// enqueues the pack and the chunk CRCs on the learner's stream and posts a job to the writer, which waits for the event, folds the
// CRCs, and streams the staging buffer to the file through two pinned chunks.
// dqnhip_snapshot_async: the Caffe snapshot's files, a second kind of job for the same writer.  The caller's thread enqueues the
// parameter pack, the `.replaymemory` stream and its CRC into a staging buffer of the snapshot's own; the writer builds the protobuf
// files with snapshot.cpp's builders and hands the stream to GzipParallelWriter.
#include <condition_variable>
#include <functional>
#include <memory>

#include "learner_state.hip.h"
#include "gzip_parallel.h"
#include "snapshot_codec.h"
#include "snapshot_stream.h"
#include "state_kernels.hip.h"
#include "snapshot_kernels.hip.h"

using namespace dqnhip_state;

namespace dqnhip_host {

constexpr size_t kPinnedChunk = (size_t)8 << 20;       // the pinned ring: two of these
enum JobKind { kJobState = 0, kJobSnapshot = 1, kJobKinds = 2 };

// One kind of job's device staging buffer, allocated by the first job of its kind and kept until dqnhip_destroy.  Its map (byte
// offsets, everything on a 16-byte boundary): the record, the segment table, the chunk CRCs, the dense parameter arrays; what lies
// behind them is the kind's own.
struct Stage {
  uint8_t* buf = nullptr; size_t bytes = 0;
  hipEvent_t ev = nullptr;
  size_t off_rec = 0, off_segs = 0, off_crc = 0;
  std::vector<size_t> off_par, par_bytes;
  int n_seg = 0;
};

// what one save needs besides the staging buffer: fixed on the caller's thread, read by the writer
struct StateJob {
  std::string filename;
  int32_t flags = 0;
  StateShape shape{};                    // ring_size comes from the record
  FixedSections fixed{};                 // the host's share; DEVS, LSCL, RING and PERC's p_max come from the record
  std::vector<uint8_t> user;
  dqnhip_config cfg{};                   // the header's share of it, the device, the ring's capacity
};
struct StateStage : Stage {
  size_t off_ring[kRingArrays] = {0};
  CrcArgs crc{};                         // the launch of the save in flight (the writer reads chunk0 / the offsets)
  StateJob job;
};

// what one asynchronous snapshot needs besides its staging buffer
struct SnapJob {
  std::string save_path, prefix;
  bool remove_old = false, with_mem = false;
  int workers = 8;
  dqnhip_config cfg{};
};
constexpr int kSnapPar = 6;              // W actor, W critic, history 1 / 2 of the actor, history 1 / 2 of the critic
struct SnapStage : Stage {
  // the stream (its records start on a 16-byte boundary: the count sits in the 4 bytes before one), the guard band behind its upper bound
  size_t off_stream = 0, off_guard = 0;
  SnapJob job;
  int32_t actor_iter = 0, critic_iter = 0;       // of the last job that wrote its files
};

// The writer both kinds of job share, allocated by whichever comes first: the thread and its queue, the pinned ring, the copy stream,
// the combine table.  The thread touches only a job's stage, the job and its own copy stream — never the learner, the learner's
// stream or an event recorded on that stream (which may be capturing by then).
struct SaveWriter {
  uint8_t* pinned = nullptr;
  hipStream_t copy_stream = nullptr;
  uint32_t chunk_tab[kCrcTableWords];    // crc_op_table of Z_kCrcChunk
  StateStage* state = nullptr;           // null: this learner has only snapshotted asynchronously
  SnapStage* snap = nullptr;             // ... only saved its state
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<int> queue;                 // the kinds of the jobs that wait for the thread, first in first out
  bool busy[kJobKinds] = {false, false}; // a job of this kind is in flight (waiting or being written): at most one of each
  bool quit = false;
  // of the last job of each kind: what it writes ("save of <file>"), and its failure until a join reports it
  std::string subject[kJobKinds], err[kJobKinds];
  bool failed[kJobKinds] = {false, false};

  // the copy stream's wait for the stage's event — every copy of the job is behind the image — and the job into the queue
  int post(int kind, hipEvent_t ev, const std::string& what_it_writes) {
    HIPCHK(hipStreamWaitEvent(copy_stream, ev, 0));
    std::lock_guard<std::mutex> lk(mu);
    subject[kind] = what_it_writes;
    failed[kind] = false; err[kind].clear();
    queue.push_back(kind); busy[kind] = true;
    cv.notify_all();
    return 0;
  }
  // waits for the job of `kind` in flight; its failure, once, as `what`'s
  int join(int kind, const char* what) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [this, kind] { return !busy[kind]; });
    if (!failed[kind]) return 0;
    failed[kind] = false;
    return fail("%s: the asynchronous %s failed: %s", what, subject[kind].c_str(), err[kind].c_str());
  }
  bool poll(int kind) { std::lock_guard<std::mutex> lk(mu); return !busy[kind]; }
};

}  // namespace dqnhip_host

namespace {

std::string hip_msg(const char* what, hipError_t e) { return std::string(what) + " failed: " + hipGetErrorString(e); }
#define WCHK(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { *err = hip_msg(#expr, e__); return 1; } } while (0)

// `bytes` bytes of a staging buffer at src -> dst (host memory of any kind), through the pinned ring
int fetch_dev(SaveWriter* w, const uint8_t* src, size_t bytes, void* dst, std::string* err) {
  for (size_t done = 0; done < bytes;) {
    const size_t k = std::min(bytes - done, kPinnedChunk);
    WCHK(hipMemcpyAsync(w->pinned, src + done, k, hipMemcpyDeviceToHost, w->copy_stream));
    WCHK(hipStreamSynchronize(w->copy_stream));
    memcpy((char*)dst + done, w->pinned, k);
    done += k;
  }
  return 0;
}
// ... -> the file (StreamWriter, GzipParallelWriter): the copy of chunk k + 1 runs while chunk k is written
template <class Writer>
int stream_dev(SaveWriter* w, const uint8_t* src, size_t bytes, Writer* out, std::string* err) {
  if (!bytes) return 0;
  int b = 0;
  size_t k = std::min(bytes, kPinnedChunk);
  WCHK(hipMemcpyAsync(w->pinned, src, k, hipMemcpyDeviceToHost, w->copy_stream));
  for (size_t done = 0; done < bytes;) {
    WCHK(hipStreamSynchronize(w->copy_stream));
    const size_t next = done + k, k_next = std::min(bytes - next, kPinnedChunk);
    if (k_next) WCHK(hipMemcpyAsync(w->pinned + (size_t)(b ^ 1) * kPinnedChunk, src + next, k_next, hipMemcpyDeviceToHost, w->copy_stream));
    if (out->append(w->pinned + (size_t)b * kPinnedChunk, k, err)) return 1;
    done = next; k = k_next; b ^= 1;
  }
  return 0;
}
// the record at the front of a stage, and the window it names checked against the ring's capacity
int fetch_rec(SaveWriter* w, const Stage* s, const dqnhip_config& c, bool with_mem, StateRec* rec, std::string* err) {
  WCHK(hipSetDevice(c.device));
  // (the copy stream already waits for the stage's event — SaveWriter::post enqueued that wait)
  if (fetch_dev(w, s->buf + s->off_rec, sizeof *rec, rec, err)) return 1;
  if (with_mem) *err = ring_range_error(rec->ring_head, rec->ring_size, c.replay_capacity);
  return err->empty() ? 0 : 1;
}

// The writer thread's share of one save: the file's sections by the manifest, the device-checksummed ones out of the staging buffer.
int write_state_job(SaveWriter* w, std::string* err) {
  const StateStage* s = w->state;
  const StateJob& j = s->job;
  StateRec rec{};
  if (fetch_rec(w, s, j.cfg, j.shape.with_memory, &rec, err)) return 1;
  StateShape shape = j.shape;
  shape.ring_size = shape.with_memory ? rec.ring_size : 0;
  FixedSections fixed = j.fixed;
  fixed.user = j.user.data();
  fixed.dev = DevSection{rec.actor_iter, rec.critic_iter, rec.update_counter, rec.critic_loss, rec.avg_q, rec.flags, rec.skipped_steps};
  fixed.ls = LossScaleSection{{rec.ls_mult[0], rec.ls_mult[1]}, {rec.ls_good[0], rec.ls_good[1]}, {rec.ls_backoffs[0], rec.ls_backoffs[1]},
                              {rec.ls_growths[0], rec.ls_growths[1]}};
  fixed.ring = RingSection{rec.ring_head, rec.ring_size};
  fixed.per.p_max = rec.p_max;
  // the launch checksummed the eight parameter sections, then the ring's arrays: sec[index] / sec[kParSections + index]
  const std::vector<ManifestEntry> man = manifest(shape);
  std::vector<StreamEntry> entries;
  std::vector<uint32_t> raws;
  for (const ManifestEntry& e : man) {
    if (e.src != Src::Par && e.src != Src::RingArray) { entries.push_back({e.tag, crc32_of(fixed.of(e.src), e.bytes), e.bytes}); continue; }
    const CrcSection& c = s->crc.sec[e.src == Src::Par ? e.index : kParSections + e.index];
    raws.resize((size_t)((e.bytes + kCrcChunk - 1) / kCrcChunk));
    if (fetch_dev(w, s->buf + s->off_crc + (size_t)c.chunk0 * sizeof(uint32_t), raws.size() * sizeof(uint32_t), raws.data(), err)) return 1;
    entries.push_back({e.tag, crc_fold_chunks(raws.data(), e.bytes, w->chunk_tab), e.bytes});
  }
  const dqnhip_state_info_t info = info_of(j.cfg, j.flags, shape, rec.actor_iter, rec.critic_iter, rec.update_counter);
  StreamWriter out;
  if (out.open(j.filename.c_str(), info, entries, err)) return 1;
  for (const ManifestEntry& e : man) {
    if (e.src == Src::Par) { if (stream_dev(w, s->buf + s->off_par[e.index], (size_t)e.bytes, &out, err)) return 1; }
    else if (e.src == Src::RingArray) { if (stream_dev(w, s->buf + s->off_ring[e.index], (size_t)e.bytes, &out, err)) return 1; }
    else if (out.append(fixed.of(e.src), e.bytes, err)) return 1;
  }
  return out.finish(err);
}

// The writer thread's share of one asynchronous snapshot.  Order and names are dqnhip_snapshot's; every file appears under a name
// only when it is complete.
int write_snap_job(SaveWriter* w, std::string* err) {
  SnapStage* s = w->snap;
  const SnapJob& j = s->job;
  StateRec rec{};
  if (fetch_rec(w, s, j.cfg, j.with_mem, &rec, err)) return 1;
  if (j.with_mem) {
    uint32_t guard[dqnhip_snap::kGuardWords];
    if (fetch_dev(w, s->buf + s->off_guard, sizeof guard, guard, err)) return 1;
    for (int i = 0; i < dqnhip_snap::kGuardWords; ++i)
      if (guard[i] != dqnhip_snap::kGuardWord) { *err = "guard word " + std::to_string(i) + " behind the replay-memory stream was overwritten; no file was written"; return 1; }
  }
  // ---- the four protobuf files, from the staged dense arrays ----
  std::vector<float> par[kSnapPar];
  for (int i = 0; i < kSnapPar; ++i) {
    par[i].resize(s->par_bytes[i] / sizeof(float));
    if (fetch_dev(w, s->buf + s->off_par[i], s->par_bytes[i], par[i].data(), err)) return 1;
  }
  const int iters[2] = {rec.actor_iter, rec.critic_iter};
  const dqnhip_snap::Names names = dqnhip_snap::names_of(j.save_path, j.prefix, iters[0], iters[1]);
  for (int net = 0; net < 2; ++net) {
    const std::string& from = names.from[net];
    if (dqnhip_snap::publish_file(from + ".caffemodel", dqnhip_snap::caffemodel_bytes(j.cfg, net, par[net].data()), err)) return 1;
    const float* h2 = dqnhip_snap::two_histories(j.cfg.solver_type) ? par[3 + 2 * net].data() : nullptr;
    if (dqnhip_snap::publish_file(from + ".solverstate", dqnhip_snap::solverstate_bytes(j.cfg, net, iters[net], from + ".caffemodel", par[2 + 2 * net].data(), h2), err)) return 1;
  }
  for (int net = 0; net < 2; ++net)
    for (const char* ext : {".caffemodel", ".solverstate"})
      if (dqnhip_snap::move_file(names.from[net] + ext, names.to[net] + ext, err)) return 1;
  // ---- the replay memory: one gzip member, the trailer's CRC from the device ----
  if (j.with_mem) {
    const int32_t count = rec.ring_size;
    const uint64_t rec_bytes = (uint64_t)count * dqnhip_snap::record_bytes(j.cfg.state_size);
    std::vector<uint32_t> raws((size_t)((rec_bytes + kCrcChunk - 1) / kCrcChunk));
    if (fetch_dev(w, s->buf + s->off_crc, raws.size() * sizeof(uint32_t), raws.data(), err)) return 1;
    // k_state_crc checksums the records; the count in front is four bytes the host knows: crc(A || B) = Z_|B|(crc(A)) ^ crc(B),
    // zlib's crc32_combine
    const uint32_t crc = (uint32_t)crc32_combine(crc32_of(&count, sizeof count), crc_fold_chunks(raws.data(), rec_bytes, w->chunk_tab), (z_off_t)rec_bytes);
    GzipParallelWriter out;
    if (out.open(names.memory.c_str(), j.workers, GzipParallelWriter::kDefaultChunk, err)) return 1;
    if (stream_dev(w, s->buf + s->off_stream, (size_t)(4 + rec_bytes), &out, err)) return 1;
    if (out.finish(crc, err)) return 1;
  }
  if (j.remove_old) dqnhip_snap::remove_old_snapshots(j.prefix, iters[0], iters[1]);      // only now: all of this job's files are in place
  s->actor_iter = iters[0]; s->critic_iter = iters[1];
  return 0;
}

void writer_main(SaveWriter* w) {
  // the learner captures its graphs in thread-local mode; this thread's copies and waits are checked against its own captures (none)
  hipStreamCaptureMode mode = hipStreamCaptureModeThreadLocal;
  (void)hipThreadExchangeStreamCaptureMode(&mode);
  std::unique_lock<std::mutex> lk(w->mu);
  for (;;) {
    w->cv.wait(lk, [w] { return !w->queue.empty() || w->quit; });
    if (w->queue.empty()) return;        // quit, and nothing left to write
    const int kind = w->queue.front();
    w->queue.pop_front();
    lk.unlock();
    std::string err;
    const int rc = kind == kJobState ? write_state_job(w, &err) : write_snap_job(w, &err);
    lk.lock();
    w->failed[kind] = rc != 0; w->err[kind] = err;
    w->busy[kind] = false;
    w->cv.notify_all();
  }
}

// first use of either kind of job: the writer
int writer_init(H* h) {
  if (h->sasync) return 0;
  std::unique_ptr<SaveWriter> up(new SaveWriter);
  SaveWriter* w = up.get();
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipHostMalloc((void**)&w->pinned, 2 * kPinnedChunk, hipHostMallocDefault));
  const hipError_t e = hipStreamCreateWithFlags(&w->copy_stream, hipStreamNonBlocking);
  if (e != hipSuccess) { hipHostFree(w->pinned); return fail("hipStreamCreateWithFlags failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__); }
  uint32_t op[32];
  crc_zeros_op(op, kCrcChunk);
  crc_op_table(w->chunk_tab, op);
  w->th = std::thread(writer_main, w);
  h->sasync = up.release();
  return 0;
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

uint64_t crc_chunks(uint64_t bytes) { return (bytes + kCrcChunk - 1) / kCrcChunk; }

// First job of a kind: its staging buffer.  The map — the record, the segment table, `chunks` chunk CRCs, the dense image of every
// arena in `par` (staged false: an empty one), then whatever `rest` lays out from the offset it is given (it returns the buffer's
// size) — the buffer, its event, and the segment table uploaded.  A failure leaves nothing allocated.
struct StagePar { const float* arena; int net; bool staged; };
int stage_alloc(H* h, Stage* s, const char* who, const char* no_memory_fmt, const std::vector<StagePar>& par, uint64_t chunks,
                const std::function<size_t(size_t)>& rest) {
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off = round_up_z(off + bytes, 16); return at; };
  const int max_segs = (int)par.size() * (2 * kMaxL + 4);
  s->off_rec = take(sizeof(StateRec));
  s->off_segs = take((size_t)max_segs * sizeof(PackSeg));
  s->off_crc = take((size_t)chunks * sizeof(uint32_t));
  for (const StagePar& p : par) {
    s->par_bytes.push_back(p.staged ? layout_of(h, p.net).dense * sizeof(float) : 0);
    s->off_par.push_back(take(s->par_bytes.back()));
  }
  s->bytes = rest(off);
  HIPCHK(hipSetDevice(h->cfg.device));
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, s->bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(no_memory_fmt, who, s->bytes, hipGetErrorString(e));
  }
  s->buf = (uint8_t*)p;
  auto bail = [&](int rc) {
    if (s->ev) hipEventDestroy(s->ev);
    hipFree(s->buf);
    return rc;
  };
#define ICHK(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return bail(fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__)); } while (0)
  ICHK(hipEventCreateWithFlags(&s->ev, hipEventDisableTiming));
  std::vector<PackSeg> segs;             // (the host copy of the table at off_segs: its upload reads it)
  for (size_t i = 0; i < par.size(); ++i)
    if (s->par_bytes[i] && arena_segs(layout_of(h, par[i].net), par[i].arena, (float*)(s->buf + s->off_par[i]), &segs)) return bail(1);
  s->n_seg = (int)segs.size();
  if (s->n_seg > max_segs) return bail(fail("%s: %d parameter pieces, room for %d", who, s->n_seg, max_segs));
  ICHK(hipMemcpyAsync(s->buf + s->off_segs, segs.data(), segs.size() * sizeof(PackSeg), hipMemcpyHostToDevice, h->stream));
  ICHK(hipStreamSynchronize(h->stream));
#undef ICHK
  return 0;
}

// first asynchronous save: behind the parameters, the ring's arrays at their longest
int state_stage_init(H* h) {
  RC(writer_init(h));
  if (h->sasync->state) return 0;
  std::unique_ptr<StateStage> up(new StateStage);
  StateStage* s = up.get();
  const size_t cap = (size_t)h->ring.cap;
  // the order of the parameter sections (state_codec.h: kTagPar)
  const std::vector<StagePar> par = {{h->w[0], 0, true}, {h->w[1], 1, true}, {h->w[2], 2, true}, {h->w[3], 3, true},
                                     {h->m[0], 0, true}, {h->v[0], 0, true}, {h->m[1], 1, true}, {h->v[1], 1, true}};
  uint64_t chunks = 0;
  for (const StagePar& p : par) chunks += crc_chunks(layout_of(h, p.net).dense * sizeof(float));
  for (int i = 0; i < kRingArrays; ++i) chunks += crc_chunks(cap * ring_row_bytes(i, h->S));
  if (chunks > 0x7fffffffull) return fail("dqnhip_save_state_async: this learner's file is too large for the chunk table");
  RC(stage_alloc(h, s, "dqnhip_save_state_async", "%s: cannot allocate the device staging buffer of %zu bytes (%s); the learner is untouched and "
                 "dqnhip_save_state, which needs none, still works", par, chunks, [&](size_t off) {
    for (int i = 0; i < kRingArrays; ++i) { s->off_ring[i] = off; off = round_up_z(off + cap * ring_row_bytes(i, h->S), 16); }
    return off;
  }));
  h->sasync->state = up.release();
  return 0;
}

// first asynchronous snapshot: the same for the snapshot's own staging buffer — the two kinds of job can be in flight together
int snap_stage_init(H* h) {
  RC(writer_init(h));
  if (h->sasync->snap) return 0;
  std::unique_ptr<SnapStage> up(new SnapStage);
  SnapStage* s = up.get();
  const uint64_t cap = (uint64_t)h->ring.cap, chunks = crc_chunks(cap * dqnhip_snap::record_bytes(h->S));
  if (chunks > 0x7fffffffull) return fail("dqnhip_snapshot_async: this learner's replay memory is too large for the chunk table");
  // the builders of snapshot.cpp index the dense arrays by their own blob table: the two must describe the same array
  for (int net = 0; net < 2; ++net)
    if (dqnhip_snap::dense_count(h->cfg, net) != (size_t)layout_of(h, net).dense)
      return fail("dqnhip_snapshot_async: the snapshot codec counts %zu dense parameters in net %d, the learner %zu", dqnhip_snap::dense_count(h->cfg, net), net,
                  (size_t)layout_of(h, net).dense);
  // W of actor and critic, then (history 1, history 2) of each; a single-history solver has no second set
  const bool two = dqnhip_snap::two_histories(h->cfg.solver_type);
  const std::vector<StagePar> par = {{h->w[0], 0, true}, {h->w[1], 1, true}, {h->m[0], 0, true}, {h->v[0], 0, two}, {h->m[1], 1, true}, {h->v[1], 1, two}};
  RC(stage_alloc(h, s, "dqnhip_snapshot_async", "%s: the asynchronous snapshot cannot allocate its device staging buffer of %zu bytes (%s); the learner is "
                 "untouched and dqnhip_snapshot, which needs none, still works", par, chunks, [&](size_t off) {
    // the count's four bytes end on a 16-byte boundary: k_snap_pack_replay stores whole 16-byte pieces of records, their CRC reads whole lines
    s->off_stream = off + 12;
    s->off_guard = s->off_stream + 4 * (size_t)dqnhip_snap::stream_dwords(h->S, cap);
    return round_up_z(s->off_guard + dqnhip_snap::kGuardWords * sizeof(uint32_t), 16);
  }));
  h->sasync->snap = up.release();
  return 0;
}

void stage_free(Stage* s) { hipEventDestroy(s->ev); hipFree(s->buf); }

// ---- the launchers of state_kernels.hip.h, on the learner's stream ----
int state_pack_params_launch(H* h, const PackSeg* segs_dev, int n_seg, StateRec* rec_dev) {
  HIPCHK(launch(h->stream, k_state_pack_params, dim3(64, n_seg + 1), dim3(256), 0, segs_dev, n_seg, (const DevState*)h->st, per_p_max_dev(h), rec_dev));
  return 0;
}
int state_pack_ring_launch(H* h, const RingPackArgs& a) {
  if (a.cap < 1 || a.n_arr < 1 || a.n_arr > kRingArrays) return fail("state_pack_ring_launch: bad arguments");
  HIPCHK(launch(h->stream, k_state_pack_ring, dim3((a.cap + kPackRows - 1) / kPackRows, a.n_arr), dim3(256), 0, a));
  return 0;
}
int state_crc_launch(H* h, const CrcArgs& a) {
  if (a.n < 1 || a.n > kMaxCrcSections) return fail("state_crc_launch: bad arguments");
  if (a.total_chunks == 0) return 0;
  HIPCHK(launch(h->stream, k_state_crc, dim3((a.total_chunks + 255) / 256), dim3(256), 0, a));
  return 0;
}
// asynchronous Caffe snapshot (snapshot_kernels.hip.h): the ring's window as the `.replaymemory` stream at `stream_dev`, which has
// room for the stream of a full ring and, behind that (rounded up to a dword), the guard band this call fills and nothing else writes.
// The stream's first record (stream_dev + 4) lies on a 16-byte boundary.  64 records per workgroup measured fastest
// (profiles/snapshot_async_ab.md); fewer where the state is so long that 64 rows do not fit the LDS a launch gets without asking
int snap_pack_replay_launch(H* h, uint8_t* stream_dev) {
  const uint64_t max_dwords = dqnhip_snap::stream_dwords(h->S, (uint64_t)h->ring.cap);
  const size_t row_bytes = (size_t)dqnhip_snap::snap_lds_row_words(h->S) * sizeof(uint32_t);
  int K = 64;
  while (K > 16 && K * row_bytes > 48 * 1024) K /= 2;
  if (K * row_bytes > 48 * 1024) return fail("the asynchronous snapshot's pack kernel stages 16 records of %zu bytes in LDS: too long a state (S = %d)", row_bytes, h->S);
  if ((uintptr_t)(stream_dev + 4) % 16 != 0 || h->ring.cap < 1) return fail("snap_pack_replay_launch: bad arguments");
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(stream_dev + 4 * max_dwords), (int)dqnhip_snap::kGuardWord, dqnhip_snap::kGuardWords, h->stream));
  HIPCHK(launch(h->stream, k_snap_pack_replay, dim3((unsigned)((h->ring.cap + K - 1) / K)), dim3(256), K * row_bytes, h->ring, (const DevState*)h->st,
                (uint32_t*)stream_dev, max_dwords, K));
  return 0;
}

}  // namespace

namespace dqnhip_host {

int state_async_join(H* h, const char* what) { return h->sasync ? h->sasync->join(kJobState, what) : 0; }
int snapshot_async_join(H* h, const char* what) { return h->sasync ? h->sasync->join(kJobSnapshot, what) : 0; }

void state_async_free(H* h) {
  SaveWriter* w = h->sasync;
  if (!w) return;
  {
    std::unique_lock<std::mutex> lk(w->mu);
    w->cv.wait(lk, [w] { return !w->busy[kJobState] && !w->busy[kJobSnapshot]; });
    w->quit = true;
    w->cv.notify_all();
  }
  w->th.join();
  if (w->snap) { stage_free(w->snap); delete w->snap; }
  if (w->state) { stage_free(w->state); delete w->state; }
  hipStreamDestroy(w->copy_stream); hipHostFree(w->pinned);
  delete w;
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
  RC(state_stage_init(h));
  StateStage* s = h->sasync->state;
  // ---- the learner's stream: pack, checksum, event ----
  RC(state_pack_params_launch(h, (const PackSeg*)(s->buf + s->off_segs), s->n_seg, (StateRec*)(s->buf + s->off_rec)));
  RingDev ring[kRingArrays];
  const int n_arr = with_mem ? ring_arrays_of(h, ring) : 0;
  if (with_mem) {
    RingPackArgs r{};
    r.st = h->st; r.cap = h->ring.cap; r.n_arr = n_arr;
    for (int i = 0; i < n_arr; ++i) {
      const RingDev& g = ring[i];
      r.arr[i] = RingArr{g.ptr, s->buf + s->off_ring[i], g.width, g.pitch, g.elem, g.elem == 4 && g.width % 4 == 0 && g.pitch % 4 == 0};
    }
    RC(state_pack_ring_launch(h, r));
  }
  CrcArgs& c = s->crc;                   // (no save is in flight: the writer does not read it now)
  c = CrcArgs{};
  c.base = s->buf; c.rec = (const StateRec*)(s->buf + s->off_rec); c.out = (uint32_t*)(s->buf + s->off_crc);
  c.max_rows = h->ring.cap;
  uint32_t chunk0 = 0;
  for (int i = 0; i < kParSections; ++i) {
    c.sec[c.n++] = CrcSection{s->off_par[i], s->par_bytes[i], 0u, chunk0};
    chunk0 += (uint32_t)crc_chunks(s->par_bytes[i]);
  }
  for (int i = 0; i < n_arr; ++i) {
    c.sec[c.n++] = CrcSection{s->off_ring[i], 0, ring_row_bytes(i, h->S), chunk0};
    chunk0 += (uint32_t)crc_chunks((uint64_t)h->ring.cap * ring_row_bytes(i, h->S));
  }
  c.total_chunks = chunk0;
  RC(state_crc_launch(h, c));
  HIPCHK(hipEventRecord(s->ev, h->stream));
  // ---- the job: everything the writer needs of the host, as it is now ----
  StateJob& j = s->job;
  j = StateJob{};
  j.filename = filename; j.flags = flags;
  j.shape = state_shape_of(h, with_mem, 0, user_bytes);
  j.fixed = state_fixed_of(h);
  if (user_bytes) j.user.assign((const uint8_t*)user, (const uint8_t*)user + user_bytes);
  j.cfg = h->cfg;
  return h->sasync->post(kJobState, s->ev, "save of " + j.filename);
}

int dqnhip_save_state_wait(dqnhip_handle h) {
  if (!h) return fail("dqnhip_save_state_wait: null argument");
  return state_async_join(h, "dqnhip_save_state_wait");
}

int dqnhip_save_state_poll(dqnhip_handle h, int32_t* done) {
  if (!h || !done) return fail("dqnhip_save_state_poll: null argument");
  *done = !h->sasync || h->sasync->poll(kJobState);
  return 0;
}

int dqnhip_snapshot_async(dqnhip_handle h, const char* save_path, const char* snapshot_prefix, int32_t remove_old, int32_t snapshot_memory,
                          int32_t compress_threads) {
  if (!h || !save_path || !snapshot_prefix) return fail("dqnhip_snapshot_async: null argument");
  if (compress_threads < 0 || compress_threads > 64) return fail("dqnhip_snapshot_async: compress_threads %d is outside 0 ... 64 (0: the default, 8)", compress_threads);
  RC(state_refuse(h, "dqnhip_snapshot_async: the asynchronous snapshot"));
  RC(snapshot_async_join(h, "dqnhip_snapshot_async"));      // one snapshot in flight per learner
  HIPCHK(hipSetDevice(h->cfg.device));
  RC(snap_stage_init(h));
  SnapStage* s = h->sasync->snap;
  // ---- the learner's stream: parameters and record, the stream, its checksum, event ----
  RC(state_pack_params_launch(h, (const PackSeg*)(s->buf + s->off_segs), s->n_seg, (StateRec*)(s->buf + s->off_rec)));
  if (snapshot_memory) {
    RC(snap_pack_replay_launch(h, s->buf + s->off_stream));
    CrcArgs c{};
    c.base = s->buf; c.rec = (const StateRec*)(s->buf + s->off_rec); c.out = (uint32_t*)(s->buf + s->off_crc);
    c.max_rows = h->ring.cap; c.n = 1;
    const uint32_t R = (uint32_t)dqnhip_snap::record_bytes(h->S);
    c.sec[0] = CrcSection{s->off_stream + 4, 0, R, 0u};       // the records; the count in front of them is the host's to add
    c.total_chunks = (uint32_t)crc_chunks((uint64_t)h->ring.cap * R);
    RC(state_crc_launch(h, c));
  }
  HIPCHK(hipEventRecord(s->ev, h->stream));
  // ---- the job ----
  SnapJob& j = s->job;
  j = SnapJob{};
  j.save_path = save_path; j.prefix = snapshot_prefix; j.remove_old = remove_old != 0; j.with_mem = snapshot_memory != 0;
  j.workers = compress_threads ? compress_threads : 8;       // (never derived from the machine's CPU count: a container may grant fewer)
  j.cfg = h->cfg;
  return h->sasync->post(kJobSnapshot, s->ev, "snapshot to " + j.prefix);
}

int dqnhip_snapshot_wait(dqnhip_handle h, int32_t* actor_iter, int32_t* critic_iter) {
  if (!h) return fail("dqnhip_snapshot_wait: null argument");
  RC(snapshot_async_join(h, "dqnhip_snapshot_wait"));
  const SnapStage* s = h->sasync ? h->sasync->snap : nullptr;
  if (actor_iter) *actor_iter = s ? s->actor_iter : 0;
  if (critic_iter) *critic_iter = s ? s->critic_iter : 0;
  return 0;
}

int dqnhip_snapshot_poll(dqnhip_handle h, int32_t* done) {
  if (!h || !done) return fail("dqnhip_snapshot_poll: null argument");
  *done = !h->sasync || h->sasync->poll(kJobSnapshot);
  return 0;
}

// k_state_crc on caller-supplied bytes, through the learner's staging buffer: the door the tests check the device checksum through
int dqnhip_state_crc32_device(dqnhip_handle h, const void* host_bytes, size_t bytes, int32_t misalign, uint32_t* crc) {
  if (!h || !crc || (!host_bytes && bytes)) return fail("dqnhip_state_crc32_device: null argument");
  if (misalign < 0 || misalign > 15) return fail("dqnhip_state_crc32_device: misalign %d is outside 0 ... 15", misalign);
  if (bytes > ((size_t)1 << 31)) return fail("dqnhip_state_crc32_device: %zu bytes are more than this door takes (2^31)", bytes);
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t chunks = (bytes + kCrcChunk - 1) / kCrcChunk, out_off = round_up_z((size_t)misalign + bytes, 16);
  RC(ensure_stage(h, out_off + chunks * sizeof(uint32_t) + 16));
  uint8_t* base = (uint8_t*)h->stage_dev;
  if (bytes) HIPCHK(hipMemcpyAsync(base + misalign, host_bytes, bytes, hipMemcpyHostToDevice, h->stream));
  CrcArgs a{};
  a.base = base; a.rec = nullptr; a.out = (uint32_t*)(base + out_off); a.n = 1; a.max_rows = 0; a.total_chunks = (uint32_t)chunks;
  a.sec[0] = CrcSection{(uint64_t)misalign, (uint64_t)bytes, 0u, 0u};
  RC(state_crc_launch(h, a));
  std::vector<uint32_t> raws(chunks);
  if (chunks) HIPCHK(hipMemcpyAsync(raws.data(), a.out, chunks * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  uint32_t op[32];
  std::vector<uint32_t> tab(kCrcTableWords);
  crc_zeros_op(op, kCrcChunk);
  crc_op_table(tab.data(), op);
  *crc = crc_fold_chunks(raws.data(), bytes, tab.data());
  return 0;
}

}  // extern "C"
