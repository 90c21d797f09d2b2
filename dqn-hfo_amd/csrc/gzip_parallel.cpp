// gzip_parallel.cpp — GzipParallelWriter (gzip_parallel.h): one gzip member, its chunks deflated by a pool of threads and written in
// order by the caller's thread.  No device code, no HIP.
#include "gzip_parallel.h"

#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cerrno>
#include <cstring>

namespace dqnhip_state {

namespace {

// what gzopen("wb") + gzwrite put in front: magic, deflate, no flags, no mtime, no extra flags, OS 3 (Unix)
const uint8_t kGzipHeader[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};

// one chunk as a raw deflate stream of its own, at the level, memory level and strategy of gzopen("wb")
int deflate_chunk(const std::vector<uint8_t>& in, bool last, std::vector<uint8_t>* out) {
  z_stream z;
  memset(&z, 0, sizeof z);
  if (deflateInit2(&z, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return 1;
  out->resize((size_t)deflateBound(&z, (uLong)in.size()) + 64);      // (+ the empty stored block of a sync flush)
  static const uint8_t none = 0;
  z.next_in = (Bytef*)(in.empty() ? &none : in.data()); z.avail_in = (uInt)in.size();
  z.next_out = out->data(); z.avail_out = (uInt)out->size();
  const int rc = deflate(&z, last ? Z_FINISH : Z_SYNC_FLUSH);
  const bool ok = (last ? rc == Z_STREAM_END : rc == Z_OK) && z.avail_in == 0 && z.avail_out > 0;
  out->resize(out->size() - z.avail_out);
  deflateEnd(&z);
  return ok ? 0 : 1;
}

}  // namespace

int GzipParallelWriter::fail(std::string* err, const std::string& why) {
  abort();
  if (err) *err = why;
  return 1;
}

void GzipParallelWriter::stop_workers() {
  {
    std::lock_guard<std::mutex> lk(mu_);
    quit_ = true;
    cv_.notify_all();
  }
  for (std::thread& t : th_) t.join();
  th_.clear();
}

void GzipParallelWriter::abort() {
  stop_workers();
  if (f_) { fclose(f_); f_ = nullptr; remove(tmp_.c_str()); }
  slots_.clear(); work_.clear(); cur_.clear();
}

void GzipParallelWriter::worker_main() {
  std::unique_lock<std::mutex> lk(mu_);
  for (;;) {
    cv_.wait(lk, [this] { return quit_ || !work_.empty(); });
    if (work_.empty()) return;                 // quit, and nothing left to deflate
    Slot& s = slots_[work_.front() % slots_.size()];
    work_.pop_front();
    s.state = kBusy;
    lk.unlock();
    const int rc = deflate_chunk(s.in, s.last, &s.out);      // (a busy slot is this thread's alone)
    lk.lock();
    s.rc = rc; s.state = kDone;
    cv_.notify_all();
  }
}

int GzipParallelWriter::open(const char* filename, int workers, size_t chunk_bytes, std::string* err) {
  abort();
  fn_ = filename; tmp_ = fn_ + ".tmp";
  if (workers < 1 || chunk_bytes < 1 || chunk_bytes > ((size_t)1 << 30)) return fail(err, fn_ + ": bad worker count or chunk size");
  chunk_ = chunk_bytes;
  total_in_ = total_out_ = 0; seq_ = written_ = 0; quit_ = false;
  f_ = fopen(tmp_.c_str(), "wb");
  if (!f_) return fail(err, "cannot open " + tmp_ + " for writing: " + strerror(errno));
  if (fwrite(kGzipHeader, 1, sizeof kGzipHeader, f_) != sizeof kGzipHeader) { const std::string why = strerror(errno); return fail(err, "short write to " + tmp_ + ": " + why); }
  total_out_ = sizeof kGzipHeader;
  slots_.assign((size_t)workers, Slot{});
  cur_.reserve(chunk_);
  for (int i = 0; i < workers; ++i) th_.emplace_back([this] { worker_main(); });
  return 0;
}

int GzipParallelWriter::write_next(std::string* err) {
  std::vector<uint8_t> out;
  {
    std::unique_lock<std::mutex> lk(mu_);
    Slot& s = slots_[written_ % slots_.size()];
    cv_.wait(lk, [&s] { return s.state == kDone; });
    if (s.rc) { lk.unlock(); return fail(err, fn_ + ": deflate failed"); }
    out.swap(s.out);
    s.state = kFree;
  }
  written_ += 1;
  if (fwrite(out.data(), 1, out.size(), f_) != out.size()) { const std::string why = strerror(errno); return fail(err, "short write to " + tmp_ + ": " + why); }
  total_out_ += out.size();
  return 0;
}

int GzipParallelWriter::submit(bool last, std::string* err) {
  // the slot of chunk seq_ is free once chunk seq_ - workers has been written
  while (seq_ - written_ >= slots_.size())
    if (write_next(err)) return 1;
  {
    std::lock_guard<std::mutex> lk(mu_);
    Slot& s = slots_[seq_ % slots_.size()];
    s.in.swap(cur_); s.last = last; s.rc = 0; s.state = kReady;
    work_.push_back(seq_);
    cv_.notify_all();
  }
  seq_ += 1;
  cur_.clear();
  cur_.reserve(chunk_);
  return 0;
}

int GzipParallelWriter::append(const void* data, size_t bytes, std::string* err) {
  if (!f_) { if (err) *err = fn_ + ": append without an open file"; return 1; }
  const uint8_t* p = (const uint8_t*)data;
  while (bytes) {
    // a full chunk waits for the next byte: only then is it known not to be the last
    if (cur_.size() == chunk_ && submit(false, err)) return 1;
    const size_t k = std::min(bytes, chunk_ - cur_.size());
    cur_.insert(cur_.end(), p, p + k);
    p += k; bytes -= k; total_in_ += k;
  }
  return 0;
}

int GzipParallelWriter::finish(uint32_t crc, std::string* err) {
  if (!f_) { if (err) *err = fn_ + ": finish without an open file"; return 1; }
  if (submit(true, err)) return 1;
  while (written_ < seq_)
    if (write_next(err)) return 1;
  stop_workers();
  uint8_t trailer[8];
  const uint32_t isize = (uint32_t)(total_in_ & 0xffffffffull);
  for (int i = 0; i < 4; ++i) { trailer[i] = (uint8_t)(crc >> (8 * i)); trailer[4 + i] = (uint8_t)(isize >> (8 * i)); }
  int bad = 0;                                      // errno of the first call that failed
  if (fwrite(trailer, 1, sizeof trailer, f_) != sizeof trailer) bad = errno ? errno : EIO;
  total_out_ += sizeof trailer;
  if (fflush(f_) != 0 && !bad) bad = errno;
  if (fsync(fileno(f_)) != 0 && !bad) bad = errno;  // (the rename below must not overtake the data on its way to the disk)
  if (fclose(f_) != 0 && !bad) bad = errno;
  f_ = nullptr;
  slots_.clear();
  if (bad) { remove(tmp_.c_str()); if (err) *err = "short write to " + tmp_ + ": " + strerror(bad); return 1; }
  if (rename(tmp_.c_str(), fn_.c_str()) != 0) { const std::string why = strerror(errno); remove(tmp_.c_str()); if (err) *err = "rename " + tmp_ + " -> " + fn_ + " failed: " + why; return 1; }
  return 0;
}

}  // namespace dqnhip_state
