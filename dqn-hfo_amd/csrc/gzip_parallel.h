// gzip_parallel.h — one gzip member written by several compressor threads (the `.replaymemory` file of dqnhip_snapshot_async;
// DESIGN.md 9 has the construction).  The member is the 10-byte header gzopen("wb") writes, the payload cut into chunks that are
// deflated independently as raw deflate at gzopen's level — every chunk but the last ends with Z_SYNC_FLUSH, which leaves the bit
// stream on a byte boundary, the last with Z_FINISH — and the trailer: the CRC-32 of the uncompressed bytes, which the caller
// supplies (the snapshot computes it on the device), and their count mod 2^32.  gzread / gzip.decompress read it as any other member
// and verify both trailer fields.
// The caller's thread appends and writes the compressed chunks, in order; `workers` threads deflate.  Memory in flight is bounded:
// `workers` slots of one chunk in and one chunk out, plus the chunk being filled.  The file is written as filename + ".tmp",
// fsynced and renamed by finish(); a failure, and a writer dropped before finish(), removes the ".tmp" and leaves filename alone.
// Host code only, no HIP; not installed, not part of the C-ABI.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace dqnhip_state {

class GzipParallelWriter {
 public:
  static constexpr size_t kDefaultChunk = (size_t)1 << 20;
  GzipParallelWriter() = default;
  GzipParallelWriter(const GzipParallelWriter&) = delete;
  GzipParallelWriter& operator=(const GzipParallelWriter&) = delete;
  ~GzipParallelWriter() { abort(); }
  // workers >= 1, chunk_bytes >= 1.  open / append / finish return 0 or set *err.
  int open(const char* filename, int workers, size_t chunk_bytes, std::string* err);
  int append(const void* data, size_t bytes, std::string* err);
  int finish(uint32_t crc32_of_payload, std::string* err);
  void abort();
  uint64_t payload_bytes() const { return total_in_; }
  uint64_t file_bytes() const { return total_out_; }      // after finish()

 private:
  enum SlotState { kFree, kReady, kBusy, kDone };
  struct Slot { std::vector<uint8_t> in, out; bool last = false; int rc = 0; SlotState state = kFree; };
  int submit(bool last, std::string* err);                // the chunk being filled -> the slot of its sequence number
  int write_next(std::string* err);                       // waits for the oldest chunk in flight and writes it
  int fail(std::string* err, const std::string& why);
  void stop_workers();
  void worker_main();

  std::string fn_, tmp_;
  FILE* f_ = nullptr;
  size_t chunk_ = kDefaultChunk;
  std::vector<uint8_t> cur_;
  uint64_t total_in_ = 0, total_out_ = 0;
  uint64_t seq_ = 0, written_ = 0;                        // chunks submitted / written
  std::vector<Slot> slots_;                               // chunk k lives in slot k % workers
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<uint64_t> work_;                             // sequence numbers ready for a worker
  bool quit_ = false;
};

}  // namespace dqnhip_state
