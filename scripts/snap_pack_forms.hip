// snap_pack_forms.hip — the two forms of the asynchronous Caffe snapshot's pack kernel, each timed on its own (an event pair around
// the one launch) on a ring of the headline shape, with k_state_pack_ring (the learner-state save's pack) on the same ring in the same
// process as the yardstick.  Stand-alone: it includes the library's kernel headers and needs no learner.
//   k_snap_pack_replay_dword   one thread per aligned output dword (defined here: the form the library did not keep)
//   k_snap_pack_replay         the library's: a workgroup stages K records in LDS and streams aligned 16-byte pieces (K = 16 ... 256)
// Every form's output is compared with snap_dword() on the host, dword by dword, and the guard band behind the stream is checked,
// before any time is printed.  Prints one markdown table (median of --reps launches after a warm-up).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I dqn-hfo_amd/csrc -o snap_pack_forms scripts/snap_pack_forms.hip
//   ./snap_pack_forms [cap 1000000] [S 58] [reps 20] [head 123457]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "state_kernels.hip.h"
#include "snapshot_kernels.hip.h"

using namespace dqnhip;

// one thread per aligned output dword of the stream: snap_dword() of snapshot_stream.h; threads past the stream's last dword exit
__global__ __launch_bounds__(256) void k_snap_pack_replay_dword(Ring ring, const DevState* __restrict__ st, uint32_t* __restrict__ out, uint64_t max_dwords) {
  const int head = st->ring_head, n = min(max(st->ring_size, 0), ring.cap);
  if (head < 0 || head >= ring.cap) return;
  const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= max_dwords || d >= dqnhip_snap::stream_dwords(ring.S, (uint64_t)n)) return;
  dqnhip_snap::SnapSrc s{(const uint32_t*)ring.state, (const uint32_t*)ring.act, (const uint32_t*)ring.reward, (const uint32_t*)ring.mc, ring.term,
                         ring.S, ring.SP, ring.cap, head, n};
  out[d] = dqnhip_snap::snap_dword(s, d);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
  const int cap = argc > 1 ? atoi(argv[1]) : 1000000, S = argc > 2 ? atoi(argv[2]) : 58, reps = argc > 3 ? atoi(argv[3]) : 20;
  const int head = argc > 4 ? atoi(argv[4]) : 123457 % cap, SP = (S + 63) / 64 * 64, n = cap;
  if (cap < 1 || S < 1 || reps < 1 || head < 0 || head >= cap) { fprintf(stderr, "bad arguments\n"); return 1; }
  // the ring, filled with a cheap hash so that every byte of the stream says where it came from
  std::vector<uint32_t> hs((size_t)cap * SP), ha((size_t)cap * kAP), hr(cap), hm(cap);
  std::vector<uint8_t> ht(cap);
  uint32_t x = 0x9E3779B9u;
  auto next = [&] { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
  for (auto& v : hs) v = next();
  for (auto& v : ha) v = next();
  for (int i = 0; i < cap; ++i) { hr[i] = next(); hm[i] = next(); ht[i] = (uint8_t)(next() % 3); }      // (2: any non-zero byte is "terminal")
  Ring ring{}; ring.cap = cap; ring.S = S; ring.SP = SP;
  CK(hipMalloc(&ring.state, hs.size() * 4)); CK(hipMalloc(&ring.next, hs.size() * 4)); CK(hipMalloc(&ring.act, ha.size() * 4));
  CK(hipMalloc(&ring.reward, (size_t)cap * 4)); CK(hipMalloc(&ring.mc, (size_t)cap * 4)); CK(hipMalloc(&ring.term, cap));
  CK(hipMemcpy(ring.state, hs.data(), hs.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(ring.next, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(ring.act, ha.data(), ha.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(ring.reward, hr.data(), (size_t)cap * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(ring.mc, hm.data(), (size_t)cap * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(ring.term, ht.data(), cap, hipMemcpyHostToDevice));
  DevState hst{}; hst.ring_head = head; hst.ring_size = n;
  DevState* st; CK(hipMalloc(&st, sizeof(DevState))); CK(hipMemcpy(st, &hst, sizeof(DevState), hipMemcpyHostToDevice));

  const uint64_t max_dwords = dqnhip_snap::stream_dwords(S, (uint64_t)cap), total = dqnhip_snap::stream_dwords(S, (uint64_t)n);
  const size_t out_words = max_dwords + dqnhip_snap::kGuardWords;
  uint32_t* out_base; CK(hipMalloc(&out_base, (out_words + 3) * 4));
  uint32_t* out = out_base + 3;                                 // as the library places the stream: the first record on a 16-byte boundary
  dqnhip_snap::SnapSrc src{hs.data(), ha.data(), hr.data(), hm.data(), ht.data(), S, SP, cap, head, n};
  std::vector<uint32_t> want(total), got(out_words);
  for (uint64_t d = 0; d < total; ++d) want[d] = dqnhip_snap::snap_dword(src, d);

  hipStream_t stream; CK(hipStreamCreate(&stream));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int max_lds = 256 * dqnhip_snap::snap_lds_row_words(S) * 4;
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_snap_pack_replay), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
  auto launch_form = [&](int K) -> hipError_t {                 // K 0: the per-dword form
    if (K == 0) hipLaunchKernelGGL(k_snap_pack_replay_dword, dim3((unsigned)((max_dwords + 255) / 256)), dim3(256), 0, stream, ring, (const DevState*)st, out, max_dwords);
    else hipLaunchKernelGGL(k_snap_pack_replay, dim3((unsigned)((cap + K - 1) / K)), dim3(256),
                            (size_t)K * dqnhip_snap::snap_lds_row_words(S) * 4, stream, ring, (const DevState*)st, out, max_dwords, K);
    return hipGetLastError();
  };
  auto median_us = [&](auto&& fn, double* us) -> int {
    std::vector<float> t;
    for (int i = 0; i < reps + 3; ++i) {
      CK(hipEventRecord(e0, stream)); CK(fn()); CK(hipEventRecord(e1, stream)); CK(hipEventSynchronize(e1));
      float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
      if (i >= 3) t.push_back(ms);
    }
    std::sort(t.begin(), t.end());
    *us = 1e3 * t[t.size() / 2];
    return 0;
  };

  printf("cap = n = %d, S = %d, head = %d: the stream is %llu bytes; median of %d launches, each between its own pair of events\n\n", cap, S, head,
         (unsigned long long)dqnhip_snap::stream_bytes(S, (uint64_t)n), reps);
  printf("| kernel | µs | bytes read + written | GB/s |\n|---|---|---|---|\n");
  const int forms[] = {0, 16, 32, 64, 128, 256};
  for (int K : forms) {
    CK(hipMemsetD32Async((hipDeviceptr_t)out, (int)dqnhip_snap::kGuardWord, out_words, stream));
    CK(launch_form(K));
    CK(hipMemcpyAsync(got.data(), out, out_words * 4, hipMemcpyDeviceToHost, stream)); CK(hipStreamSynchronize(stream));
    if (memcmp(got.data(), want.data(), total * 4) != 0) {
      uint64_t d = 0; while (got[d] == want[d]) ++d;
      fprintf(stderr, "form K = %d: dword %llu is %08x, expected %08x\n", K, (unsigned long long)d, got[d], want[d]); return 1;
    }
    for (uint64_t d = total; d < out_words; ++d) if (got[d] != dqnhip_snap::kGuardWord) { fprintf(stderr, "form K = %d wrote behind the stream (dword %llu)\n", K, (unsigned long long)d); return 1; }
    double us = 0;
    if (median_us([&] { return launch_form(K); }, &us)) return 1;
    const double bytes = (double)n * ((double)SP * 4 + kAP * 4 + 9) + 4.0 * total;
    char name[96];
    if (K) snprintf(name, sizeof name, "`k_snap_pack_replay`, %d records per workgroup", K); else snprintf(name, sizeof name, "`k_snap_pack_replay_dword`, one thread per dword");
    printf("| %s | %.1f | %.0f | %.0f |\n", name, us, bytes, bytes / us * 1e-3);
  }
  {  // the yardstick: k_state_pack_ring over the six arrays of the learner-state file (state, next, act, reward, mc, term)
    const size_t row = (size_t)S * 8 + kNO * 4 + 9;
    uint8_t* dst; CK(hipMalloc(&dst, (size_t)cap * row + 6 * 16));
    RingPackArgs a{}; a.st = st; a.cap = cap; a.n_arr = 6;
    size_t off = 0; auto at = [&](size_t bytes) { uint8_t* p = dst + off; off += (bytes + 15) / 16 * 16; return p; };
    const int vecS = S % 4 == 0 && SP % 4 == 0;
    a.arr[0] = RingArr{ring.state, at((size_t)cap * S * 4), S, SP, 4, vecS}; a.arr[1] = RingArr{ring.next, at((size_t)cap * S * 4), S, SP, 4, vecS};
    a.arr[2] = RingArr{ring.act, at((size_t)cap * kNO * 4), kNO, kAP, 4, 0}; a.arr[3] = RingArr{ring.reward, at((size_t)cap * 4), 1, 1, 4, 0};
    a.arr[4] = RingArr{ring.mc, at((size_t)cap * 4), 1, 1, 4, 0}; a.arr[5] = RingArr{ring.term, at(cap), 1, 1, 1, 0};
    double us = 0;
    if (median_us([&] { hipLaunchKernelGGL(k_state_pack_ring, dim3((cap + dqnhip_state::kPackRows - 1) / dqnhip_state::kPackRows, 6), dim3(256), 0, stream, a); return hipGetLastError(); }, &us)) return 1;
    const double bytes = (double)n * ((double)SP * 8 + kAP * 4 + 9) + (double)n * row;
    printf("| `k_state_pack_ring` (yardstick), six arrays | %.1f | %.0f | %.0f |\n", us, bytes, bytes / us * 1e-3);
    CK(hipFree(dst));
  }
  printf("\nEvery form's output equals snap_dword() on the host dword for dword, and none wrote behind the stream.\n");
  return 0;
}
