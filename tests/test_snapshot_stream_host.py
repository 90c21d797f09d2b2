"""The host-compilable parts of the asynchronous Caffe snapshot (dqnhip_snapshot_async), without a GPU: tests/cpp/snapshot_stream_host.cpp
is a stand-alone program that runs the pack body of dqn-hfo_amd/csrc/snapshot_stream.h (the code k_snap_pack_replay runs per output
dword) against the memcpy loop of the synchronous dqnhip_snapshot_replay_memory — S in {58, 59, 77, 1, 64}, n in {0 ... 5, 255, 256,
257, cap - 1, cap}, heads that make the window wrap, the bytes behind the stream untouched — and the parallel gzip writer of
gzip_parallel.cpp against gzread: 1 / 2 / 8 workers, stream lengths 0, 1, chunk - 1, chunk, chunk + 1 and several chunks plus an odd
tail, the trailer's CRC and length, a wrong CRC (gzread must fail), a missing directory.  It is built and run three times: plain, with
the address + undefined-behaviour sanitizers, and with the thread sanitizer linked in (nothing preloaded, nothing loaded into
Python; where the thread sanitizer's runtime refuses the kernel's randomised address-space layout before main() runs, that one
process is started again with the randomisation off).  The members it leaves are then decompressed by Python's gzip, which verifies CRC and ISIZE on its own."""
import gzip
import os
import platform
import shutil
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dqn-hfo_amd", "csrc")

TSAN_CANNOT_START = "FATAL: ThreadSanitizer: unexpected memory mapping"
SANITIZERS = {
    "plain": [],
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"],
    "tsan": ["-fsanitize=thread", "-fno-omit-frame-pointer", "-g"],
}


@pytest.mark.parametrize("mode", list(SANITIZERS))
def test_pack_body_and_parallel_gzip_writer(tmp_path, mode):
    exe = os.path.join(ROOT, "tests", "cpp", "snapshot_stream_host" + ("" if mode == "plain" else "_" + mode))
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I" + CSRC] + SANITIZERS[mode] + [
        "-o", exe, os.path.join(ROOT, "tests", "cpp", "snapshot_stream_host.cpp"), os.path.join(CSRC, "gzip_parallel.cpp"), "-lz"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    if mode == "tsan" and r.returncode != 0 and TSAN_CANNOT_START in r.stderr and not r.stdout and shutil.which("setarch"):
        # the sanitizer's runtime refuses some kernels' randomised address-space layouts before main() runs: once more with the
        # randomisation off for this one process (the personality flag `setarch -R` sets; nothing of the host changes).  Whatever
        # that run gives is asserted on below: a thread sanitizer that cannot start fails this test
        r = subprocess.run(["setarch", platform.machine(), "-R", exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "snapshot stream host OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
    payload = (tmp_path / "payload.bin").read_bytes()
    sizes = {}
    for workers in (1, 8):
        member = (tmp_path / ("member_w%d.gz" % workers)).read_bytes()
        assert gzip.decompress(member) == payload
        sizes[workers] = len(member)
    assert sizes[1] == sizes[8]                      # the bytes do not depend on how many threads deflated them
    print("member", sizes[1], "bytes; one deflate stream at the same level", len(gzip.compress(payload, compresslevel=6)), "bytes")
    assert zlib.crc32(payload) == int.from_bytes(member[-8:-4], "little")
    left = sorted(f for f in os.listdir(tmp_path) if f not in ("payload.bin", "member_w1.gz", "member_w8.gz"))
    assert left == []
