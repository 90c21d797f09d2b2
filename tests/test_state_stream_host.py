"""The host-compilable parts of the asynchronous learner-state save (dqnhip_save_state_async), without a GPU: tests/cpp/state_stream_host.cpp
is a stand-alone program that runs the chunk-CRC and combine bodies of dqn-hfo_amd/csrc/state_image.h (the code k_state_crc runs per
thread and the writer thread runs per section) against zlib's crc32 / crc32_combine — lengths 0 ... 1 MB + 13 around the chunk size,
all-zero / all-0xFF / random contents, start offsets 0 ... 3 — and the streaming writer of state_codec.cpp against write_file, byte
for byte (zero-length sections, odd-length RTRM / USER, the 64-section limit), and checks that a failed append leaves no file and no
.tmp.  It is built and run twice: plain, and with the address + undefined-behaviour sanitizers linked in (nothing preloaded).  The
files it leaves are then read back by tests/state_ref.py, the independent reader of the layout."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dqn-hfo_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _pattern(n, salt):
    return bytes((salt * 7 + j * 13 + (j >> 8)) & 0xFF for j in range(n))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_crc_bodies_and_streaming_writer(tmp_path, sanitize):
    exe = os.path.join(ROOT, "tests", "cpp", "state_stream_host" + ("_san" if sanitize else ""))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    cmd = [HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I" + CSRC] + flags + [
        "-o", exe, os.path.join(ROOT, "tests", "cpp", "state_stream_host.cpp"), os.path.join(CSRC, "state_codec.cpp"), "-lz"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "state stream host OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    # the streamed files through the independent reader
    whole, stream = (tmp_path / "whole.bin").read_bytes(), (tmp_path / "stream.bin").read_bytes()
    assert whole == stream
    info, sections = state_ref.read_bytes(stream)
    assert info["memory_size"] == 95 and info["hidden"][:2] == (64, 128) and info["update_counter"] == (1 << 40) + 7
    assert list(sections) == ["WGT0", "DEVS", "HOST", "RSTA", "RTRM", "PERL", "USER"]
    assert sections["WGT0"] == _pattern(4004, 1) and sections["HOST"] == b"" and sections["RSTA"] == _pattern(95 * 58 * 4, 3)
    assert sections["RTRM"] == _pattern(95, 4) and sections["PERL"] == b"" and sections["USER"] == _pattern(4097, 5)
    assert info["user_bytes"] == 4097 and info["file_bytes"] == len(stream)
    info, sections = state_ref.read_bytes((tmp_path / "many.bin").read_bytes())
    assert len(sections) == 64
    for i, (name, data) in enumerate(sections.items()):
        assert name == "SC%02d" % i and data == _pattern((i * 37) % 300, i)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp") or f.startswith("fail") or f.startswith("toomany")]
