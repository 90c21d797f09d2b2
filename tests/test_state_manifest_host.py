"""The manifest of the learner-state file (dqn-hfo_amd/csrc/state_codec.h: the ordered list of a file's sections that both savers walk
and the load takes its sizes from), without a GPU: tests/cpp/state_manifest_host.cpp is a stand-alone program that holds the manifest
of every combination of the optional sections (SOLV, LRSC, LSCL, the memory, the priorities, USER of 0 / 5 bytes; ring sizes 0, 1, 95)
against a literal expectation written from DESIGN.md 9, and writes a handful of files of pattern bytes through StreamWriter, table and
payload driven by the manifest.  It is built and run twice: plain, and with the address + undefined-behaviour sanitizers linked in
(nothing preloaded).  Its files are then read by tests/state_ref.py, the independent reader of the layout: every section holds its
pattern, and decode() finds the shapes it expects."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dqn-hfo_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PARAMS = ["WGT0", "WGT1", "WGT2", "WGT3", "ADM0", "ADV0", "ADM1", "ADV1"]
MEMORY = ["RING", "RSTA", "RNXT", "RACT", "RREW", "RMCT", "RTRM"]
# the program's shapes: (state_size, memory_size, the tags in file order)
SHAPES = [
    (58, 95, PARAMS + ["DEVS", "HOST"] + MEMORY),
    (59, 95, PARAMS + ["SOLV", "LRSC", "DEVS", "LSCL", "HOST"] + MEMORY + ["PERC", "PERL", "USER"]),
    (59, 0, PARAMS + ["DEVS", "LSCL", "HOST", "USER"]),
    (58, 0, PARAMS + ["LRSC", "DEVS", "HOST"] + MEMORY + ["PERC", "PERL"]),
    (59, 1, PARAMS + ["SOLV", "DEVS", "HOST"] + MEMORY),
]
DENSE = (1001, 2003, 1001, 2003)


def _pattern(n, salt):
    return bytes((salt * 7 + j * 13 + (j >> 8)) & 0xFF for j in range(n))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_manifest_against_the_documented_order(tmp_path, sanitize):
    exe = os.path.join(ROOT, "tests", "cpp", "state_manifest_host" + ("_san" if sanitize else ""))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    cmd = [HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I" + CSRC] + flags + [
        "-o", exe, os.path.join(ROOT, "tests", "cpp", "state_manifest_host.cpp"), os.path.join(CSRC, "state_codec.cpp"), "-lz"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "state manifest host OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    for k, (S, n, tags) in enumerate(SHAPES):
        data = (tmp_path / ("shape%d.bin" % k)).read_bytes()
        info, sections = state_ref.read_bytes(data)
        assert list(sections) == tags, k
        for i, tag in enumerate(tags):
            assert sections[tag] == _pattern(len(sections[tag]), i), (k, tag)
        has_memory, has_per = "RING" in tags, "PERC" in tags
        assert (info["state_size"], info["memory_size"], info["has_memory"], info["has_per"], info["has_loss_scale"]) == (
            S, n, int(has_memory), int(has_per), int("LSCL" in tags)), k
        assert info["flags"] == (0 if has_memory else 1) and info["replay_capacity"] == 96 and info["hidden"][:3] == (64, 128, 0)
        assert (info["actor_iter"], info["critic_iter"], info["update_counter"], info["seed"]) == (3, 4, (1 << 40) + 7, 0xFEDCBA9876543210)
        assert info["user_bytes"] == (5 if "USER" in tags else 0) and info["file_bytes"] == len(data)
        out = state_ref.decode(info, sections)
        assert [len(w) for w in out["w"]] == list(DENSE) and [len(m) for m in out["m"] + out["v"]] == [1001, 2003, 1001, 2003]
        assert ("loss_scale" in out) == ("LSCL" in tags) and len(out["user"]) == info["user_bytes"]
        assert len(sections.get("SOLV", b"")) == (16 if "SOLV" in tags else 0) and len(sections.get("LRSC", b"")) == (104 if "LRSC" in tags else 0)
        if has_memory:
            assert out["states"].shape == out["next_states"].shape == (n, S) and out["actor_out"].shape == (n, 10)
            assert len(out["rewards"]) == len(out["mc"]) == len(out["terminal"]) == n
            assert len(sections["RTRM"]) == n and len(sections["RSTA"]) == n * S * 4
        else:
            assert "ring" not in out
        if has_per:
            assert len(out["leaves"]) == n and set(out["per"]) >= {"alpha", "p_max", "syncs"}
        else:
            assert "per" not in out
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
