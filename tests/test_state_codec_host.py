"""The learner-state file's container without a GPU: dqnhip_state_info / dqnhip_state_read_user (csrc/state_codec.cpp) on files
written by tests/state_ref.py, an independent writer of the layout in DESIGN.md 9 — every header field comes back, the user
section comes back, and a damaged file is refused with a message that names the defect."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_ref  # noqa: E402

INFO = {"flags": 0, "precision": 1, "minibatch": 128, "state_size": 58, "num_hidden": 3, "hidden": (128, 64, 192), "replay_capacity": 4096,
        "memory_size": 5, "actor_iter": 12, "critic_iter": 13, "has_memory": 1, "has_per": 1, "has_loss_scale": 1,
        "seed": 0xFEDCBA9876543210, "update_counter": (1 << 40) + 7}
USER = bytes(range(256)) * 3 + b"tail"


def _sections(user=USER):
    rng = np.random.default_rng(5)
    blob = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    sec = [(("WGT%d" % k).encode(), blob(4 * (100 + k))) for k in range(4)]
    sec += [(b"ADM0", blob(400)), (b"ADV0", blob(400)), (b"ADM1", blob(404)), (b"ADV1", blob(404))]
    sec += [(b"DEVS", state_ref.DEVS.pack(12, 13, (1 << 40) + 7, 0.5, -1.25, 0, 2)), (b"LSCL", state_ref.LSCL.pack(0.5, 0.25, 1, 2, 3, 4, 5, 6)),
            (b"HOST", state_ref.HOST.pack(3, INFO["seed"])), (b"RING", state_ref.RING.pack(4094, 5)),
            (b"RSTA", blob(5 * 58 * 4)), (b"RNXT", blob(5 * 58 * 4)), (b"RACT", blob(5 * 40)), (b"RREW", blob(20)), (b"RMCT", blob(20)),
            (b"RTRM", blob(5)), (b"PERC", state_ref.PERC.pack(0.6, 0.4, 20, 1e-6, 99, 1.5, 0, 4)), (b"PERL", blob(20))]
    if user:
        sec.append((b"USER", user))
    return sec


def _write(tmp_path, data, name="f.learnerstate"):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def _refused(pkg, path, *words):
    for call in (pkg.state_info, pkg.state_user):
        with pytest.raises(pkg.DQNFatal) as e:
            call(path)
        msg = str(e.value)
        assert os.path.basename(path) in msg, msg
        assert any(w in msg for w in words), (words, msg)
    return msg


def test_info_reports_every_field_and_the_user_section_comes_back(pkg, tmp_path):
    data = state_ref.write_bytes(INFO, _sections())
    assert state_ref.read_bytes(data)[1]["USER"] == USER
    path = _write(tmp_path, data)
    info = pkg.state_info(path)
    for k in state_ref.INFO_FIELDS:
        assert info[k] == INFO[k], (k, info[k], INFO[k])
    assert info["version"] == 1 and info["user_bytes"] == len(USER) and info["file_bytes"] == len(data) == os.path.getsize(path)
    assert pkg.state_user(path) == USER
    # no user section: an empty blob, not an error
    path = _write(tmp_path, state_ref.write_bytes(INFO, _sections(user=b"")), "nouser")
    assert pkg.state_info(path)["user_bytes"] == 0 and pkg.state_user(path) == b""
    # a buffer smaller than the section is refused with both sizes
    import ctypes as C
    lib, n, buf = pkg.capi.load(), C.c_size_t(), C.create_string_buffer(16)
    assert lib.dqnhip_state_read_user(os.fsencode(_write(tmp_path, data)), buf, 16, C.byref(n)) != 0
    assert n.value == len(USER) and str(len(USER)) in lib.dqnhip_last_error().decode()
    # ABI check of the struct
    s = pkg.capi.StateInfo()
    assert lib.dqnhip_state_info(os.fsencode(path), C.byref(s)) != 0 and "struct_size" in lib.dqnhip_last_error().decode()


def test_wrong_magic_and_unknown_version(pkg, tmp_path):
    data = state_ref.write_bytes(INFO, _sections())
    _refused(pkg, _write(tmp_path, b"DQNHIPSX" + data[8:]), "bad magic")
    _refused(pkg, _write(tmp_path, b""), "bad magic")
    _refused(pkg, _write(tmp_path, state_ref.write_bytes(dict(INFO, version=2), _sections())), "unknown format version 2")
    with pytest.raises(pkg.DQNFatal, match="cannot open"):
        pkg.state_info(str(tmp_path / "missing"))


def test_cut_at_every_section_boundary_and_in_mid_section(pkg, tmp_path):
    data = state_ref.write_bytes(INFO, _sections())
    for name, first, end in state_ref.layout(data):
        for cut in sorted({first, (first + end) // 2}):
            if cut == len(data):
                continue
            msg = _refused(pkg, _write(tmp_path, data[:cut]), "truncated", "bad magic")
            assert ("bad magic" in msg) == (cut < 8), (name, cut, msg)
            with pytest.raises(state_ref.StateFileError):
                state_ref.read_bytes(data[:cut])
    _refused(pkg, _write(tmp_path, data + b"\0"), "trailing bytes")


def test_a_section_running_past_the_end(pkg, tmp_path):
    sec = _sections()
    last = len(sec) - 1
    # the table is consistent (its CRC holds, the header's too) but its last entry claims 8 bytes more than the file has
    data = state_ref.write_bytes(INFO, sec, table_override=lambda i, tag, c, off, nb: (tag, c, off, nb + (8 if i == last else 0)))
    _refused(pkg, _write(tmp_path, data), "section USER runs past the end of the file")
    mid = 3
    data = state_ref.write_bytes(INFO, sec, table_override=lambda i, tag, c, off, nb: (tag, c, off + (1 << 40 if i == mid else 0), nb))
    _refused(pkg, _write(tmp_path, data), "section WGT3 runs past the end of the file")
    # ... and one that overlaps its predecessor
    data = state_ref.write_bytes(INFO, sec, table_override=lambda i, tag, c, off, nb: (tag, c, off - (4 if i == mid else 0), nb))
    _refused(pkg, _write(tmp_path, data), "section WGT3 does not follow its predecessor")


def test_one_flipped_byte_anywhere(pkg, tmp_path):
    data = state_ref.write_bytes(INFO, _sections())
    for name, first, end in state_ref.layout(data):
        # the header's first 12 bytes are magic and version, which have messages of their own (above)
        for pos in sorted({max(first, 12), (first + end) // 2, end - 1}):
            bad = bytearray(data)
            bad[pos] ^= 0x10
            want = {"header": "header CRC mismatch", "table": "section table CRC mismatch"}.get(name, "section %s CRC mismatch" % name)
            _refused(pkg, _write(tmp_path, bytes(bad)), want)
            with pytest.raises(state_ref.StateFileError):
                state_ref.read_bytes(bytes(bad))
