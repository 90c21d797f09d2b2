"""An independent reader / writer of the native learner-state file, written from the byte layout in DESIGN.md 9 with `struct` and
`zlib.crc32` alone (no line of the library's codec is involved): the host tests write files with it and hand them to
dqnhip_state_info / dqnhip_state_read_user, the GPU tests read the files dqnhip_save_state wrote with it.

Layout (little endian, no padding anywhere):
  header, 144 bytes   magic "DQNHIPST" | u32 version (1) | u32 header_bytes (144) | i32 flags, precision, minibatch, state_size,
                      num_hidden, hidden[8], replay_capacity, memory_size, actor_iter, critic_iter, has_memory, has_per,
                      has_loss_scale | u32 n_sections | u32 reserved (0) | u64 seed, update_counter, user_bytes, file_bytes |
                      u32 CRC-32 of the table | u32 CRC-32 of the header's first 140 bytes
  table               n_sections entries of 24 bytes: 4-character tag | u32 CRC-32 of the section | u64 offset | u64 bytes
  sections            back to back in table order, the first one right behind the table; file_bytes = the end of the last one
"""
import struct
import zlib

import numpy as np

MAGIC = b"DQNHIPST"
VERSION = 1
HEADER = struct.Struct("<8sII" + "i" * 5 + "8i" + "i" * 7 + "II" + "QQQQ")     # ... + the two CRCs = 144 bytes
HEADER_BYTES = HEADER.size + 8
ENTRY = struct.Struct("<4sIQQ")
INFO_FIELDS = ("flags", "precision", "minibatch", "state_size", "num_hidden", "hidden", "replay_capacity", "memory_size", "actor_iter",
               "critic_iter", "has_memory", "has_per", "has_loss_scale", "seed", "update_counter")
# fixed-size sections
DEVS = struct.Struct("<iiQffii")        # actor_iter, critic_iter, update_counter, critic_loss, avg_q, flags, skipped_steps
LSCL = struct.Struct("<ff2i2i2i")       # mult[actor, critic], good[2], backoffs[2], growths[2]
HOST = struct.Struct("<QQ")             # sample_states_calls, seed
RING = struct.Struct("<ii")             # ring_head, ring_size
PERC = struct.Struct("<ffifQfiq")       # alpha, beta0, beta_anneal_iters, eps, seed, p_max, reserved, syncs
assert (HEADER_BYTES, ENTRY.size, DEVS.size, LSCL.size, HOST.size, RING.size, PERC.size) == (144, 24, 32, 32, 16, 8, 40)


class StateFileError(ValueError):
    pass


def crc(b):
    return zlib.crc32(bytes(b)) & 0xFFFFFFFF


def write_bytes(info, sections, table_override=None, file_bytes=None):
    """info: a dict with INFO_FIELDS (hidden: a sequence of up to 8); sections: [(tag: 4 bytes, payload: bytes)].
    table_override(i, tag, crc, offset, nbytes) -> the entry's values, for files that are wrong on purpose."""
    n = len(sections)
    off = HEADER_BYTES + n * ENTRY.size
    table, user_bytes = b"", 0
    for i, (tag, payload) in enumerate(sections):
        ent = (tag, crc(payload), off, len(payload))
        if table_override is not None:
            ent = table_override(i, *ent)
        table += ENTRY.pack(*ent)
        off += len(payload)
        if tag == b"USER":
            user_bytes = len(payload)
    hidden = list(info["hidden"]) + [0] * (8 - len(info["hidden"]))
    head = HEADER.pack(MAGIC, info.get("version", VERSION), HEADER_BYTES, info["flags"], info["precision"], info["minibatch"], info["state_size"],
                       info["num_hidden"], *hidden, info["replay_capacity"], info["memory_size"], info["actor_iter"], info["critic_iter"],
                       info["has_memory"], info["has_per"], info["has_loss_scale"], n, 0, info["seed"], info["update_counter"], user_bytes,
                       off if file_bytes is None else file_bytes)
    head += struct.pack("<I", crc(table))
    head += struct.pack("<I", crc(head))
    return head + table + b"".join(p for _, p in sections)


def layout(data):
    """[(name, first byte, end)] of the header, the table and every section of a well-formed file: where a test cuts and flips."""
    n = struct.unpack_from("<I", data, 96)[0]
    out = [("header", 0, HEADER_BYTES), ("table", HEADER_BYTES, HEADER_BYTES + n * ENTRY.size)]
    for i in range(n):
        tag, _, off, nb = ENTRY.unpack_from(data, HEADER_BYTES + i * ENTRY.size)
        out.append((tag.decode(), off, off + nb))
    return out


def read_bytes(data):
    """-> (info dict, {tag: payload bytes}); raises StateFileError naming the defect, checks in the library's order."""
    if len(data) < 8 or data[:8] != MAGIC:
        raise StateFileError("bad magic")
    if len(data) < 12:
        raise StateFileError("truncated inside the header")
    if struct.unpack_from("<I", data, 8)[0] != VERSION:
        raise StateFileError("unknown format version")
    if len(data) < HEADER_BYTES:
        raise StateFileError("truncated inside the header")
    f = HEADER.unpack_from(data, 0)
    table_crc, header_crc = struct.unpack_from("<II", data, HEADER.size)
    if crc(data[:HEADER_BYTES - 4]) != header_crc:
        raise StateFileError("header CRC mismatch")
    info = {"version": f[1], "flags": f[3], "precision": f[4], "minibatch": f[5], "state_size": f[6], "num_hidden": f[7], "hidden": tuple(f[8:16]),
            "replay_capacity": f[16], "memory_size": f[17], "actor_iter": f[18], "critic_iter": f[19], "has_memory": f[20], "has_per": f[21],
            "has_loss_scale": f[22], "seed": f[25], "update_counter": f[26], "user_bytes": f[27], "file_bytes": f[28]}
    n = f[23]
    if f[2] != HEADER_BYTES or n > 64:
        raise StateFileError("bad header")
    end = HEADER_BYTES + n * ENTRY.size
    if len(data) < end:
        raise StateFileError("truncated inside the section table")
    if crc(data[HEADER_BYTES:end]) != table_crc:
        raise StateFileError("section table CRC mismatch")
    entries = [ENTRY.unpack_from(data, HEADER_BYTES + i * ENTRY.size) for i in range(n)]
    for tag, _, off, nb in entries:
        if off + nb > info["file_bytes"]:
            raise StateFileError("section %s runs past the end of the file" % tag.decode())
        if off != end:
            raise StateFileError("section %s does not follow its predecessor" % tag.decode())
        end += nb
    if end != info["file_bytes"]:
        raise StateFileError("bad header (file_bytes)")
    if len(data) != info["file_bytes"]:
        raise StateFileError("truncated" if len(data) < info["file_bytes"] else "trailing bytes")
    sections = {}
    for tag, c, off, nb in entries:
        if crc(data[off:off + nb]) != c:
            raise StateFileError("section %s CRC mismatch" % tag.decode())
        sections[tag.decode()] = data[off:off + nb]
    return info, sections


def read(path):
    with open(path, "rb") as f:
        return read_bytes(f.read())


def decode(info, sections):
    """The sections as numpy arrays / dicts, by the meaning DESIGN.md 9 gives them."""
    S, n = info["state_size"], info["memory_size"]
    f32 = lambda tag: np.frombuffer(sections[tag], "<f4").copy()
    out = {"w": [f32("WGT%d" % k) for k in range(4)], "m": [f32("ADM%d" % k) for k in range(2)], "v": [f32("ADV%d" % k) for k in range(2)]}
    out["dev"] = dict(zip(("actor_iter", "critic_iter", "update_counter", "critic_loss", "avg_q", "flags", "skipped_steps"), DEVS.unpack(sections["DEVS"])))
    out["host"] = dict(zip(("sample_states_calls", "seed"), HOST.unpack(sections["HOST"])))
    if "LSCL" in sections:
        v = LSCL.unpack(sections["LSCL"])
        out["loss_scale"] = {"mult": v[0:2], "good": v[2:4], "backoffs": v[4:6], "growths": v[6:8]}
    if info["has_memory"]:
        out["ring"] = dict(zip(("ring_head", "ring_size"), RING.unpack(sections["RING"])))
        out["states"], out["next_states"] = f32("RSTA").reshape(n, S), f32("RNXT").reshape(n, S)
        out["actor_out"], out["rewards"], out["mc"] = f32("RACT").reshape(n, 10), f32("RREW"), f32("RMCT")
        out["terminal"] = np.frombuffer(sections["RTRM"], np.uint8).copy()
    if info["has_per"]:
        out["per"] = dict(zip(("alpha", "beta0", "beta_anneal_iters", "eps", "seed", "p_max", "reserved", "syncs"), PERC.unpack(sections["PERC"])))
        out["leaves"] = f32("PERL")
    out["user"] = sections.get("USER", b"")
    return out
