#!/usr/bin/env python3
"""Count, per kernel of a gfx950 assembly listing, the scalar wait stages a wave goes through before its first vector load.

usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o learner.s dqn-hfo_amd/csrc/learner.hip
       scripts/first_load_chain.py learner.s [name-filter ...]

A "stage" is an `s_waitcnt` that covers lgkmcnt while at least one `s_load_*` issued since the previous such wait is
outstanding: scalar loads return out of order, so each of these is one full round trip to the scalar cache (or, after a kernel
boundary, to wherever the kernarg line lives).
Column `stages`: the listing read in text order up to the first global / buffer / flat load.  In a kernel whose rider blocks
branch away first (gemm_wgrad_tail, gemm_dgrad_narrow_qrider, k_dqda_head_bwd) that load is a rider's.  Column `gemm`: the
same count along the basic-block paths from the entry to their first vector load, fewest..most, over the paths that go on to an
MFMA (riders have none) — the GEMM workgroups' paths; `-` for a kernel without MFMA.
Column `preload`: the kernel descriptor's `.amdhsa_user_sgpr_kernarg_preload_length` (dwords of kernarg the hardware delivers in
SGPRs at wave launch; 0: none).  Column `entry path`: along the MFMA path with the fewest scalar waits — the one a tile of
problem 0 takes — from the REAL entry to the first vector load, `instructions / s_waitcnt lgkmcnt with a scalar load outstanding`.
The real entry of a kernel with preloaded arguments lies behind the compatibility prologue the compiler emits in front of it
(the same words by `s_load`, a wait and a branch, for firmware that does not preload); the other columns count from the
kernel symbol, i.e. through that prologue.
Both are heuristics that rest on the compiler's present code layout: the end of the prologue is taken to be the first `s_branch`
of the listing (the prologue's jump to the real entry), and "the path of a tile of problem 0" to be the MFMA path with the fewest
waits.  Read the listing itself before relying on a row whose kernel has changed shape.
"""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def stages(lines):
    n_stage, pending, loads, instr = 0, 0, 0, 0
    for ln in lines:
        t = ln.strip()
        if not t or t.startswith((";", ".")) or t.endswith(":"):
            continue
        op = t.split()[0]
        if op.startswith(("global_load", "buffer_load", "flat_load")):
            return n_stage, loads, instr
        instr += 1
        if op.startswith(("s_load_", "s_buffer_load_")):
            pending += 1
            loads += 1
        elif op == "s_waitcnt" and "lgkmcnt" in t and pending:
            n_stage += 1
            pending = 0
    return n_stage, loads, instr


def blocks_of(lines):
    """basic blocks {label: instructions}, their order, and successor labels"""
    blocks = [("entry", [])]
    for ln in lines:
        t = ln.split(";")[0].strip()
        if not t:
            continue
        if t.endswith(":"):
            blocks.append((t[:-1], []))
            continue
        if t.startswith("."):
            continue
        blocks[-1][1].append(t)
        if t.split()[0].startswith(("s_cbranch", "s_branch", "s_endpgm")):
            blocks.append(("%s+%d" % (blocks[-1][0], len(blocks)), []))
    succ = {}
    for i, (lab, ins) in enumerate(blocks):
        last = ins[-1].split() if ins else [""]
        out = [last[1]] if last[0].startswith(("s_cbranch", "s_branch")) else []
        if last[0] not in ("s_branch", "s_endpgm") and i + 1 < len(blocks):
            out.append(blocks[i + 1][0])
        succ[lab] = out
    return dict(blocks), succ


def gemm_path_stages(lines):
    """(fewest, most) stages up to the first vector load over the block paths that later reach an MFMA; None without MFMA"""
    blocks, succ = blocks_of(lines)
    reach = {b for b, ins in blocks.items() if any(t.startswith("v_mfma") for t in ins)}
    if not reach:
        return None
    grew = True
    while grew:                                   # blocks from which an MFMA block is reachable
        grew = False
        for b, out in succ.items():
            if b not in reach and any(o in reach for o in out):
                reach.add(b); grew = True
    memo, stack = {}, set()

    def walk(lab, pending):
        """stage counts from the top of `lab` (with scalar loads outstanding or not) to a first vector load on an MFMA path"""
        key = (lab, pending)
        if key in memo:
            return memo[key]
        if lab not in blocks or lab not in reach or key in stack:
            return set()
        stack.add(key)
        n, res = 0, None
        for t in blocks[lab]:
            op = t.split()[0]
            if op.startswith(("global_load", "buffer_load", "flat_load")):
                res = {n}
                break
            if op.startswith(("s_load_", "s_buffer_load_")):
                pending = True
            elif op == "s_waitcnt" and "lgkmcnt" in t and pending:
                n, pending = n + 1, False
        if res is None:
            res = {n + m for nx in succ[lab] for m in walk(nx, pending)}
        stack.discard(key)
        memo[key] = res
        return res

    found = walk("entry", False)
    return (min(found), max(found)) if found else None


def real_entry(lines, preload):
    """the listing behind the compatibility prologue of a kernel with preloaded arguments (up to its first s_branch)"""
    if not preload:
        return lines
    for i, ln in enumerate(lines):
        if ln.split(";")[0].strip().startswith("s_branch"):
            return lines[i + 1:]
    return lines


def entry_path(lines):
    """(scalar waits, instructions) to the first vector load along the MFMA path (no MFMA: any path) with the fewest waits"""
    blocks, succ = blocks_of(lines)
    reach = {b for b, ins in blocks.items() if any(t.startswith("v_mfma") for t in ins)}
    if not reach:
        reach = set(blocks)                       # a kernel without MFMA (the head forward): every path counts
    grew = True
    while grew:
        grew = False
        for b, out in succ.items():
            if b not in reach and any(o in reach for o in out):
                reach.add(b); grew = True
    memo, stack = {}, set()

    def walk(lab, pending):
        key = (lab, pending)
        if key in memo:
            return memo[key]
        if lab not in blocks or lab not in reach or key in stack:
            return None
        stack.add(key)
        waits, instr, res = 0, 0, None
        for t in blocks[lab]:
            op = t.split()[0]
            if op.startswith(("global_load", "buffer_load", "flat_load")):
                res = (waits, instr)
                break
            instr += 1
            if op.startswith(("s_load_", "s_buffer_load_")):
                pending = True
            elif op == "s_waitcnt" and "lgkmcnt" in t and pending:
                waits, pending = waits + 1, False
        if res is None:
            tails = [w for w in (walk(nx, pending) for nx in succ[lab]) if w is not None]
            res = (waits + min(tails)[0], instr + min(tails)[1]) if tails else None
        stack.discard(key)
        memo[key] = res
        return res

    first = next(iter(blocks))
    return walk(first, False)


def listing(path):
    """{demangled kernel name: (stages, gemm path stages or None, s_loads, instructions, preload length, entry path or None)};
    entry path = (scalar waits, instructions)"""
    kernels, cur, body = {}, None, []
    kd, preload, in_kd = set(), {}, None
    text = open(path).read().split("\n")
    for ln in text:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            kd.add(m.group(1)); in_kd = m.group(1)
        m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", ln)
        if m and in_kd:
            preload[in_kd] = int(m.group(1))
    for ln in text:
        m = re.match(r"^(\w+):", ln)
        if m and m.group(1) in kd:
            cur, body = m.group(1), []
            kernels[cur] = body
        elif cur is not None:
            if re.match(r"\s*\.section|\s*\.amdhsa_kernel", ln):
                cur = None
            else:
                body.append(ln)
    names = demangle(sorted(kernels))
    out = {}
    for k in kernels:
        st, ld, ins = stages(kernels[k])
        pl = preload.get(k, 0)
        out[names[k]] = (st, gemm_path_stages(kernels[k]), ld, ins, pl, entry_path(real_entry(kernels[k], pl)))
    return out


def main():
    path, filters = sys.argv[1], sys.argv[2:]
    print("%-7s %-6s %-8s %-6s %-8s %-11s kernel" % ("stages", "gemm", "s_loads", "instr", "preload", "entry path"))
    for nm, (st, g, ld, ins, pl, ep) in sorted(listing(path).items()):
        if filters and not any(f in nm for f in filters):
            continue
        print("%-7d %-6s %-8d %-6d %-8d %-11s %s" % (st, "-" if g is None else "%d..%d" % g, ld, ins, pl,
                                                     "-" if ep is None else "%d / %d" % (ep[1], ep[0]), nm[:150]))


if __name__ == "__main__":
    main()
