"""-debug_info_iter through the adaptor (include/dqn.hpp + dqn_dropin.cpp, tests/cpp/diag_smoke.cpp): with `-debug_info_iter 7
-loss_display_iter 7` the episode loop's 40 updates log floor(40 / 7) diagnostic blocks, every line starting "[Agent0] [Diag]", each
block with one summary line, one [Update] line per parameter blob, one [Forward] line per activation panel, one [Q] and one [Action]
line, all numbers finite; the two lines of src/dqn.cpp:806-818 keep their format and their values; without the flag the log and the
digest are those of a run that never collected.  The same with -deferred_updates."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_dropin", "diag_smoke")
ARGS = ["-seed", "7", "-memory", "5000", "-memory_threshold", "50", "-loss_display_iter", "7", "-minibatch", "32", "-snapshot_freq", "100000"]
L = 4                                                      # diag_smoke's tower: 128 x 4
NUM = r"-?(?:\d+\.?\d*(?:e[+-]?\d+)?|\.\d+)"


def _build(pkg):
    lib = pkg.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "shim"),
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "diag_smoke.cpp"), os.path.join(ROOT, "dqn-hfo_amd", "csrc", "dqn_dropin.cpp"),
           lib, "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def _agent_lines(stderr):
    return [l[l.index("[Agent"):] for l in stderr.splitlines() if "[Agent" in l and "Seeding" not in l]


def _run(exe, extra, tmp_path):
    r = subprocess.run([exe] + ARGS + ["-prefix", str(tmp_path / "agent0")] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (extra, r.returncode, r.stdout, r.stderr)
    assert "diag smoke OK" in r.stdout and "digest: actor_iter 40 critic_iter 40 memory_size 120" in r.stdout, r.stdout
    return r


def _check_reference_lines(lines):
    assert len(lines) == 2 * (40 // 7), lines
    for i, l in enumerate(lines):
        it = 7 * (i // 2 + 1)
        want = r"\[Agent0\] Critic Iteration %d, loss = \S+$" % it if i % 2 == 0 else r"\[Agent0\] Actor Iteration %d, avg_q_value = \S+$" % it
        assert re.match(want, l), (i, l)
        assert all(c in "0123456789.e+-" for c in l.split("= ")[1]), l      # a finite number


def _check_blocks(diag):
    per_block = 1 + (4 * L + 6) + 5 * L + 2
    assert len(diag) == (40 // 7) * per_block, len(diag)
    for k in range(40 // 7):
        blk = diag[k * per_block:(k + 1) * per_block]
        assert re.match(r"\[Agent0\] \[Diag\] iter %d: grad_norm actor = %s \(clip x%s\), critic = %s \(clip x%s\), non-finite w/g = 0$"
                        % (7 * (k + 1), NUM, NUM, NUM, NUM), blk[0]), blk[0]
        upd = [l for l in blk if l.startswith("[Agent0] [Diag] [Update] ")]
        fwd = [l for l in blk if l.startswith("[Agent0] [Diag] [Forward] ")]
        assert len(upd) == 4 * L + 6 and len(fwd) == 5 * L
        assert upd == blk[1:1 + len(upd)] and fwd == blk[1 + len(upd):1 + len(upd) + len(fwd)]
        for l in upd:
            assert re.search(r"(actor|critic) \w+_layer (weight|bias): \|w\| = %s, \|g\| = %s, \|step\| = %s, \|lag\| = %s$" % (NUM, NUM, NUM, NUM), l), l
        assert [l.split("[Update] ")[1].split(":")[0] for l in upd[:2 * L + 4:2]] == \
            ["actor ip%d_layer weight" % i for i in range(1, L + 1)] + ["actor action_layer weight", "actor actionpara_layer weight"]
        assert upd[-1].split("[Update] ")[1].startswith("critic q_values_layer bias:")
        for l in fwd:
            assert re.search(r" ip[1-4]_layer: \|a\| = %s, leaky = %s, dead = \d+ / 128$" % (NUM, NUM), l), l
        assert blk[-2].startswith("[Agent0] [Diag] [Q] q_target [") and blk[-2].endswith("non-finite = 0"), blk[-2]
        assert re.match(r"\[Agent0\] \[Diag\] \[Action\] mean actor_out = (%s ){9}%s, out of bounds = \d+ / 320, \|dq_da\| = %s \(max %s\)$"
                        % (NUM, NUM, NUM, NUM), blk[-1]), blk[-1]
        for l in blk:
            assert "nan" not in l.lower() and "inf" not in l.lower(), l


@pytest.mark.gpu
@pytest.mark.parametrize("deferred", [False, True])
def test_flag_logs_blocks_and_leaves_everything_else_alone(pkg, gpu, tmp_path, deferred):
    exe = _build(pkg)
    extra = ["-deferred_updates=true"] if deferred else []
    off = _run(exe, extra, tmp_path)
    on = _run(exe, extra + ["-debug_info_iter", "7"], tmp_path)
    lines_off, lines_on = _agent_lines(off.stderr), _agent_lines(on.stderr)
    assert not any("[Diag]" in l for l in lines_off)
    _check_reference_lines(lines_off)
    diag = [l for l in lines_on if l.startswith("[Agent0] [Diag]")]
    _check_blocks(diag)
    # the reference's two lines: same format, same values; the learner computed the same thing
    assert [l for l in lines_on if "[Diag]" not in l] == lines_off
    assert on.stdout == off.stdout
    # each block follows the lines of its own iteration
    first = lines_on.index(diag[0])
    assert "Actor Iteration 7," in lines_on[first - 1] and "Critic Iteration 7," in lines_on[first - 2]
    # the flag at 0 is the flag absent
    zero = _run(exe, extra + ["-debug_info_iter", "0"], tmp_path)
    assert _agent_lines(zero.stderr) == lines_off and zero.stdout == off.stdout
