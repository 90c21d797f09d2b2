"""Caffe's learning-rate policies without a GPU.  tests/cpp/lr_schedule_host.cpp is a stand-alone program around the host build of
dqn-hfo_amd/csrc/lr_schedule.hip.h — lr_rate, the function the gather's scalars block evaluates on the device — for nineteen schedules
over the seven policies, iterations 0 ... 2000 (every boundary of every schedule lies inside) and a few far ones.  Each rate must be
within 1 float32 ulp of tests/sched_ref.py's, evaluated in float64 and rounded once: a double pow / exp good to a few double ulps can
land on the other side of a float32 rounding boundary and can do no more than that.  The exponents of step and multistep are exact
integers; poly beyond max_iter is 0.  The program also checks every create-time refusal's wording; it is built and run twice, plain and
with the address + undefined-behaviour sanitizers linked in (a stand-alone binary: nothing is preloaded).  The same refusals through
the C call that shares dqnhip_create's validator (dqnhip_grad_arena_bytes: no device needed), the names, the config block's place in
the struct and the old struct_size."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sched_ref as SR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dqn-hfo_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
F32 = np.float32


def _f(bits):
    return np.array([int(bits, 16)], np.uint32).view(F32)[0]


def _parse(out):
    """-> [(Schedule, (base_actor, base_critic), [(it, rate_actor, rate_critic, current_step)])]"""
    table = []
    for line in out.splitlines():
        t = line.split()
        if t and t[0] == "S":
            n = int(t[6])
            s = SR.schedule(SR.POLICIES[int(t[1])], _f(t[2]), _f(t[3]), int(t[4]), int(t[5]), [int(v) for v in t[7:7 + n]])
            assert t[7 + n] == "|"
            table.append((s, (_f(t[8 + n]), _f(t[9 + n])), []))
        elif t and t[0] == "R":
            table[-1][2].append((int(t[1]), _f(t[2]), _f(t[3]), int(t[4])))
    return table


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_build_of_lr_rate(sanitize):
    exe = os.path.join(ROOT, "tests", "cpp", "lr_schedule_host" + ("_san" if sanitize else ""))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    cmd = [HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I" + CSRC] + flags + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "lr_schedule_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lr schedule host OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    table = _parse(r.stdout)
    assert len(table) == 19 and {s.policy for s, _, _ in table} == set(SR.POLICIES)
    worst = {}
    for s, base, rows in table:
        assert len(rows) == 2007 and [r[0] for r in rows[:2001]] == list(range(2001))
        for it, ra, rc, step in rows:
            assert step == SR.current_step(s, it), (s, it, step)                      # exact integers
            for net, got in ((0, ra), (1, rc)):
                want = SR.rate(s, base[net], it)
                if not np.isfinite(want) or not np.isfinite(got):
                    assert got == want, (s, it, net, got, want)
                    continue
                d = SR.ulps32(got, want)
                assert d <= SR.RATE_ULP, (s, it, net, float(got), float(want), d)
                worst[s.policy] = max(worst.get(s.policy, 0), d)
            if s.policy == "fixed":
                assert (ra, rc) == base
            if s.policy == "poly" and it >= s.max_iter and s.power > 0:
                assert ra == 0 and rc == 0, (s, it)
            if s.policy in ("step", "multistep") and step == 0:
                assert (ra, rc) == base, (s, it)
    print("worst distance in float32 ulps per policy:", worst)


# ---- through the C call ------------------------------------------------------------------------------------------------------------------------
def _cfg(pkg, **kw):
    lib = pkg.capi.load()
    cfg = pkg.capi.Config()
    lib.dqnhip_default_config(C.byref(cfg), 59)
    cfg.num_hidden = 2
    cfg.hidden[0], cfg.hidden[1] = 64, 128
    for k, v in kw.items():
        if k == "lr_stepvalue":
            for i, x in enumerate(v):
                cfg.lr_stepvalue[i] = x
        else:
            setattr(cfg, k, v)
    return lib, cfg


def test_defaults_names_and_place_in_the_struct(pkg):
    lib, cfg = _cfg(pkg)
    assert cfg.struct_size == C.sizeof(pkg.capi.Config)
    assert (cfg.lr_policy, cfg.lr_gamma, cfg.lr_power, cfg.lr_stepsize, cfg.lr_max_iter, cfg.lr_n_stepvalue) == (0, 0.0, 0.0, 0, 0, 0)
    assert not any(cfg.lr_stepvalue) and cfg.weight_decay == 0.0 and cfg.regularization_type == 0
    assert [lib.dqnhip_lr_policy_name(i) for i in range(7)] == [p.encode() for p in SR.POLICIES] == [p.encode() for p in pkg.capi.LR_POLICIES]
    assert lib.dqnhip_lr_policy_name(-1) is None and lib.dqnhip_lr_policy_name(7) is None
    # the 24 words sit between rms_decay and tuning_flags: every field before them keeps its offset
    names = [n for n, _ in pkg.capi.Config._fields_]
    block = names[names.index("rms_decay") + 1:names.index("tuning_flags")]
    assert block == ["lr_policy", "lr_gamma", "lr_power", "lr_stepsize", "lr_max_iter", "lr_n_stepvalue", "lr_stepvalue", "weight_decay", "regularization_type"]
    assert pkg.capi.Config.tuning_flags.offset - pkg.capi.Config.lr_policy.offset == 96
    assert lib.dqnhip_grad_arena_bytes(C.byref(cfg)) > 0


def test_the_old_struct_size_is_a_fixed_learner(pkg):
    """a caller compiled before the block existed: its struct is 96 bytes shorter and its tail sits where the block is now"""
    lib, cfg = _cfg(pkg, tuning_flags=32)
    want = lib.dqnhip_grad_arena_bytes(C.byref(cfg))
    raw = bytes(cfg)
    a, b = pkg.capi.Config.lr_policy.offset, pkg.capi.Config.tuning_flags.offset
    old = bytearray(raw[:a] + raw[b:])
    old[0:4] = np.array([len(old)], np.int32).tobytes()
    buf = (C.c_char * len(old)).from_buffer(old)
    lib.dqnhip_grad_arena_bytes.argtypes = [C.c_void_p]
    try:
        assert lib.dqnhip_grad_arena_bytes(C.addressof(buf)) == want > 0, lib.dqnhip_last_error()
        # the tail is read from where the old struct has it: a bad loss_scale_mode there is seen
        bad = bytearray(old)
        off = pkg.capi.Config.loss_scale_mode.offset - 96
        bad[off:off + 4] = np.array([7], np.int32).tobytes()
        bbuf = (C.c_char * len(bad)).from_buffer(bad)
        assert lib.dqnhip_grad_arena_bytes(C.addressof(bbuf)) == 0 and b"loss_scale_mode" in lib.dqnhip_last_error()
    finally:
        lib.dqnhip_grad_arena_bytes.argtypes = [C.POINTER(pkg.capi.Config)]


@pytest.mark.parametrize("policy", list(range(1, 7)))
def test_each_policy_is_accepted(pkg, policy):
    kw = {1: dict(lr_gamma=0.5, lr_stepsize=2), 2: dict(lr_gamma=0.5), 3: dict(lr_gamma=0.0, lr_power=1.0),
          4: dict(lr_gamma=0.1, lr_n_stepvalue=2, lr_stepvalue=(3, 5)), 5: dict(lr_max_iter=8, lr_power=0.0), 6: dict(lr_gamma=-1.0, lr_stepsize=0)}[policy]
    lib, cfg = _cfg(pkg, lr_policy=policy, weight_decay=1e-2, regularization_type=1, **kw)
    assert lib.dqnhip_grad_arena_bytes(C.byref(cfg)) > 0, lib.dqnhip_last_error()


@pytest.mark.parametrize("kw,message", [
    (dict(lr_policy=7), b"Unknown learning rate policy: 7"),
    (dict(lr_policy=-2), b"Unknown learning rate policy: -2"),
    (dict(lr_policy=1, lr_gamma=0.5), b"lr_policy step: stepsize > 0"),                       # the unchanged driver's -lr_policy step and nothing else
    (dict(lr_policy=1, lr_stepsize=10), b"lr_policy step: gamma > 0"),
    (dict(lr_policy=2), b"lr_policy exp: gamma > 0"),
    (dict(lr_policy=2, lr_gamma=float("nan")), b"lr_policy exp: gamma > 0"),
    (dict(lr_policy=3, lr_gamma=-0.5), b"lr_policy inv: gamma >= 0"),
    (dict(lr_policy=4, lr_gamma=0.5), b"lr_policy multistep: 1 to 16 stepvalues"),
    (dict(lr_policy=4, lr_gamma=0.5, lr_n_stepvalue=17), b"lr_policy multistep: 1 to 16 stepvalues"),
    (dict(lr_policy=4, lr_gamma=0.5, lr_n_stepvalue=2, lr_stepvalue=(5, 5)), b"lr_policy multistep: stepvalues must be positive and strictly increasing"),
    (dict(lr_policy=4, lr_gamma=0.5, lr_n_stepvalue=2, lr_stepvalue=(0, 5)), b"lr_policy multistep: stepvalues must be positive"),
    (dict(lr_policy=4, lr_gamma=0.0, lr_n_stepvalue=1, lr_stepvalue=(5,)), b"lr_policy multistep: gamma > 0"),
    (dict(lr_policy=5, lr_power=1.0), b"lr_policy poly: max_iter > 0"),
    (dict(lr_policy=5, lr_max_iter=10, lr_power=-1.0), b"lr_policy poly: power >= 0"),
    (dict(lr_policy=6, lr_gamma=1.0, lr_stepsize=-1), b"lr_policy sigmoid: stepsize >= 0"),
    (dict(weight_decay=-1e-3), b"weight_decay >= 0"),
    (dict(weight_decay=1e-3, regularization_type=2), b"Unknown regularization type: 2"),
    (dict(lr_policy=2, lr_gamma=0.5, dp_world=2), b"lr_policy exp"),
    (dict(weight_decay=1e-3, dp_world=2), b"weight_decay 0.001"),
])
def test_refusals(pkg, kw, message):
    lib, cfg = _cfg(pkg, **kw)
    assert lib.dqnhip_grad_arena_bytes(C.byref(cfg)) == 0
    assert message in lib.dqnhip_last_error(), lib.dqnhip_last_error()
    if "dp_world" in kw:
        assert b"dp_world" in lib.dqnhip_last_error()


def test_python_constructor_refuses_unknown_names(pkg):
    with pytest.raises(pkg.DQNFatal, match="Unknown learning rate policy: bogus"):
        pkg.DQN(59, lr_policy="bogus")
    with pytest.raises(pkg.DQNFatal, match="Unknown regularization type: L3"):
        pkg.DQN(59, regularization="L3")
    with pytest.raises(pkg.DQNFatal, match="multistep"):
        pkg.DQN(59, lr_policy="multistep", lr_gamma=0.5, lr_stepvalues=tuple(range(1, 18)))
