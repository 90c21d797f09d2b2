"""dqnhip_set_act_precision / dqnhip_get_act_precision without a GPU: the symbols, their ctypes entries, the argument checks that
need no learner, and the drop-in's -act_precision flag, which is CHECKed against -precision in the constructor before the device is
touched (driven through tests/cpp/loss_scale_smoke.cpp, as tests/test_gpu_dynamic_loss_scale_adaptor.py drives its flag).  What the
switch does on the device: tests/test_gpu_act_precision.py, tests/test_gpu_env_act_precision.py."""
import ctypes as C
import inspect
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_dropin", "act_precision_flag")


def test_symbols_are_exported_and_declared(pkg):
    lib = pkg.capi.load()
    for name, args in (("dqnhip_set_act_precision", [pkg.capi.H, C.c_int32]), ("dqnhip_get_act_precision", [pkg.capi.H, pkg.capi.ip])):
        assert name in pkg.capi.SIGNATURES
        assert pkg.capi.SIGNATURES[name] == (C.c_int, args)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args
    header = open(os.path.join(ROOT, "include", "dqnhip.h")).read()
    assert "int dqnhip_set_act_precision(dqnhip_handle h, int32_t precision);" in header
    assert "int dqnhip_get_act_precision(dqnhip_handle h, int32_t* precision);" in header
    assert (pkg.capi.FP32, pkg.capi.FP16) == (0, 1)


def test_null_arguments_are_refused_with_a_message(pkg):
    lib = pkg.capi.load()
    assert lib.dqnhip_set_act_precision(None, pkg.capi.FP16) != 0
    assert b"null handle" in lib.dqnhip_last_error()
    v = C.c_int32(7)
    assert lib.dqnhip_get_act_precision(None, C.byref(v)) != 0
    assert b"null" in lib.dqnhip_last_error() and v.value == 7


def test_python_surface(pkg):
    sig = inspect.signature(pkg.DQN.__init__)
    assert sig.parameters["act_precision"].default == "fp32"
    assert callable(pkg.DQN.set_act_precision) and isinstance(pkg.DQN.act_precision, property)


def test_dropin_flag_is_checked_against_precision(pkg, tmp_path):
    """-act_precision fp16 needs -precision fp16; both CHECKs fire in the constructor, before dqnhip_create: no device needed"""
    lib = pkg.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "shim"),
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "loss_scale_smoke.cpp"), os.path.join(ROOT, "dqn-hfo_amd", "csrc", "dqn_dropin.cpp"),
           lib, "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    base = ["-memory", "5000", "-minibatch", "128", "-prefix", str(tmp_path / "agent0")]
    for extra, what in ((["-precision", "fp32", "-act_precision", "fp16"], "-act_precision fp16 needs -precision fp16"),
                        (["-act_precision", "fp16"], "-act_precision fp16 needs -precision fp16"),          # (-precision defaults to fp32)
                        (["-precision", "fp16", "-act_precision", "half"], "-act_precision must be fp32 or fp16")):
        r = subprocess.run([EXE] + base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "loss scale smoke OK" not in r.stdout, (extra, r.returncode, r.stdout)
        assert "Check failed" in r.stderr and what in r.stderr, (extra, r.stderr)
