"""Build + dlopen of the test / tuning harness (tests/csrc/dqnhip_internal.h): tests/csrc/libdqnhip_test.so, kernel-level
tests and probes, and tests/csrc/libdqnhip_test_h.so, the door to the fp16 launchers as libdqnhip.so compiles them
(hgemm_forms.hip).  Tests and scripts only — nothing under dqn-hfo_amd/ knows they exist."""
import ctypes as C
import fcntl
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
TEST_LIB = os.path.join(CSRC, "libdqnhip_test.so")
TEST_LIB_H = os.path.join(CSRC, "libdqnhip_test_h.so")
_lib = None
_lib_h = None


def build_test(verbose=False):
    """`make` (both libraries) under an exclusive file lock (several test processes may arrive at once), always consulted: a
    stale prebuilt library is never tested silently."""
    with open(os.path.join(CSRC, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            r = subprocess.run(["make", "-C", CSRC], capture_output=True, text=True)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    if verbose or r.returncode:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode:
        raise RuntimeError("hipcc build of libdqnhip_test.so / libdqnhip_test_h.so failed")
    return TEST_LIB


def load_test():
    global _lib
    if _lib is None:
        build_test()
        _lib = C.CDLL(TEST_LIB)
    return _lib


def load_test_h():
    """libdqnhip_test_h.so: dqnhip_test_hgemm_form.  A library of its own (RTLD_LOCAL, as CDLL loads): its hgemm_nt<...> are the
    product's bodies, libdqnhip_test.so's carry the test-build epilogues."""
    global _lib_h
    if _lib_h is None:
        build_test()
        _lib_h = C.CDLL(TEST_LIB_H)
    return _lib_h
