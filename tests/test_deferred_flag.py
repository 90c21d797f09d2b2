"""-deferred_updates at the boundaries that need no device: the two C-ABI entry points exist (header, library, ctypes table), the
adaptor knows the flag, and the combinations it refuses are refused before the device is touched."""
import ctypes as C
import os
import subprocess

import test_abi_symbols
import test_cpp_adaptor


def test_indexed_entry_points_are_declared_exported_and_bound(pkg):
    decl = test_abi_symbols.declared_functions()
    lib = C.CDLL(pkg.build())
    for name in ("dqnhip_update_indexed_n", "dqnhip_collect_stats"):
        assert name in decl and hasattr(lib, name) and name in pkg.capi.SIGNATURES
    assert set(pkg.capi.SIGNATURES) == decl
    assert not [n for n in sorted(decl) if not hasattr(lib, n)]


def test_cpu_mode_message_with_the_flag_set(pkg):
    exe = test_cpp_adaptor._build(pkg)
    r = subprocess.run([exe, "-check", "cpu_mode", "-deferred_updates=true"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and r.returncode != 20, (r.returncode, r.stdout, r.stderr)
    assert "unknown command line flag" not in r.stderr, r.stderr
    assert "-gpu=false" in r.stderr and "not provided by the MI355X drop-in" in r.stderr, r.stderr


def test_refused_flag_combinations(pkg):
    """both checks sit in front of dqnhip_create: no device is needed to see them"""
    exe = test_cpp_adaptor._build(pkg)
    for other in ("-pipelined_stats", "-device_sampling"):
        r = subprocess.run([exe, "-deferred_updates", other], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0, (other, r.stdout, r.stderr)
        assert "-deferred_updates" in r.stderr and other in r.stderr and "cannot be combined" in r.stderr, r.stderr
