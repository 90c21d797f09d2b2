"""Which kernels each translation unit of libdqnhip.so embeds, without a GPU: a unit includes the headers of the kernels it launches
and no others (the map: dqn-hfo_amd/csrc/learner_args.hip.h), so the kernels in an object's gfx950 code object are exactly the
kernels the object has a host launch stub for, and the host-only units carry no device code at all.  An include that drags a kernel
group into a unit that does not launch it (every unit used to carry most of the update's kernels: 159 embedded for 80 launched)
fails here."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dqn-hfo_amd", "csrc")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def demangled(names):
    names = sorted(names)
    return set(run("c++filt", *names).splitlines()) if names else set()


def embedded_kernels(obj, tmp):
    """the kernels (demangled) of the object's gfx950 code object; None: the object has no device code"""
    if ".hip_fatbin" not in run(os.path.join(LLVM, "llvm-readelf"), "-S", "-W", obj):
        return None
    fatbin, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
    run("objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fatbin)
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fatbin, "--output=" + co)
    syms = [line.split()[-1] for line in run(os.path.join(LLVM, "llvm-readelf"), "--dyn-syms", "-W", co).splitlines() if line.strip()]
    return demangled(s[:-len(".kd")] for s in syms if s.endswith(".kd"))


def launch_stubs(obj):
    """the kernels (demangled) the object's host code has a launch stub for"""
    syms = [line.split()[-1] for line in run("nm", obj).splitlines() if "__device_stub__" in line]
    return {d.replace("__device_stub__", "") for d in demangled(syms)}


def test_each_unit_embeds_the_kernels_it_launches(pkg, tmp_path):
    pkg.build()
    objects = sorted(glob.glob(os.path.join(CSRC, "*.o")))
    assert len(objects) >= 11, objects
    kernels = {}
    for obj in objects:
        tmp = tmp_path / os.path.basename(obj)
        tmp.mkdir()
        k = embedded_kernels(obj, str(tmp))
        if k is not None:
            kernels[os.path.basename(obj)] = k
    assert sorted(kernels) == ["learner.o", "learner_env.o", "learner_eval.o", "learner_io.o", "learner_per.o", "learner_save_async.o"]
    for name, embedded in sorted(kernels.items()):
        stubs = launch_stubs(os.path.join(CSRC, name))
        print(name, len(embedded), "kernels embedded,", len(stubs), "launch stubs")
        assert embedded, name
        assert embedded == stubs, (name, "embedded, never launched:", sorted(embedded - stubs), "launched, not embedded:", sorted(stubs - embedded))
