"""Build and run the C++ programs the tests drive against the drop-in (include/certfhe + libcertFHE.so): the drivers
under tests/cpp, oracle/ref_driver.cpp as a shared library, and tools/shard_mul.cpp.  One compile line for all of
them; a program is rebuilt when its source, tests/cpp/driver.h, a public header or a library it links is newer."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "csgn_amd", "lib")
INCLUDE = os.path.join(ROOT, "include")
HEADERS = ([os.path.join(ROOT, "tests", "cpp", "driver.h")] + glob.glob(os.path.join(INCLUDE, "*.h"))
           + glob.glob(os.path.join(INCLUDE, "certfhe", "*.h")))
DROPIN = ("certFHE", "csgn_hip")
SHARDED = ("certFHE_shard", "certFHE", "csgn_shard", "csgn_hip")


def build(src, out=None, libs=DROPIN, opt="-O1", shared=False):
    """Compile `src` (relative to the repository root) into `out` (default: `src` without its extension), linked
    against `libs` in csgn_amd/lib; the native libraries are built first.  A program that links libcsgn_shard.so
    (RCCL) also gets an rpath to the ROCm libraries of the toolchain csgn_amd/build.py compiles with."""
    from csgn_amd import build as native
    native.build_all()
    src = os.path.join(ROOT, src)
    out = os.path.join(ROOT, out) if out else os.path.splitext(src)[0]
    lib_files = [os.path.join(LIBDIR, "lib%s.so" % name) for name in libs]
    deps = [src] + HEADERS + lib_files
    if os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(d) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    rpaths = [LIBDIR]
    if "csgn_shard" in libs:
        rpaths.append(os.path.join(os.path.dirname(os.path.dirname(native._hipcc())), "lib"))
    cmd = (["g++", "-std=c++11", opt] + (["-fPIC", "-shared"] if shared else ["-Wall"])
           + ["-I" + os.path.join(INCLUDE, "certfhe"), "-I" + INCLUDE, "-o", out, src, "-L" + LIBDIR]
           + ["-l" + name for name in libs] + ["-lpthread"] + ["-Wl,-rpath," + p for p in rpaths])
    subprocess.check_call(cmd)
    return out


def fixture(src, **kw):
    """A module-scoped fixture that builds `src` and gives the program's path."""
    return pytest.fixture(scope="module")(lambda: build(src, **kw))


def run(program, *args, timeout=600, check=True):
    """Run `program` with `args`; with `check`, it must exit 0 (the tails of its output name the failure)."""
    p = subprocess.run([program, *map(str, args)], capture_output=True, text=True, timeout=timeout)
    if check:
        assert p.returncode == 0, f"{args}: rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-2000:]}"
    return p


def run_mode(driver, mode, timeout=900):
    """One mode of an operation driver (tests/cpp/driver.h's runModes): exit 0 and its "<mode> ok" line."""
    p = run(driver, mode, timeout=timeout)
    assert f"{mode} ok" in p.stdout, p.stdout[-3000:]
    return p
