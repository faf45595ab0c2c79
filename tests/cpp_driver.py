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


def run(program, *args, timeout=600, check=True, env=None):
    """Run `program` with `args`, the mapping `env` added to its environment; with `check`, it must exit 0 (the tails
    of its output name the failure).  A value of None removes that variable."""
    child = None
    if env:                                              # a value of None takes the variable out of the child's environment
        child = {k: v for k, v in os.environ.items() if env.get(k, "") is not None}
        child.update({k: str(v) for k, v in env.items() if v is not None})
    p = subprocess.run([program, *map(str, args)], capture_output=True, text=True, timeout=timeout, env=child)
    if check:
        assert p.returncode == 0, f"{args} {env or ''}: rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-2000:]}"
    return p


def run_mode(driver, mode, timeout=900, env=None):
    """One mode of an operation driver (tests/cpp/driver.h's runModes): exit 0 and its "<mode> ok" line."""
    p = run(driver, mode, timeout=timeout, env=env)
    assert f"{mode} ok" in p.stdout, p.stdout[-3000:]
    return p


# The class-level drivers in every form.  Each uniform-batch operation has a fused kernel and a composed (pitched)
# form picked by one knob of csgn_amd/csrc/csgn_tuning.h; the library reads CSGN_<KNOB IN CAPITALS> once when it loads,
# so a forced form is one child process.  The drivers are the only tests whose payloads come from the classes' block
# cache (hipMalloc / hipFree around the operators, recycled dirty blocks), which is where a composed form gave wrong
# words that no torch process showed.
FORM_KNOBS = {"gates": "gate_fused", "uint": "uint_fused", "uint_plain": "uint_plain_fused",
              "uint_lut": "uint_lut_fused", "uint_read": "uint_read_fused", "uint_addk": "uint_addk_fused"}
NO_BLOCK_CACHE = {"CSGN_NO_BLOCK_CACHE": "1"}        # BlockCache::give frees every payload at once


def form_env(name, value):
    """The environment that forces driver `name`'s own knob to `value` (0 composed / pitched, 1 fused)."""
    return {"CSGN_" + FORM_KNOBS[name].upper(): str(value)}


FORMS = [pytest.param(0, id="composed"), pytest.param(1, id="fused")]
FUSED_KERNEL = {"gates": "k_gate_fused", "uint": "k_uint_step", "uint_plain": "k_uint_plain", "uint_lut": "k_uint_lut",
                "uint_read": "k_uint_read", "uint_addk": "k_uint_addk"}


def form_lines(driver, name, value):
    """The `forms` mode of a driver, its knob forced to `value` or (None) taken out of the environment: the
    (shape, form the library names) of every line."""
    env = {"CSGN_" + FORM_KNOBS[name].upper(): None if value is None else str(value)}
    p = run_mode(driver, "forms", env=env)
    rows = [line.split(" -> ") for line in p.stdout.splitlines() if " -> " in line]
    assert rows, p.stdout[-2000:]
    return [(shape.strip(), form.strip()) for shape, form in rows]


def check_forced_forms(driver, name, value, always_fused=(), always_composed=()):
    """A forced form must be shown to have run: with the knob at 0 no shape of `forms` names the fused kernel, with it at
    1 every shape does -- except the shapes the headers document as taking one form whatever the knob says, which the
    caller lists by name (predicates over the shape text) and which must then take exactly that form."""
    rows = form_lines(driver, name, value)
    seen = {"fused": 0, "composed": 0}
    for shape, got in rows:
        if any(f(shape) for f in always_fused):
            want_fused = True
        elif any(f(shape) for f in always_composed):
            want_fused = False
        else:
            want_fused = value == 1
        assert (got == FUSED_KERNEL[name]) == want_fused, (shape, got, value)
        seen["fused" if want_fused else "composed"] += 1
    assert seen["fused" if value == 1 else "composed"] > len(rows) // 2, seen     # the exceptions are the few
    return rows
