"""The host code of the drop-in classes (csgn_amd/csrc/certfhe: runtime.cpp, Ciphertext.cpp, SecretKey.cpp -- the block
cache, the pinned pool, the staging buffers, the result slot, the deferred small-operation queue) on a CPU.
tests/cpp/capi_stub.cpp defines the 30 entry points of the C ABI that the seven base sources of the class layer call, and
no others, so the link itself fails when the class layer starts calling something the stub does not know; neither
libcsgn_hip nor the HIP runtime is linked.  The stub keeps every "device" and pinned block as a host allocation of
exactly the bytes asked for, checks every pointer a call is handed against the live blocks, logs the calls and can be
told to refuse them; tests/cpp/runtime_host_driver.cpp asserts words from its own evaluation and call sequences from the
log.  Built three ways: plain, with -fsanitize=address,undefined, and with -fsanitize=thread -- stand-alone programs:
nothing is preloaded, nothing loaded into Python is sanitized.  Every mode runs in every build (none had to be left out
of a sanitizer); a sanitized parameter is skipped only where a one-line probe shows its runtime does not link.  The stub
is synchronous and cannot show ordering on a stream: the GPU modes of tests/test_dropin_cpp.py stay the test of that."""
import os
import subprocess

import pytest

from tests.cpp_driver import ROOT, run_mode

CPP = os.path.join(ROOT, "tests", "cpp")
CLASSES = os.path.join(ROOT, "csgn_amd", "csrc", "certfhe")
UNITS = ["runtime.cpp", "Ciphertext.cpp", "SecretKey.cpp", "Context.cpp", "Permutation.cpp", "Helpers.cpp", "Plaintext.cpp"]
ORACLE = os.path.join(ROOT, "oracle", "csgn_oracle.c")
MODES = ["words", "batch", "ring", "fail_flush", "exit", "threads", "cache", "pinned", "staged"]
BUILDS = {"plain": [],
          "address": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
          "thread": ["-fsanitize=thread"]}


def compile_driver(out, flags=(), units=None):
    """The driver, the stub, the seven class sources (`units`: paths that replace those of the same name) and the oracle
    into `out`; the completed process of the step that failed, or of the link."""
    units = {os.path.basename(u): u for u in (units or [])}
    sources = [os.path.join(CPP, "runtime_host_driver.cpp"), os.path.join(CPP, "capi_stub.cpp")]
    sources += [units.get(u, os.path.join(CLASSES, u)) for u in UNITS]
    oracle = subprocess.run(["gcc", "-O1", "-g"] + list(flags) + ["-c", ORACLE, "-o", out + ".oracle.o"],
                            capture_output=True, text=True)
    if oracle.returncode != 0:
        return oracle
    cmd = (["g++", "-std=c++17", "-O1", "-g", "-Wall"] + list(flags)
           + ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "certfhe"), "-I" + CLASSES,
              "-I" + CPP, "-I" + os.path.join(ROOT, "oracle"), "-o", out] + sources + [out + ".oracle.o", "-lpthread"])
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module", params=list(BUILDS))
def driver(request, tmp_path_factory):
    flags = BUILDS[request.param]
    out = str(tmp_path_factory.mktemp("runtime_host") / ("runtime_host_driver_" + request.param))
    if flags:
        probe = out + "_probe"
        with open(probe + ".cpp", "w") as f:
            f.write("int main() { return 0; }\n")
        linked = subprocess.run(["g++"] + flags + ["-o", probe, probe + ".cpp"], capture_output=True, text=True)
        if linked.returncode != 0:
            pytest.skip("the sanitizer runtime does not link here: " + linked.stderr[-300:])
    p = compile_driver(out, flags)
    assert p.returncode == 0, p.stderr[-4000:]
    return out


@pytest.mark.parametrize("mode", MODES)
def test_runtime_host_mode(driver, mode):
    p = run_mode(driver, mode, timeout=120)
    assert "Sanitizer" not in p.stdout + p.stderr and "runtime error" not in p.stderr, (p.stdout + p.stderr)[-3000:]


def test_runtime_host_usage(driver):
    """An unknown mode is refused, so a mistyped mode cannot pass as a run."""
    p = subprocess.run([driver, "nothing"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and " ok" not in p.stdout


def test_stub_defines_what_the_class_layer_calls():
    """The stub's entry points are exactly the csgn_* symbols the seven sources leave undefined: one more in the class
    layer fails the link of every build above, one more in the stub fails here."""
    import re
    with open(os.path.join(CPP, "capi_stub.cpp")) as f:
        text = f.read()
    body = text[text.index('extern "C" {'):]
    defined = set(re.findall(r"^(?:int|size_t|uint64_t|const char \*)\s*\*?(csgn_[a-z0-9_]+)\(", body, re.M))
    called = set()
    for unit in UNITS:
        with open(os.path.join(CLASSES, unit)) as f:
            called |= set(re.findall(r"\b(csgn_[a-z0-9_]+)\(", f.read()))
    assert defined == called and len(defined) == 30, (sorted(defined - called), sorted(called - defined))
