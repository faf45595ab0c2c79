"""The multi-GPU path at world sizes 2 to 8, on a CPU: csgn_amd/csrc/certfhe_shard/ShardedBatch.cpp (one host thread,
one communicator and one block pool per rank) on the real communicator code, csgn_amd/csrc/csgn_shard_comm.cpp (enter /
leave / abort, the grace, the bounded barrier, both forms of the gather), which RCCL's refusal of two ranks on one
device keeps at world 1 on a one-GPU machine.  Underneath: tests/cpp/fake_hip_rccl.cpp, an in-process fake of the HIP
and RCCL calls the communicator code makes, with deferred completion; tests/cpp/capi_stub.cpp and capi_stub_shard.cpp,
the host stub of the C ABI; oracle/csgn_oracle.c.  tests/cpp/sharded_host_driver.cpp asserts the oracle's words, bits,
counts and digests by global element index.  Built three ways: plain, with -fsanitize=address,undefined, and with
-fsanitize=thread -- a stand-alone program: nothing is preloaded, nothing loaded into Python is sanitized; a sanitized
parameter is skipped only where a one-line probe shows its runtime does not link.  Every mode runs in every build.

What this cannot show: the stream order of the real kernels, RCCL's transports, xGMI -- tests/cpp/sharded_driver.cpp on
a node with several GPUs stays the test of those.

Time limits.  A call that fails at world W may sit out the communicator's abort grace (kAbortGraceMs, read from the
source) once per peer communicator.  The limit of one such call is that plus the time `compare W` took in the same build
(the plain run of everything the failing call does, many times over); the driver ends itself with status 4 when a call
passes it, and the process's own limit is that per failing call the mode makes, plus the same plain run."""
import os
import re
import subprocess
import time

import pytest

from tests.cpp_driver import ROOT, run

CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "csgn_amd", "csrc")
CLASSES = os.path.join(CSRC, "certfhe")
UNITS = ["runtime.cpp", "Ciphertext.cpp", "SecretKey.cpp", "Context.cpp", "Permutation.cpp", "Helpers.cpp", "Plaintext.cpp"]
SHARDED = os.path.join(CSRC, "certfhe_shard", "ShardedBatch.cpp")
COMM = os.path.join(CSRC, "csgn_shard_comm.cpp")
ORACLE = os.path.join(ROOT, "oracle", "csgn_oracle.c")
STUBS = ["sharded_host_driver.cpp", "capi_stub.cpp", "capi_stub_shard.cpp", "fake_hip_rccl.cpp"]
BUILDS = {"plain": [],
          "address": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
          "thread": ["-fsanitize=thread"]}
WORLDS = [1, 2, 3, 4, 8]
FAIL_WORLDS = [2, 3, 4]


def rocm_include():
    """The directory that holds hip/hip_runtime_api.h and rccl/rccl.h: headers only, no library of theirs is linked."""
    from csgn_amd import build as native
    return os.path.join(os.path.dirname(os.path.dirname(native._hipcc())), "include")


def grace_ms():
    with open(COMM) as f:
        return int(re.search(r"constexpr int kAbortGraceMs = (\d+);", f.read()).group(1))


def compile_driver(out, flags=(), units=None):
    """The driver, the two stub files, the fake, ShardedBatch.cpp, csgn_shard_comm.cpp, the seven base class sources
    (`units`: paths that replace the sources of the same name) and the oracle into `out`; the completed process of the
    step that failed, or of the link."""
    units = {os.path.basename(u): u for u in (units or [])}
    sources = [os.path.join(CPP, s) for s in STUBS]
    sources += [units.get(os.path.basename(s), s) for s in [SHARDED, COMM] + [os.path.join(CLASSES, u) for u in UNITS]]
    oracle = subprocess.run(["gcc", "-O1", "-g"] + list(flags) + ["-c", ORACLE, "-o", out + ".oracle.o"],
                            capture_output=True, text=True)
    if oracle.returncode != 0:
        return oracle
    cmd = (["g++", "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__"] + list(flags)
           + ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "certfhe"), "-I" + CLASSES, "-I" + CSRC,
              "-I" + CPP, "-I" + os.path.join(ROOT, "oracle"), "-isystem", rocm_include(), "-o", out]
           + sources + [out + ".oracle.o", "-lpthread", "-ldl"])
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module", params=list(BUILDS))
def driver(request, tmp_path_factory):
    flags = BUILDS[request.param]
    out = str(tmp_path_factory.mktemp("sharded_host") / ("sharded_host_driver_" + request.param))
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


def clean(p, mode):
    assert f"{mode} ok" in p.stdout, p.stdout[-3000:]
    assert "Sanitizer" not in p.stdout + p.stderr and "runtime error" not in p.stderr, (p.stdout + p.stderr)[-3000:]


_plain = {}


def plain_seconds(driver, world):
    """How long `compare world` takes in this build: the yardstick of the failing modes' limits.  Measured once a build
    and world; the run is checked like any other."""
    if (driver, world) not in _plain:
        t0 = time.monotonic()
        clean(run(driver, "compare", world, timeout=900), "compare")
        _plain[driver, world] = time.monotonic() - t0
    return _plain[driver, world]


@pytest.mark.parametrize("world", WORLDS)
def test_compare(driver, world):
    plain_seconds(driver, world)


def failing(driver, mode, world, calls, *more):
    """`mode` at `world`, which makes `calls` calls that are expected to fail."""
    plain = plain_seconds(driver, world)
    limit_ms = grace_ms() * (world - 1) + int(plain * 1000)
    clean(run(driver, mode, world, limit_ms, *more, timeout=calls * limit_ms / 1000 + plain), mode)


@pytest.mark.parametrize("world", FAIL_WORLDS)
def test_fail(driver, world):
    failing(driver, "fail", world, 4 * world)                    # each rank, two collectives, and the call after each


@pytest.mark.parametrize("world", FAIL_WORLDS)
def test_fail_mid(driver, world):
    failing(driver, "fail_mid", world, 3)


@pytest.mark.parametrize("world", FAIL_WORLDS)
def test_stuck(driver, world):
    failing(driver, "stuck", world, 4 * world + 1, grace_ms())


@pytest.mark.parametrize("mode", ["pool", "lifetime"])
def test_mode(driver, mode):
    clean(run(driver, mode, timeout=120 + plain_seconds(driver, 4)), mode)


def test_usage(driver):
    """An unknown mode, a world size out of range or a failing mode without its limit is refused, so a mistyped command
    cannot pass as a run."""
    for args in (["nothing"], ["compare"], ["compare", "9"], ["fail", "2"], ["stuck", "2", "5000"]):
        p = subprocess.run([driver] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and " ok" not in p.stdout, args


def test_stubs_define_what_the_sharded_layer_calls():
    """Twin of test_runtime_host_cpu.test_stub_defines_what_the_class_layer_calls: capi_stub.cpp and capi_stub_shard.cpp
    together define exactly the csgn_* entry points of include/csgn_hip.h, and csgn_shard_product_counts, that the seven
    base sources and ShardedBatch.cpp call.  One more call fails the link of every build above; a spare stub entry fails
    here.  (The other csgn_shard_* and csgn_comm_* calls are the real ones, of csgn_shard_comm.cpp.)"""
    def body(name):
        with open(os.path.join(CPP, name)) as f:
            text = f.read()
        return text[text.index('extern "C" {'):]
    definition = r"^(?:int|size_t|uint64_t|const char \*)\s*\*?(csgn_[a-z0-9_]+)\("
    base = set(re.findall(definition, body("capi_stub.cpp"), re.M))
    extra = set(re.findall(definition, body("capi_stub_shard.cpp"), re.M))
    with open(COMM) as f:
        real = set(re.findall(definition.replace("(?:", "(?:void \\*|"), f.read(), re.M))
    called = set()
    for path in [os.path.join(CLASSES, u) for u in UNITS] + [SHARDED]:
        with open(path) as f:
            called |= set(re.findall(r"\b(csgn_[a-z0-9_]+)\(", f.read()))
    assert not base & extra and not (base | extra) & real
    assert base | extra == called - real, (sorted((base | extra) - called), sorted(called - real - base - extra))
    assert len(base) == 30 and len(extra) == 11
