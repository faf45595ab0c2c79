"""The per-thread temporary blocks of the composed forms (csgn_amd/csrc/csgn_scratch.cpp: scratch_take, scratch_done) on
a CPU.  tests/cpp/scratch_stub.cpp is compiled with g++ TOGETHER WITH that file and defines the only HIP calls it makes
(hipMalloc, hipFree, hipStreamIsCapturing), so nothing of the HIP runtime is linked: the stubs record every live pointer,
count calls and can fail or report a capturing stream.  Built twice: plain, and with -fsanitize=address,undefined (a
stand-alone program: nothing is preloaded, nothing loaded into Python is sanitized); the sanitized parameter is skipped
where the sanitizer runtime does not link."""
import os
import subprocess

import pytest

from tests.cpp_driver import ROOT, run_mode

SRC = os.path.join(ROOT, "tests", "cpp", "scratch_stub.cpp")
UNIT = os.path.join(ROOT, "csgn_amd", "csrc", "csgn_scratch.cpp")
MODES = ["reuse", "grow", "evict", "owned", "capture", "pinned", "exit"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def compile_stub(out, unit=UNIT, flags=()):
    """g++ of the stub with `unit` (csgn_scratch.cpp, or a copy of it) into `out`; the completed process."""
    from csgn_amd import build as native
    rocm = os.path.dirname(os.path.dirname(native._hipcc()))
    csrc = os.path.join(ROOT, "csgn_amd", "csrc")
    deps = [SRC, unit, os.path.join(csrc, "csgn_kernels.h"), os.path.join(csrc, "csgn_common.h")]
    if os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(d) for d in deps):
        return None
    cmd = (["g++", "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
            "-I" + csrc, "-I" + os.path.join(ROOT, "include")] + list(flags) + ["-o", out, SRC, unit, "-lpthread"])
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def stub(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("scratch_stub") / ("scratch_stub_" + request.param))
    if request.param == "sanitized":
        probe = out + "_probe"
        with open(probe + ".cpp", "w") as f:
            f.write("int main() { return 0; }\n")
        linked = subprocess.run(["g++"] + SANITIZE + ["-o", probe, probe + ".cpp"], capture_output=True, text=True)
        if linked.returncode != 0:
            pytest.skip("the sanitizer runtime does not link here: " + linked.stderr[-300:])
    p = compile_stub(out, flags=SANITIZE if request.param == "sanitized" else ())
    assert p is None or p.returncode == 0, p.stderr[-4000:]
    return out


@pytest.mark.parametrize("mode", MODES)
def test_scratch_mode(stub, mode):
    run_mode(stub, mode, timeout=120)


def test_scratch_usage(stub):
    """An unknown mode is refused, so a mistyped mode cannot pass as a run."""
    p = subprocess.run([stub, "nothing"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and " ok" not in p.stdout
