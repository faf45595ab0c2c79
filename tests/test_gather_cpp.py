"""Gather, slice, broadcast and concatenation at the class level (include/certfhe/Batch.h, UInt.h) through
tests/cpp/gather_driver.cpp: user-style C++ against the drop-in headers.  The driver builds everywhere; its flows run
on an MI355X (`pytest -m gpu`)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "gather_driver.cpp")
DRIVER = os.path.join(ROOT, "tests", "cpp", "gather_driver")
LIBDIR = os.path.join(ROOT, "csgn_amd", "lib")


@pytest.fixture(scope="module")
def driver():
    from csgn_amd import build
    build.build_all()
    deps = [DRIVER_SRC, os.path.join(LIBDIR, "libcertFHE.so")] + [
        os.path.join(ROOT, "include", "certfhe", f) for f in ("UInt.h", "Gates.h", "Batch.h")]
    if (not os.path.exists(DRIVER)
            or os.path.getmtime(DRIVER) < max(os.path.getmtime(d) for d in deps)):
        subprocess.check_call(
            ["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include", "certfhe"),
             "-I" + os.path.join(ROOT, "include"), "-o", DRIVER, DRIVER_SRC,
             "-L" + LIBDIR, "-lcertFHE", "-lcsgn_hip", "-lpthread", "-Wl,-rpath," + LIBDIR])
    return DRIVER


def run(driver, mode):
    p = subprocess.run([driver, mode], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, f"{mode}: rc={p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-2000:]}"
    assert f"{mode} ok" in p.stdout
    return p


def test_gather_driver_builds(driver):
    assert os.path.exists(driver)


@pytest.mark.gpu
def test_gather_slice_broadcast_concat_words(driver):
    run(driver, "move")


@pytest.mark.gpu
def test_encrypted_query_broadcast(driver):
    run(driver, "query")


@pytest.mark.gpu
def test_gather_bad_arguments_throw(driver):
    run(driver, "throws")
