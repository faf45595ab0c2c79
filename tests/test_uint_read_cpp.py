"""Encrypted tables read at encrypted indices at the class level (include/certfhe/UInt.h, readAt) through
tests/cpp/uint_read_driver.cpp: user-style C++ against the drop-in headers.  The driver builds everywhere; its flows run
on an MI355X (`pytest -m gpu`)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "uint_read_driver.cpp")
DRIVER = os.path.join(ROOT, "tests", "cpp", "uint_read_driver")
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


def test_uint_read_driver_builds(driver):
    assert os.path.exists(driver)


@pytest.mark.gpu
def test_uint_read_words_and_decryptions(driver):
    run(driver, "words")


@pytest.mark.gpu
def test_uint_read_ragged_planes_same_words(driver):
    run(driver, "ragged")


@pytest.mark.gpu
def test_uint_read_oversize_throws_first(driver):
    run(driver, "oversize")
