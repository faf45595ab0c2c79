"""F2Polynomial, polyMap, ch, maj, chi, andAll and polyRoute at the class level (include/certfhe/UInt.h) through
tests/cpp/uint_poly_driver.cpp: user-style C++ against the drop-in headers.  The driver builds everywhere; its flows
run on an MI355X (`pytest -m gpu`)."""
import os

import pytest

from tests.cpp_driver import NO_BLOCK_CACHE, fixture, run_mode

driver = fixture("tests/cpp/uint_poly_driver.cpp")


def test_uint_poly_driver_builds(driver):
    assert os.path.exists(driver)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["words", "ragged", "errors"])
def test_uint_poly_driver(driver, mode):
    run_mode(driver, mode)


@pytest.mark.gpu
def test_uint_poly_driver_without_block_cache(driver):
    run_mode(driver, "words", env=NO_BLOCK_CACHE)
