"""The class-level integers (include/certfhe/UInt.h) through tests/cpp/uint_driver.cpp: user-style C++ against the
drop-in headers.  The driver builds everywhere; its flows run on an MI355X (`pytest -m gpu`)."""
import os

import pytest

from tests.cpp_driver import fixture, run_mode

driver = fixture("tests/cpp/uint_driver.cpp")


def test_uint_driver_builds(driver):
    assert os.path.exists(driver)


@pytest.mark.gpu
def test_uint_operations_decrypt_and_words(driver):
    run_mode(driver, "ops")


@pytest.mark.gpu
def test_uint_operations_on_ragged_planes(driver):
    run_mode(driver, "ragged")


@pytest.mark.gpu
def test_uint_encrypt_and_argument_checks(driver):
    run_mode(driver, "encrypt")


@pytest.mark.gpu
def test_uint_oversized_width_throws_first(driver):
    run_mode(driver, "oversize")
