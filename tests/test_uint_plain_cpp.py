"""Comparisons against a public constant at the class level (include/certfhe/UInt.h) through
tests/cpp/uint_plain_driver.cpp: user-style C++ against the drop-in headers.  The driver builds everywhere; its flows run
on an MI355X (`pytest -m gpu`)."""
import os

import pytest

from tests.cpp_driver import fixture, run_mode

driver = fixture("tests/cpp/uint_plain_driver.cpp")


def test_uint_plain_driver_builds(driver):
    assert os.path.exists(driver)


@pytest.mark.gpu
def test_uint_plain_comparisons_decrypt_and_words(driver):
    run_mode(driver, "ops")


@pytest.mark.gpu
def test_uint_plain_ragged_planes_same_words(driver):
    run_mode(driver, "ragged")


@pytest.mark.gpu
def test_uint_plain_oversize_throws_first(driver):
    run_mode(driver, "oversize")
