"""Encrypted tables read at encrypted indices at the class level (include/certfhe/UInt.h, readAt) through
tests/cpp/uint_read_driver.cpp: user-style C++ against the drop-in headers.  The driver builds everywhere; its flows run
on an MI355X (`pytest -m gpu`)."""
import os

import pytest

from tests.cpp_driver import fixture, run_mode

driver = fixture("tests/cpp/uint_read_driver.cpp")


def test_uint_read_driver_builds(driver):
    assert os.path.exists(driver)


@pytest.mark.gpu
def test_uint_read_words_and_decryptions(driver):
    run_mode(driver, "words")


@pytest.mark.gpu
def test_uint_read_ragged_planes_same_words(driver):
    run_mode(driver, "ragged")


@pytest.mark.gpu
def test_uint_read_oversize_throws_first(driver):
    run_mode(driver, "oversize")
