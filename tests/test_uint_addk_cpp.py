"""Arithmetic with public constants, the bitwise operators and the shifts at the class level (include/certfhe/UInt.h)
through tests/cpp/uint_addk_driver.cpp: user-style C++ against the drop-in headers.  The driver builds everywhere
(tests/test_uint_addk_cpu.py); its flows run on an MI355X (`pytest -m gpu`)."""
import pytest

from tests.cpp_driver import fixture, run_mode

driver = fixture("tests/cpp/uint_addk_driver.cpp")
pytestmark = pytest.mark.gpu


def test_uint_addk_operators_decrypt_and_match_definition(driver):
    run_mode(driver, "ops")


def test_uint_addk_ragged_planes_same_words(driver):
    run_mode(driver, "ragged")


def test_uint_addk_errors_throw_first(driver):
    run_mode(driver, "errors")


def test_uint_addk_shifts_share_payloads(driver):
    run_mode(driver, "shared")
