"""The class-level gates (include/certfhe/Gates.h) through tests/cpp/gates_driver.cpp: user-style C++ against the
drop-in headers.  The driver builds everywhere; its flows run on an MI355X (`pytest -m gpu`)."""
import os

import pytest

from tests.cpp_driver import fixture, run_mode

driver = fixture("tests/cpp/gates_driver.cpp")


def test_gates_driver_builds(driver):
    assert os.path.exists(driver)


@pytest.mark.gpu
def test_single_ciphertext_gates(driver):
    run_mode(driver, "single")


@pytest.mark.gpu
def test_batch_gates_uniform_and_ragged(driver):
    run_mode(driver, "batch")


@pytest.mark.gpu
def test_circuit_equality_and_less_than(driver):
    run_mode(driver, "circuit")
