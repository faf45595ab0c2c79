"""Gather, slice, broadcast and concatenation at the class level (include/certfhe/Batch.h, UInt.h) through
tests/cpp/gather_driver.cpp: user-style C++ against the drop-in headers.  The driver builds everywhere; its flows run
on an MI355X (`pytest -m gpu`)."""
import os

import pytest

from tests.cpp_driver import NO_BLOCK_CACHE, fixture, run_mode

driver = fixture("tests/cpp/gather_driver.cpp")


def test_gather_driver_builds(driver):
    assert os.path.exists(driver)


@pytest.mark.gpu
def test_gather_slice_broadcast_concat_words(driver):
    run_mode(driver, "move")


@pytest.mark.gpu
def test_encrypted_query_broadcast(driver):
    run_mode(driver, "query")


@pytest.mark.gpu
def test_gather_bad_arguments_throw(driver):
    run_mode(driver, "throws")


# csgn_gather_plan's status words are a default path of every class-level gather with an index list or a ragged source:
# the same modes with every payload freed at once (hipMalloc / hipFree around each operator)
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["move", "query"])
def test_gather_driver_without_block_cache(driver, mode):
    run_mode(driver, mode, env=NO_BLOCK_CACHE)
