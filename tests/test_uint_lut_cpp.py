"""Public lookup tables at the class level (include/certfhe/UInt.h) through
tests/cpp/uint_lut_driver.cpp: user-style C++ against the drop-in headers.  The driver builds everywhere; its flows run
on an MI355X (`pytest -m gpu`)."""
import os

import pytest

from tests.cpp_driver import FORMS, NO_BLOCK_CACHE, check_forced_forms, fixture, form_env, run_mode

driver = fixture("tests/cpp/uint_lut_driver.cpp")


def test_uint_lut_driver_builds(driver):
    assert os.path.exists(driver)


@pytest.mark.gpu
def test_uint_lut_sbox_decrypts_and_words(driver):
    run_mode(driver, "sbox")


@pytest.mark.gpu
def test_uint_lut_two_input_lookups(driver):
    run_mode(driver, "two")


@pytest.mark.gpu
def test_uint_lut_ragged_planes_same_words(driver):
    run_mode(driver, "ragged")


@pytest.mark.gpu
def test_uint_lut_oversize_throws_first(driver):
    run_mode(driver, "oversize")


# ---- every form where the classes run it (tests/cpp_driver.py, FORM_KNOBS): one child process per configuration

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ['sbox', 'two', 'ragged'])
@pytest.mark.parametrize("form", FORMS)
def test_uint_lut_driver_forced_form(driver, form, mode):
    run_mode(driver, mode, env=form_env("uint_lut", form))


@pytest.mark.gpu
def test_uint_lut_driver_composed_without_block_cache(driver):
    run_mode(driver, "sbox", env=dict(form_env("uint_lut", 0), **NO_BLOCK_CACHE))


# A forced form must be shown to have run: a misspelt CSGN_... leaves the default form and every forced run above goes
# green for nothing.  The library itself names the form each shape takes under the forced knob (the driver's `forms`
# mode); the shapes that take one form whatever the knob says are those include/csgn_hip.h documents, listed here.
@pytest.mark.gpu                                                    # compiling the table uploads it
@pytest.mark.parametrize("form", FORMS)
def test_uint_lut_driver_forced_form_is_the_form_that_runs(driver, form):
    rows = check_forced_forms(driver, "uint_lut", form)              # no shape is documented as keeping one form
    assert len(rows) == 2
