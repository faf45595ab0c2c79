"""Arithmetic with public constants, the bitwise operators and the shifts at the class level (include/certfhe/UInt.h)
through tests/cpp/uint_addk_driver.cpp: user-style C++ against the drop-in headers.  The driver builds everywhere
(tests/test_uint_addk_cpu.py); its flows run on an MI355X (`pytest -m gpu`)."""
import pytest

from tests.cpp_driver import FORMS, NO_BLOCK_CACHE, check_forced_forms, fixture, form_env, run_mode

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


# ---- every form where the classes run it (tests/cpp_driver.py, FORM_KNOBS): one child process per configuration

@pytest.mark.parametrize("mode", ['ops', 'ragged'])
@pytest.mark.parametrize("form", FORMS)
def test_uint_addk_driver_forced_form(driver, form, mode):
    run_mode(driver, mode, env=form_env("uint_addk", form))


def test_uint_addk_driver_composed_without_block_cache(driver):
    run_mode(driver, "ops", env=dict(form_env("uint_addk", 0), **NO_BLOCK_CACHE))


# A forced form must be shown to have run: a misspelt CSGN_... leaves the default form and every forced run above goes
# green for nothing.  The library itself names the form each shape takes under the forced knob (the driver's `forms`
# mode); the shapes that take one form whatever the knob says are those include/csgn_hip.h documents, listed here.
ALWAYS_COMPOSED = [lambda shape: shape.startswith("w=28 ")]      # one element's planes past a launch's 2^32 lanes


@pytest.mark.parametrize("form", FORMS)
def test_uint_addk_driver_forced_form_is_the_form_that_runs(driver, form):
    rows = check_forced_forms(driver, "uint_addk", form, always_composed=ALWAYS_COMPOSED)
    assert len(rows) == 2 * (7 + 8) + 1
