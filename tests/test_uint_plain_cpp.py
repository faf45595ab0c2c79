"""Comparisons against a public constant at the class level (include/certfhe/UInt.h) through
tests/cpp/uint_plain_driver.cpp: user-style C++ against the drop-in headers.  The driver builds everywhere; its flows run
on an MI355X (`pytest -m gpu`)."""
import os

import pytest

from tests.cpp_driver import FORMS, NO_BLOCK_CACHE, check_forced_forms, fixture, form_env, form_lines, run_mode

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


# ---- every form where the classes run it (tests/cpp_driver.py, FORM_KNOBS): one child process per configuration

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ['ops', 'ragged'])
@pytest.mark.parametrize("form", FORMS)
def test_uint_plain_driver_forced_form(driver, form, mode):
    run_mode(driver, mode, env=form_env("uint_plain", form))


@pytest.mark.gpu
def test_uint_plain_driver_composed_without_block_cache(driver):
    run_mode(driver, "ops", env=dict(form_env("uint_plain", 0), **NO_BLOCK_CACHE))


# A forced form must be shown to have run: a misspelt CSGN_... leaves the default form and every forced run above goes
# green for nothing.  The library itself names the form each shape takes under the forced knob (the driver's `forms`
# mode); the shapes that take one form whatever the knob says are those include/csgn_hip.h documents, listed here.
# csgn_uint_plain keeps no shape from a forced knob: "composed for width 1 and the ZERO results" is the PER SHAPE rule,
# the one the default run below checks.


@pytest.mark.parametrize("form", FORMS)
def test_uint_plain_driver_forced_form_is_the_form_that_runs(driver, form):
    rows = check_forced_forms(driver, "uint_plain", form)
    assert len(rows) == 16 * 6 * 6


def test_uint_plain_driver_default_form_per_shape(driver):
    """Without the knob: composed for width 1 and the constant results (lessThan 0, greaterEqual 0, greaterThan 2^w - 1,
    lessEqual 2^w - 1), fused otherwise."""
    rows = form_lines(driver, "uint_plain", None)
    assert len(rows) == 16 * 6 * 6
    for shape, got in rows:
        w, cmp, k = shape.split()
        w, k = int(w[2:]), int(k[2:])
        constant = (cmp in ("lessThan", "greaterEqual") and k == 0) or (cmp in ("greaterThan", "lessEqual") and k == 2 ** w - 1)
        assert got == ("composed" if w == 1 or constant else "k_uint_plain"), shape
