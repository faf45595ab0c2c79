"""The class-level gates (include/certfhe/Gates.h) through tests/cpp/gates_driver.cpp: user-style C++ against the
drop-in headers.  The driver builds everywhere; its flows run on an MI355X (`pytest -m gpu`)."""
import os

import pytest

from tests.cpp_driver import FORMS, NO_BLOCK_CACHE, check_forced_forms, fixture, form_env, run_mode

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


# ---- every form where the classes run it (tests/cpp_driver.py, FORM_KNOBS): one child process per configuration

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ['single', 'batch', 'circuit'])
@pytest.mark.parametrize("form", FORMS)
def test_gates_driver_forced_form(driver, form, mode):
    run_mode(driver, mode, env=form_env("gates", form))


@pytest.mark.gpu
def test_gates_driver_composed_without_block_cache(driver):
    run_mode(driver, "batch", env=dict(form_env("gates", 0), **NO_BLOCK_CACHE))    # the uniform-batch pitched form at size


# A forced form must be shown to have run: a misspelt CSGN_... leaves the default form and every forced run above goes
# green for nothing.  The library itself names the form each shape takes under the forced knob (the driver's `forms`
# mode); the shapes that take one form whatever the knob says are those include/csgn_hip.h documents, listed here.
ALWAYS_FUSED = [lambda shape: shape.startswith("MUL_PLAIN "),                       # no composed form
                lambda shape: shape.startswith("MUX ") and " ts=1 " not in shape]    # MUX with t_sel > 1


@pytest.mark.parametrize("form", FORMS)
def test_gates_driver_forced_form_is_the_form_that_runs(driver, form):
    rows = check_forced_forms(driver, "gates", form, always_fused=ALWAYS_FUSED)
    assert len(rows) == 4 * 8
