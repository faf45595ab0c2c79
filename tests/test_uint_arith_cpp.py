"""a + b, a - b, add / sub with the carry, equalTo, notEqualTo, lessThan and greaterThan at the class level
(include/certfhe/UInt.h) through tests/cpp/uint_arith_driver.cpp: user-style C++ against the drop-in headers.  The driver
builds everywhere; its flows run on an MI355X (`pytest -m gpu`)."""
import os

import pytest

from tests.cpp_driver import FORMS, NO_BLOCK_CACHE, fixture, run_mode

driver = fixture("tests/cpp/uint_arith_driver.cpp")

KNOB = "CSGN_UINT_ARITH_FORM"           # csgn_tuning.cpp's "uint_arith_form", as the library reads it when it loads
STEPS = "CSGN_UINT_FUSED"               # csgn_uint_step's own knob: forced, it keeps the classes on the chain
FUSED = "k_uint_arith"
SHAPES = 5 * 4                          # the driver's cases times the four operations


def test_uint_arith_driver_builds(driver):
    assert os.path.exists(driver)


def test_the_knob_is_spelt_as_the_library_stores_it():
    """A misspelt variable silently leaves the default form, and a forced-form run then passes without having forced
    anything."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = open(os.path.join(root, "csgn_amd", "csrc", "csgn_tuning.cpp")).read()
    for knob in (KNOB, STEPS):
        assert '{"%s", -1}' % knob[len("CSGN_"):].lower() in source


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["words", "ragged", "oversize"])
def test_uint_arith_driver(driver, mode):
    run_mode(driver, mode, env={KNOB: None, STEPS: None})


# ---- both forms where the classes run them: one child process per configuration

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["words", "ragged", "oversize"])
@pytest.mark.parametrize("form", FORMS)
def test_uint_arith_driver_forced_form(driver, form, mode):
    run_mode(driver, mode, env={KNOB: str(form), STEPS: None})


@pytest.mark.gpu
def test_uint_arith_driver_chain_without_block_cache(driver):
    run_mode(driver, "words", env=dict({KNOB: "0", STEPS: None}, **NO_BLOCK_CACHE))


# A forced form must be shown to have run: the classes name their route and the library the form each shape takes under
# the forced knob (the driver's `forms` mode, no device work).
def form_rows(driver, env):
    p = run_mode(driver, "forms", env=env)
    rows = [line.split(" -> ") for line in p.stdout.splitlines() if " -> " in line]
    assert len(rows) == SHAPES, p.stdout[-2000:]
    return [(shape, *got.split()) for shape, got in rows]


@pytest.mark.parametrize("form", FORMS)
def test_uint_arith_driver_forced_form_is_the_form_that_runs(driver, form):
    for shape, route, kernel in form_rows(driver, {KNOB: str(form), STEPS: None}):
        assert route == ("call" if form == 1 else "chain"), (shape, route, form)
        assert kernel == (FUSED if form == 1 else "composed"), (shape, kernel, form)


@pytest.mark.parametrize("steps", FORMS)
def test_a_forced_step_form_keeps_the_classes_on_the_chain(driver, steps):
    """tests/test_uint_cpp.py forces uint_fused to run csgn_uint_step's two forms through these very operators: with
    that knob forced and uint_arith_form left alone, the classes name the chain."""
    for shape, route, _ in form_rows(driver, {KNOB: None, STEPS: str(steps)}):
        assert route == "chain", (shape, route, steps)


def test_the_default_route_is_the_one_call(driver):
    for shape, route, kernel in form_rows(driver, {KNOB: None, STEPS: None}):
        assert route == "call" and kernel in (FUSED, "composed"), (shape, route, kernel)
