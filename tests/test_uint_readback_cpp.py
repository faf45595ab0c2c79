"""readAtEach over what writeAtEach returns at the class level (include/certfhe/UInt.h, "the read that follows") through
tests/cpp/uint_readback_driver.cpp: user-style C++ against the drop-in headers.  The driver builds everywhere; its flows
run on an MI355X (`pytest -m gpu`), once with knob uint_pick_rows_form left alone and once in each forced form, one child
process per configuration."""
import os

import pytest

from tests.cpp_driver import FORMS, NO_BLOCK_CACHE, fixture, run_mode

driver = fixture("tests/cpp/uint_readback_driver.cpp")

KNOB = "CSGN_UINT_PICK_ROWS_FORM"       # csgn_tuning.cpp's "uint_pick_rows_form", as the library reads it when it loads
FUSED = "k_uint_pick_rows"
SHAPES = 7                              # the cases of the driver's `words` mode
MODES = ["routes", "words", "oversize"]


def test_uint_readback_driver_builds(driver):
    assert os.path.exists(driver)


def test_the_knob_is_spelt_as_the_library_stores_it():
    """A misspelt variable silently leaves the default form, and a forced-form run then passes without having forced
    anything."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = open(os.path.join(root, "csgn_amd", "csrc", "csgn_tuning.cpp")).read()
    assert '{"%s", -1}' % KNOB[len("CSGN_"):].lower() in source


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_uint_readback_driver(driver, mode):
    run_mode(driver, mode, env={KNOB: None})


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", FORMS)
def test_uint_readback_driver_forced_form(driver, form, mode):
    run_mode(driver, mode, env={KNOB: str(form)})


@pytest.mark.gpu
def test_uint_readback_driver_composed_without_block_cache(driver):
    run_mode(driver, "words", env=dict({KNOB: "0"}, **NO_BLOCK_CACHE))


# A forced form must be shown to have run: the library itself names the form each shape takes under the forced knob (the
# driver's `forms` mode, no device work).
@pytest.mark.parametrize("form", FORMS)
def test_uint_readback_driver_forced_form_is_the_form_that_runs(driver, form):
    p = run_mode(driver, "forms", env={KNOB: str(form)})
    rows = [line.split(" -> ") for line in p.stdout.splitlines() if " -> " in line]
    assert len(rows) == SHAPES, p.stdout[-2000:]
    for shape, got in rows:
        assert got.strip() == (FUSED if form == 1 else "composed"), (shape, got, form)


def test_uint_readback_driver_default_form_is_fused(driver):
    p = run_mode(driver, "forms", env={KNOB: None})
    rows = [line.split(" -> ") for line in p.stdout.splitlines() if " -> " in line]
    assert len(rows) == SHAPES and all(got.strip() == FUSED for _, got in rows), p.stdout[-2000:]
