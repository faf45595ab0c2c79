"""addWhere, subWhere, incrementWhere and decrementWhere at the class level (include/certfhe/UInt.h) through
tests/cpp/uint_add_where_driver.cpp: user-style C++ against the drop-in headers.  The driver builds everywhere; its
flows run on an MI355X (`pytest -m gpu`)."""
import os

import pytest

from tests.cpp_driver import FORMS, NO_BLOCK_CACHE, fixture, run_mode

driver = fixture("tests/cpp/uint_add_where_driver.cpp")

KNOB = "CSGN_UINT_ADD_WHERE_FORM"       # csgn_tuning.cpp's "uint_add_where_form", as the library reads it when it loads
SHAPES = 8 * 2                          # the driver's widths, uniform and ragged


def test_uint_add_where_driver_builds(driver):
    assert os.path.exists(driver)


def test_the_knob_is_spelt_as_the_library_stores_it():
    """A misspelt variable silently leaves the default route, and a forced run then passes without having forced
    anything."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = open(os.path.join(root, "csgn_amd", "csrc", "csgn_tuning.cpp")).read()
    assert '{"%s", -1}' % KNOB[len("CSGN_"):].lower() in source


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["words", "ragged", "oversize"])
def test_uint_add_where_driver(driver, mode):
    run_mode(driver, mode, env={KNOB: None})


# ---- both routes where the classes run them: one child process per configuration

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["words", "ragged", "oversize"])
@pytest.mark.parametrize("form", FORMS)
def test_uint_add_where_driver_forced_form(driver, form, mode):
    run_mode(driver, mode, env={KNOB: str(form)})


@pytest.mark.gpu
def test_uint_add_where_driver_without_block_cache(driver):
    run_mode(driver, "words", env=dict({KNOB: None}, **NO_BLOCK_CACHE))


# A forced route must be shown to have run: the classes name their route under the forced knob (the driver's `forms`
# mode, no device work).
def form_rows(driver, env):
    p = run_mode(driver, "forms", env=env)
    rows = [line.split(" -> ") for line in p.stdout.splitlines() if " -> " in line]
    assert len(rows) == SHAPES, p.stdout[-2000:]
    return [(shape.split()[0], shape.split()[1], route.strip()) for shape, route in rows]


def can_call(width, kind):
    return int(width[2:]) <= 32 and kind == "uniform"


@pytest.mark.parametrize("form", FORMS)
def test_uint_add_where_driver_forced_form_is_the_route_that_runs(driver, form):
    for width, kind, route in form_rows(driver, {KNOB: str(form)}):
        assert route == ("call" if form == 1 and can_call(width, kind) else "loop"), (width, kind, route, form)


def test_the_default_route_is_the_one_call_where_it_can_run(driver):
    for width, kind, route in form_rows(driver, {KNOB: None}):
        assert route == ("call" if can_call(width, kind) else "loop"), (width, kind, route)
