"""a & b, a | b, a ^ b, ~a, a ^ k, select, keepWhere, hammingDistance and sumWhere at the class level
(include/certfhe/UInt.h) through tests/cpp/uint_bitwise_driver.cpp: user-style C++ against the drop-in headers.  The
driver builds everywhere; its flows run on an MI355X (`pytest -m gpu`)."""
import os

import pytest

from tests.cpp_driver import NO_BLOCK_CACHE, fixture, run_mode

driver = fixture("tests/cpp/uint_bitwise_driver.cpp")

KNOB = "CSGN_UINT_BITWISE_FORM"         # csgn_tuning.cpp's "uint_bitwise_form", as the library reads it when it loads
GATES = "CSGN_GATE_FUSED"               # csgn_gate_uniform's own knob: forced, it keeps the call on the planes form
KERNEL = "k_uint_bitwise"
SHAPES = 5 * 6 + 6                      # the driver's cases and its computed shape, times the six operations
FORMS = [pytest.param(0, id="planes"), pytest.param(1, id="kernel")]


def test_uint_bitwise_driver_builds(driver):
    assert os.path.exists(driver)


def test_the_knob_is_spelt_as_the_library_stores_it():
    """A misspelt variable silently leaves the default form, and a forced-form run then passes without having forced
    anything."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = open(os.path.join(root, "csgn_amd", "csrc", "csgn_tuning.cpp")).read()
    for knob in (KNOB, GATES):
        assert '{"%s", -1}' % knob[len("CSGN_"):].lower() in source


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["words", "ragged", "oversize"])
def test_uint_bitwise_driver(driver, mode):
    run_mode(driver, mode, env={KNOB: None, GATES: None})


# ---- both forms where the classes run them: one child process per configuration

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["words", "ragged", "oversize"])
@pytest.mark.parametrize("form", FORMS)
def test_uint_bitwise_driver_forced_form(driver, form, mode):
    run_mode(driver, mode, env={KNOB: str(form), GATES: None})


@pytest.mark.gpu
def test_uint_bitwise_driver_planes_without_block_cache(driver):
    run_mode(driver, "words", env=dict({KNOB: "0", GATES: None}, **NO_BLOCK_CACHE))


# A forced form must be shown to have run: the classes name their route and the library the form each shape takes under
# the forced knob (the driver's `forms` mode, no device work).
def form_rows(driver, env):
    p = run_mode(driver, "forms", env=env)
    rows = [line.split(" -> ") for line in p.stdout.splitlines() if " -> " in line]
    assert len(rows) == SHAPES, p.stdout[-2000:]
    return [(shape, *got.split()) for shape, got in rows]


@pytest.mark.parametrize("form", FORMS)
def test_uint_bitwise_driver_forced_form_is_the_form_that_runs(driver, form):
    for shape, route, kernel in form_rows(driver, {KNOB: str(form), GATES: None}):
        assert route == "call", (shape, route, form)                  # uniform planes: one call in either form
        assert kernel == (KERNEL if form == 1 else "planes"), (shape, kernel, form)


@pytest.mark.parametrize("gates", [0, 1])
def test_a_forced_gate_form_keeps_the_call_on_the_planes(driver, gates):
    """tests/test_uint_cpp.py forces gate_fused to run csgn_gate_uniform's two forms through these very operators: with
    that knob forced and uint_bitwise_form left alone, the call issues the launchers plane by plane."""
    for shape, route, kernel in form_rows(driver, {KNOB: None, GATES: str(gates)}):
        assert route == "call" and kernel == "planes", (shape, route, kernel, gates)


def test_the_default_route_is_the_one_call(driver):
    for shape, route, kernel in form_rows(driver, {KNOB: None, GATES: None}):
        assert route == "call" and kernel in (KERNEL, "planes"), (shape, route, kernel)
