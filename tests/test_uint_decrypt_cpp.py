"""The two ends of an encrypted-integer pipeline at the class level (include/certfhe/UInt.h): UIntBatch::encrypt in one
block and one launch, UIntBatch::decrypt and decryptPacked in one csgn_uint_decrypt, through
tests/cpp/uint_decrypt_driver.cpp: user-style C++ against the drop-in headers.  The driver builds everywhere; its flows
run on an MI355X (`pytest -m gpu`), once with knob uint_decrypt_form left alone, once at 0 (one CiphertextBatch::decrypt
per plane) and once at 1 (the one call): one child process each, the library reads the variable when it loads."""
import os

import pytest

from tests.cpp_driver import fixture, run_mode

driver = fixture("tests/cpp/uint_decrypt_driver.cpp")

KNOB = "CSGN_UINT_DECRYPT_FORM"         # csgn_tuning.cpp's "uint_decrypt_form", as the library reads it when it loads
MODES = ["roundtrip", "seeded", "arith", "lifetime", "refusals"]
FORMS = [pytest.param(None, id="unset"), pytest.param(0, id="planes"), pytest.param(1, id="call")]


def test_uint_decrypt_driver_builds(driver):
    assert os.path.exists(driver)


def test_the_knob_is_spelt_as_the_library_stores_it():
    """A misspelt variable silently leaves the default, and a forced run then passes without having forced anything."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = open(os.path.join(root, "csgn_amd", "csrc", "csgn_tuning.cpp")).read()
    assert '{"%s", -1}' % KNOB[len("CSGN_"):].lower() in source


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", FORMS)
def test_uint_decrypt_driver(driver, form, mode):
    p = run_mode(driver, mode, env={KNOB: None if form is None else str(form)})
    routes = [line.split(" -> ") for line in p.stdout.splitlines() if " -> " in line]
    if mode in ("roundtrip", "arith"):
        assert routes, p.stdout[-2000:]
    for shape, route in routes:                     # the forced route is the route that ran
        past_the_bound = shape.startswith("ragged 4097")
        assert route.strip() == ("planes" if form == 0 or past_the_bound else "call"), (shape, route, form)
