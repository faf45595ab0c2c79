"""The whole oracle-vs-reference parity matrix (tests/test_oracle_vs_ref.py, 100 cases) re-run
with the DROP-IN library standing where the genuine reference stood.

oracle/ref_driver.cpp drives a certFHE implementation purely through the public class API; built
against /root/reference/src it is oracle/_ref (the genuine reference), built here against
include/certfhe + libcertFHE.so it is the MI355X drop-in.  Same driver, same tests, same expected
values from the oracle: seeded encrypt streams, mul incl. the left-operand Bitlen rule and *=,
add and +=, multi-term decrypt, permutations, keygen, the basic_operations flow.
"""
import os
import subprocess

import pytest

from oracle.binding import Ref
from tests.cpp_driver import ROOT, build

pytestmark = pytest.mark.gpu

DRIVER_SO = os.path.join(ROOT, "tests", "cpp", "libdropin_refdriver.so")


@pytest.fixture(scope="module")
def ref():
    """Overrides conftest's `ref`: the same extern-C driver, linked against the drop-in."""
    build("oracle/ref_driver.cpp", "tests/cpp/libdropin_refdriver.so", shared=True)
    r = Ref(DRIVER_SO)
    maps = open("/proc/self/maps").read()
    assert "libcertFHE.so" in maps and "libcsgn_hip.so" in maps, "the drop-in library is not the one loaded"
    # (the genuine reference, libcsgn_ref.so, may be mapped too when other test modules ran first in this
    # process: what matters is the library THIS driver calls, checked by test_fixture_is_the_dropin with ldd)
    return r


def test_fixture_is_the_dropin(ref):
    """Guard: the `ref` used by this module is the drop-in build of the driver, i.e. its
    ciphertext arithmetic runs in libcsgn_hip.so on the GPU."""
    import ctypes as C
    assert ref.lib._name == DRIVER_SO
    out = subprocess.run(["ldd", DRIVER_SO], capture_output=True, text=True).stdout
    assert "libcertFHE.so" in out and "libcsgn_hip.so" in out


# the test bodies are the reference-pinning ones, unchanged; only the `ref` fixture differs
from tests.test_oracle_vs_ref import (  # noqa: E402,F401
    test_add_matches_reference,
    test_basic_operations_program,
    test_context,
    test_decrypt_multiterm_matches_reference,
    test_encrypt_stream_matches_reference,
    test_keygen_restatement_reproduces_reference_key,
    test_large_products_digest,
    test_mul_matches_reference,
    test_permutation_generation_inverse_compose,
    test_permute_ciphertext_and_key,
    test_text_forms_match_reference,
)


def test_config5_circuit_through_the_class_api(ref):
    """BASELINE config 5 (Context(4096,32), depth 16) driven purely through the public classes of
    the drop-in: 766 terms at the end and the plaintext the circuit has in the clear; the genuine
    reference, where its build travelled with the snapshot, gives the same."""
    def clear(levels):
        bit = lambda i: int((i * 7 + 3) % 5 < 3)
        x, k = bit(0), 1
        for level in range(1, levels + 1):
            if level % 2:
                x ^= bit(k); k += 1
            else:
                x &= bit(k) ^ bit(k + 1); k += 2
        return x
    for n, d, levels, terms in [(4096, 32, 16, 766), (1247, 16, 16, 766), (1247, 16, 9, 47)]:
        t, got_terms, got_bit = ref.time_circuit(n, d, levels, 2)
        assert (got_terms, got_bit) == (terms, clear(levels)), (n, levels)
        from oracle.binding import load_ref
        genuine = load_ref()
        if genuine is not None:
            assert genuine.time_circuit(n, d, levels, 1)[1:] == (terms, clear(levels))
