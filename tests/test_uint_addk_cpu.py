"""A bit-sliced integer plus a PUBLIC constant (csgn_uint_addk_*) on a box without a GPU: the DEFINITION -- a composition
of the reference's operator+ / operator* with ONE -- pinned against the compiled reference and the oracle, the term
counts, the dispatch names and knob, the loud failure without a device, and decryptions under random keys, which equal
clear arithmetic for every value and constant of the small widths.  The device side is tests/test_uint_addk_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.cpp_driver import fixture, run_mode
from tests.model import const_term, decrypt_bits, decrypt_value, encrypt_planes, lib, oracle_ops, rand_terms, ref_ops, u64s
from tests.model_addk import (addk_terms, compose_addk, full_width_ks, mask, neg_k, np_addk, rsub_k, sub_k, term_modes)

driver = fixture("tests/cpp/uint_addk_driver.cpp")
MODES = ["1", "2", "3", "mixed"]


def c_terms(lib, w, k, ts):
    out = (C.c_uint64 * 65)()
    ok = lib.csgn_uint_addk_terms(w, k, u64s(ts) if ts is not None else None, out)
    return list(out)[:w + 1] if ok else None


# -- the definition against the genuine reference and the oracle -----------------------------------------------------
@pytest.mark.parametrize("n,d", [(65, 4), (1247, 16)])
@pytest.mark.parametrize("tmode", MODES)
@pytest.mark.parametrize("w", [1, 2, 3, 4, 5])
def test_addk_definition_matches_reference_and_oracle(oracle, ref, n, d, w, tmode):
    rng = np.random.default_rng(w * 10 + len(tmode))
    ts = term_modes(w, tmode, rng)
    dl = (n + 63) // 64
    planes = [rand_terms(n, 1, t, 40 + j)[0].ravel() for j, t in enumerate(ts)]
    one, zero = const_term(n, 1), const_term(n, 0)
    for k in range(1 << w):
        want, want_c = compose_addk(planes, k, *ref_ops(ref, n, d), one, zero)
        got, got_c = compose_addk(planes, k, *oracle_ops(oracle, n), one, zero)
        counts = addk_terms(w, k, ts)
        for negate in (False, True):
            words, carry = np_addk(n, [p.reshape(1, t, -1) for p, t in zip(planes, ts)], k, negate)
            add_r, add_o = ref_ops(ref, n, d)[0], oracle_ops(oracle, n)[0]
            for j in range(w):
                wj = add_r(want[j], one) if negate else want[j]
                gj = add_o(got[j], one) if negate else got[j]
                assert np.array_equal(gj, wj), (k, j, negate)
                assert np.array_equal(words[j].ravel(), wj), (k, j, negate)
                assert wj.size == (counts[j] + negate) * dl
            assert np.array_equal(got_c, want_c) and np.array_equal(carry.ravel(), want_c), k   # never negated
            assert want_c.size == counts[w] * dl


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_addk_terms_formulas(lib):
    for w in range(1, 9):
        for tmode in MODES:
            ts = term_modes(w, tmode, np.random.default_rng(w * 10 + len(tmode)))
            for k in range(1 << w):
                assert c_terms(lib, w, k, ts) == addk_terms(w, k, ts), (w, k, ts)
    for w in (17, 31, 32, 33, 63, 64):
        for k in full_width_ks(w):
            counts = addk_terms(w, k, [1] * w)
            assert c_terms(lib, w, k, [1] * w) == counts, (w, k)
            assert max(counts[:w]) <= 129 and counts[w] <= 255, (w, k)


def test_addk_terms_fresh_planes():
    """The sizes of the definition's text for fresh 1-term planes."""
    for w in range(1, 9):
        worst = 0
        for k in range(1 << w):
            counts = addk_terms(w, k, [1] * w)
            worst = max(worst, max(counts[:w]))
            if k:
                m = (k & -k).bit_length() - 1
                for j in range(m + 1, w + 1):
                    carry_into = counts[j] - (1 + ((k >> j) & 1)) if j < w else counts[w]
                    assert carry_into <= 2 ** bin(k >> m & mask(j - m)).count("1") - 1, (w, k, j)
        assert worst <= 2 ** (w - 1) + 1
        assert addk_terms(w, 1, [1] * w)[:w] == [2] * w
    assert max(addk_terms(8, 255, [1] * 8)[:8]) == 129
    assert addk_terms(16, 1, [1] * 16)[:16] == [2] * 16 and addk_terms(32, 1, [1] * 32)[32] == 1


def test_addk_terms_invalid(lib):
    one = [1] * 64
    assert c_terms(lib, 0, 0, one) is None and c_terms(lib, 65, 0, one) is None        # width outside 1..64
    assert c_terms(lib, 4, 16, one) is None and c_terms(lib, 8, 1 << 40, one) is None  # k >= 2^w
    assert c_terms(lib, 64, (1 << 64) - 2, one) is None                                # 2^63 - 1 carry terms: overflow
    assert c_terms(lib, 64, 1 << 63, one) == [1] * 63 + [2, 1]                         # every k fits 64 bits
    assert c_terms(lib, 3, 1, [1, 0, 1]) is None                                       # a plane of no terms
    assert c_terms(lib, 3, 0, [1, 0, 1]) is None
    assert c_terms(lib, 2, 0, None) is None
    assert lib.csgn_uint_addk_terms(2, 0, u64s([1, 1]), None) == 0
    assert c_terms(lib, 2, 1, [1 << 40, 1 << 40]) is None                              # overflow
    assert c_terms(lib, 1, 1, [(1 << 64) - 1]) is None
    assert c_terms(lib, 63, (1 << 63) - 1, one) is None and c_terms(lib, 62, (1 << 62) - 1, one) is not None


def test_addk_terms_sweep(lib):
    """csgn_uint_addk_terms over the sweep of tests/test_uint_plain_cpu.py: the model's counts, and a refusal for
    whatever include/csgn_hip.h calls invalid."""
    from tests.test_uint_plain_cpu import SWEEP_WIDTHS, sweep_constants, sweep_term_vectors
    rng = np.random.default_rng(18)
    for w in SWEEP_WIDTHS:
        for ts in sweep_term_vectors(w, rng):
            for k in sweep_constants(w, rng):
                valid = 1 <= w <= 64 and k >> w == 0 and all(0 < t < (1 << 62) for t in ts[:w])
                if valid and k and ts[(k & -k).bit_length() - 1] == (1 << 62) - 1:
                    continue        # out_m = t_m + 1 = 2^62 terms: refused by the model, let through by the library,
                                    # whose limit is on the carries and the planes above m; not pinned either way
                want = addk_terms(w, k, ts[:w]) if valid else None
                assert c_terms(lib, min(w, 65), k, ts) == want, (w, k, ts[:w])


def test_addk_dispatch_names(lib, knobs):
    knobs.unset("uint_addk_fused")

    def name(w, k, carry=0, ts=None, n=1247):
        return lib.csgn_uint_addk_kernel(n, 1 << 16, w, k, u64s(ts or [1] * w), carry).decode()

    assert name(8, 1) == "k_uint_addk" and name(16, 0xFF00, 1) == "k_uint_addk" and name(8, 0) == "k_uint_addk"
    assert name(8, 100) == "k_uint_addk" and name(32, 0xFF000000) == "k_uint_addk" and name(8, 255) == "k_uint_addk"
    assert name(32, 1) == "composed" and name(32, 3) == "composed"            # 16 levels walked per chain term: measured slower
    assert name(16, 1) == "composed"                                          # 8 levels: measured a tie
    assert lib.csgn_uint_addk_kernel(1247, 1 << 20, 8, 255, u64s([1] * 8), 0) == b"composed"   # 45 GB of outputs
    assert name(1, 1) == "composed" and name(1, 1, 1) == "k_uint_addk"        # a single plane: one copy and a constant
    assert name(4, 16) == "" and name(0, 0) == "" and name(4, 1, n=0) == ""
    knobs.set("uint_addk_fused", 0)
    assert name(8, 1) == "composed" and name(16, 4711, 1, [2] * 16) == "composed"
    knobs.set("uint_addk_fused", 1)
    assert name(1, 1) == "k_uint_addk" and name(32, 1) == "k_uint_addk"


def test_addk_argument_errors_come_before_the_device(lib):
    """Argument errors and size limits are reported before the device is looked for: with or without a GPU."""
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    planes = (C.c_void_p * 64)(*([p] * 64))
    one = u64s([1] * 64)
    assert lib.csgn_uint_addk(0, 4, 8, 77, 0, planes, one, planes, None, None) == -1
    assert lib.csgn_uint_addk(1247, 4, 8, 256, 0, planes, one, planes, None, None) == -1
    assert lib.csgn_uint_addk(1247, 4, 65, 0, 0, planes, one, planes, None, None) == -1
    assert lib.csgn_uint_addk(1247, 4, 0, 0, 0, planes, one, planes, None, None) == -1
    assert lib.csgn_uint_addk(1247, 4, 3, 1, 0, planes, u64s([1, 0, 1]), planes, None, None) == -1
    assert lib.csgn_uint_addk(1247, 4, 3, 1, 0, None, one, planes, None, None) == -1
    assert lib.csgn_uint_addk(1247, 4, 3, 1, 0, planes, one, None, None, None) == -1
    # too large: the carry into plane 28 of a + (2^29 - 1) has 2^28 - 1 terms, 20 words each
    assert lib.csgn_uint_addk(1247, 4, 29, (1 << 29) - 1, 0, planes, one, planes, None, None) == -2
    assert lib.csgn_uint_addk(1247, 4, 27, (1 << 27) - 1, 0, planes, one, planes, p, None) == -2    # the carry-out alone
    assert lib.csgn_uint_addk(1247, 1 << 56, 8, 1, 0, planes, one, planes, None, None) == -2        # batch


def test_addk_fails_without_gpu(lib, driver):
    import torch
    if torch.cuda.is_available():
        return                                      # nothing to refuse: tests/test_uint_addk_gpu.py covers the device
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    planes = (C.c_void_p * 64)(*([p] * 64))
    one = u64s([1] * 64)
    assert lib.csgn_uint_addk(1247, 4, 8, 77, 0, planes, one, planes, None, None) == -3, lib.csgn_last_error()
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert lib.csgn_uint_addk(1247, 4, 8, 0, 1, planes, one, planes, p, None) == -3
    assert lib.csgn_uint_addk(1247, 4, 27, (1 << 27) - 1, 0, planes, one, planes, None, None) == -3   # fits: the device is asked
    run_mode(driver, "nodevice")                    # the classes throw


def test_addk_driver_builds(driver):
    import os
    assert os.path.exists(driver)


# -- meaning: decryptions under random keys, exhaustive at the small widths ------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6])
def test_addk_decrypts_to_clear_arithmetic(oracle, w):
    n, d = 127, 8
    x = np.arange(1 << w, dtype=np.uint64)
    m = np.uint64(mask(w))
    for trial in range(3):
        key, _ = oracle.keygen(n, d, glibc_draws(700 + 10 * w + trial, 64 * d + 64))
        planes = encrypt_planes(oracle, n, key, x, w, 800 + 10 * w + trial)
        for k in range(1 << w):
            outs, carry = np_addk(n, planes, k)
            assert max(o.shape[1] for o in outs) <= 2 ** (w - 1) + 1
            assert np.array_equal(decrypt_value(oracle, n, key, outs), (x + np.uint64(k)) & m), k
            assert np.array_equal(decrypt_bits(oracle, n, key, carry), ((x + np.uint64(k)) >> np.uint64(w)) != 0), k
            kk, negate = rsub_k(w, k)                                        # k - a
            outs, _ = np_addk(n, planes, kk, negate)
            assert np.array_equal(decrypt_value(oracle, n, key, outs), (np.uint64(k) - x) & m), k
        for k in {0, 1, mask(w), 1 << (w - 1), 5 & mask(w)}:                 # a - k is a + (2^w - k): every sum is above
            kk, negate = sub_k(w, k)
            assert np.array_equal(decrypt_value(oracle, n, key, np_addk(n, planes, kk, negate)[0]), (x - np.uint64(k)) & m)
        kk, negate = neg_k(w)                                                # -a
        assert np.array_equal(decrypt_value(oracle, n, key, np_addk(n, planes, kk, negate)[0]), (np.uint64(0) - x) & m)


def test_addk_clear_bit_recurrence():
    """The algebra of the definition in clear bits, every w <= 8, k and x: the planes are (x + k) mod 2^w, the carry-out
    the bit that left, and ~(x + ~k) = k - x."""
    for w in range(1, 9):
        x = np.arange(1 << w, dtype=np.uint64)
        bits = [((x >> np.uint64(j)) & np.uint64(1)) for j in range(w)]
        for k in range(1 << w):
            outs, carry = compose_addk(bits, k, lambda a, b: a ^ b, lambda a, b: a & b, np.uint64(1), np.zeros_like(x))
            v = sum(o << np.uint64(j) for j, o in enumerate(outs))
            assert np.array_equal(v, (x + np.uint64(k)) & np.uint64(mask(w))), (w, k)
            assert np.array_equal(carry, (x + np.uint64(k)) >> np.uint64(w)), (w, k)
            outs, _ = compose_addk(bits, ~k & mask(w), lambda a, b: a ^ b, lambda a, b: a & b, np.uint64(1), np.zeros_like(x))
            v = sum((o ^ np.uint64(1)) << np.uint64(j) for j, o in enumerate(outs))
            assert np.array_equal(v, (np.uint64(k) - x) & np.uint64(mask(w))), (w, k)
