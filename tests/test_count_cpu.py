"""Encrypted bits counted into encrypted integers (csgn_count*) on a box without a GPU: the term count and its edges,
the dispatch names and knobs, the argument checks and their order, the loud failure without a device, and the
DEFINITION -- plane j the left-nested sum, over the 2^j-subsets in lexicographic order, of the left-nested products of
the subset's inputs -- pinned against the oracle and the compiled reference, with decryptions under random keys.  The
device side is tests/test_count_gpu.py."""
import ctypes as C
from math import comb

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import INVALID, LIMIT, NO_DEVICE, UNSUPPORTED, decrypt_bits, lib, oracle_ops, rand_terms, ref_ops  # noqa: F401
from tests.model_count import compose_count, count_terms, np_count, popcount_planes


def js_array(js):
    return (C.c_uint64 * max(len(js), 1))(*js)


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_terms_against_the_model(lib):
    for g in range(1, 71):
        for t in (1, 2, 3, 1 << 31, LIMIT - 1, LIMIT):
            for j in range(8):
                assert lib.csgn_count_terms(g, t, j) == count_terms(g, t, j), (g, t, j)
    assert lib.csgn_count_terms(0, 1, 0) == 0 == count_terms(0, 1, 0)
    assert lib.csgn_count_terms(5, 0, 0) == 0 == count_terms(5, 0, 0)
    # the term counts the header names
    assert [lib.csgn_count_terms(64, 1, j) for j in (0, 1, 2, 6)] == [64, 2016, 635376, 1]
    assert lib.csgn_count_terms(65, 1, 6) == 65
    assert lib.csgn_count_terms(8, 3, 1) == 28 * 9 and lib.csgn_count_terms(8, 3, 2) == 70 * 81


def test_terms_at_the_edge_of_2_62(lib):
    """C(65, 32) lies below 2^62 and comes out exact; C(66, 32) does not, and gives 0: nothing wraps on the way."""
    assert comb(65, 32) == 3609714217008132870 < LIMIT <= comb(66, 32)
    assert lib.csgn_count_terms(65, 1, 5) == 3609714217008132870 == count_terms(65, 1, 5)
    assert lib.csgn_count_terms(66, 1, 5) == 0 == count_terms(66, 1, 5)
    assert lib.csgn_count_terms(65, 2, 5) == 0 == count_terms(65, 2, 5)
    assert lib.csgn_count_terms(LIMIT - 1, 1, 0) == LIMIT - 1 and lib.csgn_count_terms(LIMIT, 1, 0) == 0
    assert lib.csgn_count_terms((1 << 64) - 1, 1, 1) == 0 == count_terms((1 << 64) - 1, 1, 1)
    assert lib.csgn_count_terms(1 << 31, 1, 1) == comb(1 << 31, 2) == count_terms(1 << 31, 1, 1)


def test_dispatch_names(lib, knobs):
    from csgn_amd import capi
    names = capi.tuning_names()
    assert "count_form" in names and "count_cpart" in names
    assert names.index("count_form") < names.index("count_cpart") < names.index("launch_blocks")
    knobs.unset("count_form")
    assert capi.get_tuning("count_form") == -1 and capi.get_tuning("count_cpart") == 0

    def name(n=1247, count=4, g=8, t=1, n_in=1, js=(1, 2)):
        return lib.csgn_count_kernel(n, count, g, t, n_in, len(js), js_array(js)).decode()

    bench = [dict(count=c, g=g, js=js) for c in (1, 256, 4096) for g in (64, 32) for js in ((1,), (1, 2))]
    bench += [dict(count=256, g=8, t=3), dict(n=4096, count=256, g=64, js=(1,))]
    for value, want in [(-1, "k_count"), (0, "composed"), (1, "k_count")]:        # per shape: fused
        knobs.set("count_form", value)
        assert capi.get_tuning("count_form") == value
        for shape in bench:
            assert name(**shape) == want, (value, shape)
        assert name() == want and name(n_in=8) == want and name(g=64, n_in=64, js=(0, 1, 6)) == want
        # every invalid argument, whatever the knob says
        for bad in [dict(n=0), dict(count=0), dict(g=0), dict(t=0), dict(t=LIMIT), dict(n_in=0), dict(n_in=2), dict(js=()),
                    dict(g=65, n_in=65), dict(js=(2, 1)), dict(js=(1, 1)), dict(js=(4,)), dict(js=(7,)), dict(g=3, js=(2,)),
                    dict(g=66, js=(5,)), dict(t=1 << 31, js=(1,))]:
            assert name(**bad) == "", (value, bad)
    assert lib.csgn_count_kernel(1247, 4, 8, 1, 1, 1, None) == b""
    # 2^32 inputs or more are past the gather launcher: fused whatever the knob says
    knobs.set("count_form", 0)
    assert name(count=1 << 26, g=64, js=(1,)) == "k_count"
    assert name(count=(1 << 26) - 1, g=64, js=(1,)) == "composed"


def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails: n_bits; count, group, t, n_in, n_out, the planes and the host
    pointers (INVALID); 2^31 words per element and 2^60 per plane (UNSUPPORTED, computed without wrap-around); null
    device pointers (INVALID); and only then the device (NO_DEVICE on a box without one; with one, the calls that pass
    every check are not made: their pointers are not device memory)."""
    import torch
    gpu = torch.cuda.is_available()
    buf = np.zeros(8, dtype=np.uint64)
    p = buf.ctypes.data

    def ptrs(n, null_at=None):
        return (C.c_void_p * max(n, 1))(*[None if i == null_at else p for i in range(max(n, 1))])

    def cnt(n=1247, count=2, g=8, t=1, n_in=1, js=(1, 2), ins=0, outs=0, h_js=0, null_in=None, null_out=None):
        h_in = ptrs(n_in if 0 < n_in <= 64 else 1, null_in) if ins == 0 else ins
        h_out = ptrs(len(js), null_out) if outs == 0 else outs
        return lib.csgn_count(n, count, g, t, h_in, n_in, len(js), js_array(js) if h_js == 0 else h_js, h_out, None)

    # each failing check wins over every later one
    assert cnt(n=0, count=0, null_in=0) == INVALID                     # n_bits
    assert b"n_bits" in lib.csgn_last_error()
    assert cnt(n=131073, count=0) == UNSUPPORTED
    for bad in [dict(count=0), dict(g=0), dict(t=0), dict(t=LIMIT), dict(t=(1 << 64) - 1), dict(n_in=0), dict(n_in=3),
                dict(g=65, n_in=65), dict(g=1, n_in=1, js=(1,)), dict(js=()), dict(js=(2, 1)), dict(js=(1, 1)),
                dict(js=(4,)), dict(js=(7,)), dict(js=(64,)), dict(ins=None), dict(outs=None), dict(h_js=None)]:
        # ... over the sizes (g = 66 at plane 5 is past 2^62 terms) and the device pointers
        assert cnt(**dict(dict(null_in=0, null_out=0), **bad)) == INVALID, bad
    assert cnt(g=66, js=(2, 1, 5), null_in=0) == INVALID
    # sizes, before the device pointers: 2^31 words per element ...
    dl = 20
    assert cnt(g=64, js=(1, 3), null_in=0) == UNSUPPORTED              # C(64, 8) * 20 words
    assert b"per element" in lib.csgn_last_error()
    assert cnt(g=66, js=(5,), null_out=0) == UNSUPPORTED               # C(66, 32) is past 2^62
    assert cnt(g=65, js=(5,), n=64, null_out=0) == UNSUPPORTED         # C(65, 32) is not, but past 2^31
    assert cnt(g=2, t=LIMIT - 1, js=(0,), null_in=0) == UNSUPPORTED
    assert cnt(g=2, t=1 << 31, js=(1,), n=64, null_in=0) == UNSUPPORTED            # t^2 = 2^62
    assert cnt(g=8, t=1 << 16, js=(2,), n=64, null_in=0) == UNSUPPORTED            # t^4 wraps to 0
    edge = (1 << 31) // dl                                             # g * dL >= 2^31 from here on
    assert cnt(g=edge + 1, js=(0,), null_in=0) == UNSUPPORTED
    assert cnt(g=65537, js=(1,), n=64, null_in=0) == UNSUPPORTED       # C(65537, 2) = 2^31 + 32768
    # ... and 2^60 words per plane
    assert cnt(count=1 << 56, g=2, js=(0, 1), null_in=0) == UNSUPPORTED            # 2^56 * 2 * 20
    assert b"size overflows" in lib.csgn_last_error()
    assert cnt(count=1 << 59, g=2, js=(0,), n=64, null_in=0) == UNSUPPORTED        # 2^60 exactly
    assert cnt(count=1 << 63, g=2, js=(0,), n=64, null_in=0) == UNSUPPORTED        # count * T wraps to 0
    # null device pointers, before the device
    assert cnt(null_in=0) == INVALID
    assert b"null device pointer" in lib.csgn_last_error()
    assert cnt(null_out=1) == INVALID and cnt(n_in=8, null_in=7) == INVALID
    assert cnt(count=1 << 58, g=2, js=(0,), n=64, null_in=0) == INVALID            # 2^59 words pass the size check
    assert cnt(g=edge, js=(0,), null_out=0) == INVALID                             # as does the last size below 2^31
    assert cnt(g=65536, js=(1,), n=64, null_out=0) == INVALID                      # C(65536, 2) = 2^31 - 32768
    if gpu:
        return
    # no device: every call that passes the checks above
    assert cnt() == NO_DEVICE
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert cnt(n_in=8) == NO_DEVICE and cnt(g=64, n_in=64, js=(0, 1, 6)) == NO_DEVICE and cnt(g=65, js=(1, 6)) == NO_DEVICE
    assert cnt(g=edge, js=(0,)) == NO_DEVICE and cnt(g=65536, js=(1,), n=64) == NO_DEVICE


# -- the definition against the oracle and the genuine reference -----------------------------------------------------
SHAPES = [(1, 3, [0]), (3, 2, [0, 1]), (5, 2, [0, 1, 2]), (8, 1, [0, 1, 2, 3]), (6, 3, [1, 2])]
SHAPE_IDS = ["g%d_t%d_%s" % (g, t, "".join(map(str, js))) for g, t, js in SHAPES]


def check_definition(ops, n, g, t, js):
    count = 2
    x = rand_terms(n, count * g, t, 1000 * n + 10 * g + t)
    words = np_count(x, g, js)
    planes = np_count([np.ascontiguousarray(x.reshape(count, g, t, -1)[:, i]) for i in range(g)], g, js, "planes")
    dl = (n + 63) // 64
    for j, w, wp in zip(js, words, planes):
        assert w.shape == (count, count_terms(g, t, j), dl), j
        assert np.array_equal(w, wp), j                               # both layouts: the same words
        for q in range(count):
            got = compose_count(ops, [x[q * g + i].ravel() for i in range(g)], j)
            assert got.size == w[q].size and np.array_equal(w[q].ravel(), got), (j, q)


@pytest.mark.parametrize("n", [63, 129])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_decode_is_the_composition_by_the_oracle(oracle, n, shape):
    check_definition(oracle_ops(oracle, n), n, *shape)


@pytest.mark.parametrize("n,d", [(63, 4), (129, 8)])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_decode_is_the_composition_by_the_reference(ref, n, d, shape):
    check_definition(ref_ops(ref, n, d), n, *shape)


# -- decryptions -------------------------------------------------------------------------------------------------------
def encrypt_bits(oracle, n, key, bits, seed):
    flat = np.asarray(bits, dtype=np.uint8).ravel()
    dl = (n + 63) // 64
    return oracle.encrypt_seq(n, key, flat, glibc_draws(seed, flat.size * (n + 2)))[0].reshape(flat.size, 1, dl)


@pytest.mark.parametrize("g,js", [(5, [0, 1, 2]), (12, [0, 1, 2, 3])], ids=["g5_all_patterns", "g12_random"])
def test_planes_decrypt_to_the_popcount(oracle, g, js):
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(600 + g, 64 * d + 64))
    if g == 5:
        values = np.arange(32, dtype=np.uint64)
    else:
        values = np.random.default_rng(12).integers(0, 1 << 12, 20).astype(np.uint64)
        values[:2] = [0, (1 << 12) - 1]
    bits = ((values[:, None] >> np.arange(g, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)   # [count, g]
    x = encrypt_bits(oracle, n, key, bits, 610 + g)
    outs = np_count(x, g, js)
    got = np.zeros(len(values), dtype=np.uint64)
    for j, w in zip(js, outs):
        got |= decrypt_bits(oracle, n, key, w).astype(np.uint64) << np.uint64(j)
    assert np.array_equal(got, popcount_planes(values, len(js)))
