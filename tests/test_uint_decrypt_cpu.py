"""csgn_uint_decrypt (one-bit batches decrypted into one word per element in one pass) on a box without a GPU: the model
the device tests compare with (tests/model_uint_decrypt.py) against the oracle, the argument checks and their order,
the names of the two forms, the knobs and the exported symbols.  The device side is tests/test_uint_decrypt_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests.model import decrypt_value, lib, u64s  # noqa: F401  (lib: fixture)
from tests.model_uint_decrypt import CHUNK_BY_SHAPE, LONG, SUM8, Planes, has_both_bits, packed, salts

INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -3


# -- the model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1247])
def test_packed_is_the_oracles_decryption(oracle, n):
    """Planes of 1 to 5 terms an element, uniform and ragged (with empty elements): packed() is the oracle's decryption
    of every element, bit by bit, and every plane of the inputs holds both bits."""
    batch = 7
    ragged = [0, 3, 1, 5, 0, 2, 0]
    c = Planes(n, batch, [1, 2, 3, 4, 5, ragged])
    assert has_both_bits([c])
    dl = c.tab.dl
    uniform = [w.reshape(batch, t, dl) for w, t in zip(c.words[:5], c.terms[:5])]
    assert np.array_equal(decrypt_value(oracle, n, c.key, uniform), c.want & np.uint64(31))
    off = c.offs[5].astype(np.int64)
    for e in range(batch):
        words = c.words[5][off[e]:off[e + 1]].ravel()
        bit = oracle.decrypt_canonical(n, c.key, words) if words.size else 0
        assert int(bit) == int(c.want[e] >> np.uint64(5)), e
    assert np.array_equal(packed(n, c.key, c.words, c.offs), c.want) and not (c.want >> np.uint64(6)).any()


@pytest.mark.parametrize("batch", [1, 3])
def test_small_batches_hold_both_bits(batch):
    cases = [Planes(64, batch, list(SUM8), salt=s) for s in salts(batch)]
    assert has_both_bits(cases)


# -- the argument checks -----------------------------------------------------------------------------------------------
def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails: n_bits; n_planes and the batch; the host pointers; what a ragged
    plane needs (INVALID); 2^31 words per element and 2^60 per batch (UNSUPPORTED); a ragged bound above 4096
    (UNSUPPORTED); the device (NO_DEVICE on a box without one); null device pointers (INVALID, with a device only)."""
    import torch
    gpu = torch.cuda.is_available()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    ptrs = (C.c_void_p * 65)(*([p] * 65))
    nullp = (C.c_void_p * 65)(*([p] * 3 + [None] + [p] * 61))
    one = u64s([1] * 65)
    rag3 = u64s([1, 1, 1, 0] + [1] * 61)            # plane 3 is ragged
    zeros = u64s([0] * 65)

    def dec(n=1247, batch=4, w=8, planes=ptrs, terms=one, offs=ptrs, totals=zeros, bounds=zeros, mask=p, values=p):
        return lib.csgn_uint_decrypt(n, batch, w, planes, terms, offs, totals, bounds, mask, values, None)

    # each failing check wins over every later one
    assert dec(n=0, w=0, planes=None) == INVALID and dec(n=131073, w=0) == UNSUPPORTED          # 1. n_bits
    assert dec(w=0, planes=None) == INVALID and dec(w=65, terms=None) == INVALID                # 2. planes, batch
    assert b"planes" in lib.csgn_last_error()
    assert dec(batch=0, planes=None) == INVALID and b"batch" in lib.csgn_last_error()
    for arg in ("planes", "terms"):                                                            # 3. host pointers
        assert dec(**{arg: None}) == INVALID and b"null host pointer" in lib.csgn_last_error(), arg
    assert dec(planes=None, terms=rag3, offs=None) == INVALID
    for arg in ("offs", "totals", "bounds"):                                                   # 4. a ragged plane
        assert dec(terms=rag3, **{arg: None}) == INVALID and b"ragged" in lib.csgn_last_error(), arg
        assert gpu or dec(w=3, terms=rag3, **{arg: None}) == NO_DEVICE                         # ... only where there is one
    big = u64s([1] * 3 + [1 << 40] + [1] * 61)
    assert dec(terms=rag3, totals=u64s([0, 0, 0, 41]), bounds=u64s([0, 0, 0, 10])) == INVALID   # 4 * 10 < 41
    assert b"max_terms" in lib.csgn_last_error()
    # (a product batch * max_terms that would wrap is not "too small": the sizes refuse it next)
    assert dec(terms=rag3, totals=u64s([0, 0, 0, 41]), bounds=u64s([0, 0, 0, 10]), batch=1 << 62) == UNSUPPORTED
    assert dec(terms=rag3, totals=big, bounds=u64s([0, 0, 0, 10]), planes=nullp) == INVALID     # before the sizes
    # 5. sizes: 2^31 words an element, 2^60 a batch -- before the ragged bound and before the pointers
    assert dec(terms=u64s([1, 1 << 27]), w=2, planes=nullp) == UNSUPPORTED
    assert b"per element" in lib.csgn_last_error()
    assert dec(batch=1 << 56, planes=nullp) == UNSUPPORTED and b"batch" in lib.csgn_last_error()
    assert dec(terms=rag3, totals=u64s([0, 0, 0, 1 << 57]), bounds=u64s([0, 0, 0, 1 << 20]), batch=1 << 40) == UNSUPPORTED
    assert dec(terms=rag3, totals=u64s([0, 0, 0, 8]), bounds=u64s([0, 0, 0, 1 << 27])) == UNSUPPORTED
    assert b"per element" in lib.csgn_last_error()
    # 6. the ragged bound
    assert dec(terms=rag3, totals=u64s([0, 0, 0, 8]), bounds=u64s([0, 0, 0, LONG + 1]), planes=nullp) == UNSUPPORTED
    assert b"ragged plane 3" in lib.csgn_last_error()
    if gpu:
        return
    # 7. no device: every call that passes the checks above, null device pointers (check 8) included
    assert dec() == NO_DEVICE and b"no CPU fallback" in lib.csgn_last_error()
    assert dec(w=1) == NO_DEVICE and dec(w=64) == NO_DEVICE and dec(batch=1) == NO_DEVICE
    assert dec(terms=rag3, totals=u64s([0, 0, 0, 8]), bounds=u64s([0, 0, 0, LONG])) == NO_DEVICE
    assert dec(terms=rag3, totals=u64s([0, 0, 0, 8]), bounds=u64s([0, 0, 0, 2])) == NO_DEVICE      # a tight bound
    assert dec(planes=nullp) == NO_DEVICE and dec(mask=None) == NO_DEVICE and dec(values=None) == NO_DEVICE
    assert dec(offs=None, totals=None, bounds=None) == NO_DEVICE                                # no ragged plane


def test_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        return                                                        # the device tests make the calls
    buf = np.zeros(64, dtype=np.uint64)
    ptrs = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    assert lib.csgn_uint_decrypt(1247, 1, 2, ptrs, u64s([1, 1]), None, None, None, buf.ctypes.data, buf.ctypes.data,
                                 None) == NO_DEVICE
    assert b"no CPU fallback" in lib.csgn_last_error()


# -- the forms and the knobs -------------------------------------------------------------------------------------------
def test_form_names(lib, knobs):
    OWNED, CUT = b"k_uint_decrypt", b"k_zero_words+k_uint_decrypt"

    def name(terms, n=1247, batch=256, w=None):
        return lib.csgn_uint_decrypt_kernel(n, batch, len(terms) if w is None else w, u64s(terms))

    knobs.unset("uint_decrypt_chunk")
    for batch in (1, 256, 1 << 20):
        assert name([1] * 8, batch=batch) == OWNED and name([1] * 64, batch=batch) == OWNED       # fresh planes
        assert name([1, 2, 5, 129], batch=batch) == OWNED and name(list(SUM8), batch=batch) == OWNED
        assert name([1, 0, 129], batch=batch) == OWNED                                            # a ragged plane is never cut
        assert name([1, CHUNK_BY_SHAPE, 1], batch=batch) == OWNED
        assert name([1, CHUNK_BY_SHAPE + 1, 1], batch=batch) == CUT
    for chunk, terms, want in ((1, [1] * 8, OWNED), (1, [1, 2, 1], CUT), (7, [7, 1, 7], OWNED), (7, [1, 2, 5, 129], CUT),
                               (256, [1, 2, 5, 129], OWNED), (256, [257], CUT), (LONG, [LONG], OWNED),
                               (1 << 20, [LONG + 1], CUT)):                                       # never above 4096
        knobs.set("uint_decrypt_chunk", chunk)
        assert name(terms) == want, (chunk, terms)
    assert name([1], n=0) == b"" and name([1], batch=0) == b"" and name([1], w=0) == b"" and name([1] * 65) == b""
    assert lib.csgn_uint_decrypt_kernel(1247, 4, 2, None) == b""
    knobs.set("uint_decrypt_form", 0)                                 # the classes' knob: the C call is always the kernel
    knobs.unset("uint_decrypt_chunk")
    assert name([1] * 8) == OWNED


def test_knobs():
    from csgn_amd import capi
    names = capi.tuning_names()
    assert names[-1] == "launch_blocks" and names[-2] == "uint_arith_form"
    for knob, default in (("uint_decrypt_form", -1), ("uint_decrypt_chunk", 0)):
        assert knob in names and names.index(knob) < names.index("uint_arith_form")
        assert not knob.endswith("_fused")
    import os
    if "CSGN_UINT_DECRYPT_FORM" not in os.environ:
        assert capi.get_tuning("uint_decrypt_form") == -1
    if "CSGN_UINT_DECRYPT_CHUNK" not in os.environ:
        assert capi.get_tuning("uint_decrypt_chunk") == 0


def test_symbols(lib):
    from csgn_amd import capi
    for name in ("csgn_uint_decrypt", "csgn_uint_decrypt_kernel"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == capi.SIGNATURES[name][1]
    from csgn_amd.batch import HipPath
    assert callable(HipPath.uint_decrypt)
