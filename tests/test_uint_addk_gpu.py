"""A bit-sliced integer plus a public constant on the device (csgn_uint_addk), word for word against the definition of
include/csgn_hip.h (pinned against the reference and the oracle in tests/test_uint_addk_cpu.py), in all three settings
of the knob uint_addk_fused.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from tests.model import GuardedOutputs, hip, rand_terms, u64s
from tests.model_addk import addk_terms, full_width_ks, np_addk, term_modes
from tests.test_uint_plain_gpu import edge_ks

pytestmark = pytest.mark.gpu


def run(hip, n, planes, k, negate, carry, offset=0, want=None):
    """The outputs (and carry-out) downloaded; offset = 1 places every plane and output one word past a 16-byte
    boundary.  With `want` (the definition's planes and, last, its carry-out) the outputs are caller tensors of exactly
    those sizes between guard words, checked word for word and for writes outside them (tests/model.py,
    GuardedOutputs)."""
    batch = planes[0].shape[0]
    ts = [p.shape[1] for p in planes]

    def place(words):
        if not offset:
            return hip.upload(words)
        t = hip.empty_words(words.size + offset)
        t[offset:].copy_(hip.upload(words))
        return t[offset:]

    dev = [place(p.ravel()) for p in planes]
    outs = carry_out = guarded = None
    if want is not None:
        guarded = GuardedOutputs(hip, [x.size for x in (want if carry else want[:-1])], shift=offset)
        outs, carry_out = guarded.outs[:len(ts)], (guarded.outs[-1] if carry else None)
        assert all(o.data_ptr() % 16 == (8 if offset else 0) for o in guarded.outs + dev)
    elif offset:
        dl = (n + 63) // 64
        T = addk_terms(len(ts), k, ts)
        outs = [hip.empty_words(batch * (t + negate) * dl + offset)[offset:] for t in T[:-1]]
        carry_out = hip.empty_words(batch * T[-1] * dl + offset)[offset:]
        assert all(o.data_ptr() % 16 == 8 for o in outs + dev + [carry_out])
    outs, c = hip.uint_addk(n, batch, dev, ts, k, negate=negate, carry=carry, outs=outs, carry_out=carry_out)
    if guarded:
        got = guarded.check(want if carry else want[:-1], (k, negate, carry))
        return got[:len(ts)], (got[-1] if carry else None)
    return [hip.download(o) for o in outs], (hip.download(c) if carry else None)


def check_forms(hip, knobs, n, planes, k, offset=0, carries=(False, True)):
    """Every knob setting, with and without negate_out and the carry-out; returns the number of device calls."""
    calls = 0
    for negate in (False, True):
        want, want_c = np_addk(n, planes, k, negate)
        for fused in (-1, 0, 1):
            knobs.set("uint_addk_fused", fused)
            for carry in carries:
                got, got_c = run(hip, n, planes, k, negate, carry, offset,
                                 want=[x.ravel() for x in want] + [want_c.ravel()])
                tag = (fused, k, negate, carry, [p.shape[1] for p in planes])
                for j, (g, w_) in enumerate(zip(got, want)):
                    assert np.array_equal(g, w_.ravel()), (j,) + tag
                if carry:
                    assert np.array_equal(got_c, want_c.ravel()), ("carry",) + tag
                calls += 1
    return calls


# 63 and 129: odd dL, the 8-byte-unit kernel
@pytest.mark.parametrize("n", [63, 65, 129, 1247, 4096])
@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("tmode", ["1", "2", "3", "mixed"])
def test_addk_words(hip, knobs, n, w, tmode):
    # the largest case (w = 8, every t_j = 3, k = 255): a carry-out of 65 535 terms, about 100 MB at n = 4096
    ts = term_modes(w, tmode, np.random.default_rng(w * 10 + len(tmode)))
    batch = 3
    planes = [rand_terms(n, batch, t, 300 + 7 * j + t) for j, t in enumerate(ts)]
    for k in sorted(set(edge_ks(w)) | {1, (1 << w) - 1}):
        check_forms(hip, knobs, n, planes, k)


def test_addk_words_unaligned(hip, knobs):
    """Planes, outputs and the carry-out 8 bytes past a 16-byte boundary at even dL: the 8-byte units."""
    n, w = 1247, 5
    planes = [rand_terms(n, 3, t, 350 + j) for j, t in enumerate([1, 2, 1, 3, 1])]
    for k in (0, 1, 22, 31):
        check_forms(hip, knobs, n, planes, k, offset=1)


def test_addk_words_full_width(hip, knobs):
    """Levels and planes at and above bit 16, 32 and 63, the carry-out requested.  Over this whole list no plane exceeds
    129 terms and no carry-out 255 (fresh planes), so every case runs: the count is asserted."""
    listed = executed = 0
    for n in (65, 1247):
        for w in (17, 31, 32, 33, 63, 64):
            planes = [rand_terms(n, 2, 1, 4000 + 67 * w + j) for j in range(w)]
            ks = full_width_ks(w)
            assert len(ks) == 5
            for k in ks:
                listed += 1
                counts = addk_terms(w, k, [1] * w)
                assert max(counts[:w]) <= 129 and counts[w] <= 255, (w, k)
                assert check_forms(hip, knobs, n, planes, k, carries=(True,)) == 6
                executed += 1
    assert listed == executed == 2 * 6 * 5


@pytest.mark.parametrize("batch", [1, 2, 255, 257, 4099])
def test_addk_batches(hip, knobs, batch):
    n = 65
    planes = [rand_terms(n, batch, t, 700 + j) for j, t in enumerate([1, 2, 1, 1])]
    for k in (0, 5, 8, 15):
        check_forms(hip, knobs, n, planes, k)


def test_addk_plane_past_4_gib(hip, knobs):
    """One output plane of 5.4 GB (out_1 of a 2-bit a + 1 with 64-term planes, 2^18 elements at N=1247): offsets pass
    2^32 bytes.  The fused form's planes against the composed form's by csgn_digest, nothing downloaded."""
    import torch
    n, batch, ts, k = 1247, 1 << 18, [64, 64], 1
    dl = (n + 63) // 64
    T = addk_terms(2, k, ts)
    assert T[:2] == [65, 128] and batch * T[1] * dl * 8 > 1 << 32
    planes = [hip.synth_fill(900 + j, n, 0, batch * t * dl) for j, t in enumerate(ts)]
    digests = {}
    for fused in (1, 0):
        knobs.set("uint_addk_fused", fused)
        assert hip.lib.csgn_uint_addk_kernel(n, batch, 2, k, u64s(ts), 0).decode() == ("k_uint_addk" if fused else "composed")
        outs, _ = hip.uint_addk(n, batch, planes, ts, k)
        torch.cuda.synchronize()
        digests[fused] = [hip.digest(o) for o in outs]
        # both ends of the large plane against the definition
        for e in (0, batch - 1):
            small = [hip.download(p[e * t * dl:(e + 1) * t * dl]).reshape(1, t, dl) for p, t in zip(planes, ts)]
            want = np_addk(n, small, k)[0][1].ravel()
            assert np.array_equal(hip.download(outs[1][e * T[1] * dl:(e + 1) * T[1] * dl]), want), (fused, e)
        del outs
        torch.cuda.empty_cache()
    assert digests[1] == digests[0]


def test_addk_argument_errors(hip):
    lib = hip.lib
    t = hip.upload(np.zeros(64 * 20, dtype=np.uint64))
    planes = (C.c_void_p * 64)(*([t.data_ptr()] * 64))
    one = u64s([1] * 64)
    assert lib.csgn_uint_addk(1247, 1, 4, 16, 0, planes, one, planes, None, hip.stream) == -1
    assert lib.csgn_uint_addk(1247, 1, 0, 0, 0, planes, one, planes, None, hip.stream) == -1
    assert lib.csgn_uint_addk(1247, 1, 4, 3, 0, planes, u64s([1, 1, 0, 1]), planes, None, hip.stream) == -1
    assert lib.csgn_uint_addk(1247, 1, 4, 3, 0, planes, one, None, None, hip.stream) == -1
    nullp = (C.c_void_p * 4)(t.data_ptr(), None, t.data_ptr(), t.data_ptr())
    assert lib.csgn_uint_addk(1247, 1, 4, 3, 0, nullp, one, planes, None, hip.stream) == -1
    assert lib.csgn_uint_addk(1247, 1, 4, 3, 0, planes, one, nullp, None, hip.stream) == -1
    assert lib.csgn_uint_addk(1247, 1, 29, (1 << 29) - 1, 0, planes, one, planes, None, hip.stream) == -2
    assert lib.csgn_uint_addk(1247, 1, 27, (1 << 27) - 1, 0, planes, one, planes, t.data_ptr(), hip.stream) == -2   # the carry-out alone
    assert lib.csgn_uint_addk(1247, 1 << 56, 8, 1, 0, planes, one, planes, None, hip.stream) == -2                 # batch
    assert lib.csgn_uint_addk(1247, 0, 4, 3, 1, planes, one, planes, None, hip.stream) == 0      # empty batch
