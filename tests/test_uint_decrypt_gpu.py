"""csgn_uint_decrypt on the device, word for word against the definition (tests/model_uint_decrypt.py: packed(), every bit
model_decrypt.np_bits): near misses at every key position, hits at the first and last term of an element and on each
side of every pass, group and chunk boundary.  The C ABI is called directly: d_values starts as 0xFF.. between guard
words that must stay untouched, so "never written" and "written beside" both show.  Every case runs under knob
uint_decrypt_chunk at 1, 7, 256 and 0 (where the cut falls) and under a launch_blocks that splits the launch, and is
compared with csgn_decrypt_uniform / csgn_decrypt_ragged_bounded plane by plane on the same buffers.
Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

from csgn_amd.capi import check
from tests.model import hip, u64s  # noqa: F401  (hip: fixture)
from tests.model_decrypt import np_key_mask
from tests.model_uint_decrypt import CHUNKS, LONG, SUM8, Planes, has_both_bits, salts

pytestmark = pytest.mark.gpu

GUARD = 8                                           # words either side of the values
FILL = np.uint64(0xFFFFFFFFFFFFFFFF)
UNSUPPORTED = -2

VECTORS = {"one": [1], "fresh64": [1] * 64, "sum8": list(SUM8), "long": [1, 1300, 1], "mid": [2, 4, 9]}


def place(hip, a, moved):
    """Device copy of the words `a`; moved: it starts one word (8 bytes) into its buffer."""
    a = np.ascontiguousarray(a, dtype=np.uint64).ravel()
    t = hip.upload(np.concatenate([np.zeros(1, np.uint64), a, np.zeros(1, np.uint64)]))[1:-1] if moved else hip.upload(
        np.concatenate([a, np.zeros(2, np.uint64)]))[:a.size]
    assert t.data_ptr() % 16 == (8 if moved else 0)
    return t


class Device:
    """One case's planes, offsets and mask on the device, and the calls that decrypt them."""

    def __init__(self, hip, case, moved=False):
        self.hip, self.lib, self.c = hip, hip.lib, case
        mask = hip.key_mask(case.n, case.key)
        assert np.array_equal(mask, np_key_mask(case.n, case.key))
        self.mask = place(hip, mask, moved)
        self.planes = [place(hip, w, moved) for w in case.words]
        self.offs = [None if t else hip.upload(np.asarray(o, dtype=np.uint64)) for t, o in zip(case.terms, case.offs)]
        self.moved = moved

    def status(self, bounds=None, values_moved=False):
        """(status, the words, the guards are untouched) of one csgn_uint_decrypt."""
        c, w = self.c, len(self.c.terms)
        lead = GUARD + (1 if values_moved else 0)   # a fresh tensor is 16-byte aligned; GUARD is even
        buf = torch.from_numpy(np.full(lead + c.batch + GUARD, FILL, dtype=np.uint64).view(np.int64)).to(self.hip.device)
        assert buf[lead:].data_ptr() % 16 == (8 if values_moved else 0)
        bounds = c.bounds if bounds is None else bounds
        h_planes = (C.c_void_p * w)(*[p.data_ptr() for p in self.planes])
        h_offs = (C.c_void_p * w)(*[None if o is None else o.data_ptr() for o in self.offs])
        totals = u64s([0 if t else int(o[-1]) for t, o in zip(c.terms, c.offs)])
        rc = self.lib.csgn_uint_decrypt(c.n, c.batch, w, h_planes, u64s(c.terms), h_offs, totals, u64s(bounds),
                                        self.mask.data_ptr(), buf[lead:].data_ptr(), self.hip.stream)
        h = self.hip.download(buf)
        assert (h[:lead] == FILL).all() and (h[lead + c.batch:] == FILL).all(), "words beside the values were written"
        return rc, h[lead:lead + c.batch]

    def packed(self, **kw):
        rc, v = self.status(**kw)
        check(rc)
        return v

    def per_plane(self):
        """The same buffers through csgn_decrypt_uniform / csgn_decrypt_ragged_bounded, plane by plane."""
        c = self.c
        v = np.zeros(c.batch, dtype=np.uint64)
        for j, (p, t) in enumerate(zip(self.planes, c.terms)):
            if t:
                bits = self.hip.decrypt_uniform(c.n, c.batch, t, p, self.mask)
            else:
                bits = self.hip.decrypt_ragged(c.n, p, self.offs[j], self.mask, int(c.offs[j][-1]), c.bounds[j])
            v |= self.hip.download(bits).astype(np.uint64) << np.uint64(j)
        return v


def same(got, want, what):
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, (what, "%d of %d words wrong" % (wrong.size, want.size),
                             "%d never written" % int((got == FILL).sum()), "first at", wrong[:6].tolist(),
                             [hex(int(x)) for x in got[wrong[:6]]], [hex(int(x)) for x in want[wrong[:6]]])


def run_settings(knobs, dev, want, what, chunks=CHUNKS):
    """The call under every chunk setting, split into several launches at two of them: the model's words each time."""
    lib = dev.lib
    for chunk in chunks:
        knobs.set("uint_decrypt_chunk", chunk)
        knobs.set("launch_blocks", 0)
        whole = dev.packed()
        same(whole, want, what + (chunk, "one launch"))
        cut = any(t > (chunk or 1024) for t in dev.c.terms)
        name = lib.csgn_uint_decrypt_kernel(dev.c.n, dev.c.batch, len(dev.c.terms), u64s(dev.c.terms))
        assert name == (b"k_zero_words+k_uint_decrypt" if cut else b"k_uint_decrypt")
        if chunk in (0, 7):
            knobs.set("launch_blocks", 5 if dev.c.batch > 3 or cut else 1)
            same(dev.packed(), whole, what + (chunk, "split"))
    knobs.set("launch_blocks", 0)
    knobs.set("uint_decrypt_chunk", 0)


@pytest.mark.parametrize("vector", list(VECTORS))
@pytest.mark.parametrize("batch", [1, 3, 257])
@pytest.mark.parametrize("n", [64, 1247, 1300, 4096])
def test_words_under_every_setting(hip, knobs, n, batch, vector):
    """N = 64, 1247, 1300 (odd dL: 8-byte units) and 4096; batch 1, 3 and 257; one plane, 64 fresh planes, the planes of
    an 8-bit sum, a plane of 1300 terms beside fresh ones (and 2, 4 and 9 terms: several elements a wave)."""
    cases = [Planes(n, batch, VECTORS[vector], salt=s) for s in salts(batch)]
    assert has_both_bits(cases)                     # a 0 and a 1 in every plane
    for c in cases:
        dev = Device(hip, c)
        run_settings(knobs, dev, c.want, (n, batch, vector))
        same(dev.per_plane(), c.want, (n, batch, vector, "plane by plane"))


RAGGED = {
    # empty elements in front, in the middle and at the end; one element at the bound
    "wide": lambda batch: [0, 0] + [(7 * e) % 131 for e in range(2, batch // 2)] + [0, 130, 0] +
                          [(5 * e + 1) % 64 for e in range(batch // 2 + 3, batch - 1)] + [0],
    # a few terms an element: many elements a wave
    "narrow": lambda batch: [0] + [(e * e) % 4 for e in range(1, batch - 1)] + [0],
}


@pytest.mark.parametrize("shape,batch", [("wide", 67), ("narrow", 300)])
@pytest.mark.parametrize("n", [64, 1247, 1300])
def test_ragged_planes(hip, knobs, n, shape, batch):
    """Ragged planes (what compact() returns) beside uniform ones, under a tight and a loose bound; a bound above 4096 is
    refused and leaves the words alone."""
    counts = RAGGED[shape](batch)
    other = [(c + 3) % (max(counts) + 1) for c in reversed(counts)]
    assert len(counts) == batch and counts[0] == 0 and counts[-1] == 0 and 0 in counts[2:-2]
    c = Planes(n, batch, [counts, 1, other, 5])
    assert has_both_bits([c]) and c.bounds[0] == max(counts)
    dev = Device(hip, c)
    run_settings(knobs, dev, c.want, (n, shape), chunks=(0, 1))
    same(dev.packed(bounds=[b + 17 if b else 0 for b in c.bounds]), c.want, (n, shape, "loose bound"))
    same(dev.packed(bounds=[LONG if b else 0 for b in c.bounds]), c.want, (n, shape, "bound 4096"))
    same(dev.per_plane(), c.want, (n, shape, "plane by plane"))
    rc, v = dev.status(bounds=[LONG + 1, 0, c.bounds[2], 0])
    assert rc == UNSUPPORTED and (v == FILL).all()


@pytest.mark.parametrize("vector", ["fresh64", "sum8", "long"])
@pytest.mark.parametrize("n", [64, 1247, 4096])
def test_misaligned_pointers(hip, knobs, n, vector):
    """Plane pointers and the mask at 8 mod 16 with an even dL (N = 1247, 4096: the 8-byte units run), and d_values at
    8 mod 16."""
    c = Planes(n, 131, VECTORS[vector])
    assert has_both_bits([c])
    for moved in (False, True):
        dev = Device(hip, c, moved)
        for chunk in (0, 7):
            knobs.set("uint_decrypt_chunk", chunk)
            same(dev.packed(values_moved=True), c.want, (n, vector, moved, chunk, "values at 8 mod 16"))
            same(dev.packed(), c.want, (n, vector, moved, chunk))
    knobs.set("uint_decrypt_chunk", 0)


def test_wrapper(hip):
    """HipPath.uint_decrypt: uniform and ragged planes through the Python wrapper."""
    counts = [0, 3, 1, 0, 9, 2, 0]
    c = Planes(1247, 7, [1, counts, 3])
    dev = Device(hip, c)
    got = hip.uint_decrypt(c.n, c.batch, dev.planes, c.terms, dev.mask, offsets=dev.offs, max_terms=c.bounds)
    same(hip.download(got), c.want, "wrapper")
    u = Planes(1247, 5, [1, 2])
    dev = Device(hip, u)
    same(hip.download(hip.uint_decrypt(u.n, u.batch, dev.planes, u.terms, dev.mask)), u.want, "wrapper, uniform")
