"""Decrypt on inputs that see every key position and every edge of pass 2 (tests/model_decrypt.py; the conditions on
the inputs themselves are checked in tests/test_decrypt_cpu.py).

The older decrypt tests plant hits with tests/model.py: planted(), whose non-hits lack key[0] only: a pass 1 that drops a
lane of the 16-byte compare, reads the wrong mask unit in one pass of the segment form or skips a term's last unit still
gives every bit they expect.  Here every non-hit is a NEAR MISS -- all key bits but one --, the missing position rotates
against the slots of a workgroup, and hits sit at the first and last term of a ciphertext, at both ends of a bitmap
word and on either side of the 65 536-term chunk edges.  Every expected bit is np_decrypt's, the definition bit by bit.
The C ABI is called directly: the bits start as 7 and the scratch block as random bytes, so "never written" shows.

The contexts run every pass-1 instantiation the host rule can reach (K = 1, 2, 3, 5, 7 and the looping form), each at
both unit widths where dL is even: model_decrypt.CONTEXTS, asserted against a copy of the rule in test_decrypt_cpu.py.
Run with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

from csgn_amd.capi import check
from oracle.binding import canonical_bitlen
from tests.model import hip, np_add, np_mul  # noqa: F401  (hip: fixture)
from tests.model_decrypt import (CONTEXTS, FILLS, FUSED_SHAPES, LONG, LONG_T, RAGGED_COUNTS, RAGGED_RUNS, Table,
                                 boundary_positions, every_position, forms, fused_operands, long_ragged, long_uniform,
                                 near_misses, np_bits, np_decrypt, np_key_mask, pass1_form, regroup, slot_list,
                                 slot_rotations, with_empties)

pytestmark = pytest.mark.gpu

GUARD = 16                                          # bytes of 7 either side of the bits


def place(hip, a, moved):
    """Device copy of the words `a`; moved: it starts one word (8 bytes) into its buffer, so the 8-byte units run."""
    a = np.ascontiguousarray(a, dtype=np.uint64).ravel()
    t = hip.upload(np.concatenate([np.zeros(1, np.uint64), a]))[1:] if moved else hip.upload(a)
    assert t.data_ptr() % 16 == (8 if moved else 0)
    return t


class Device:
    """The words and the mask of one case on the device, and the calls that decrypt them."""

    def __init__(self, hip, case, moved=False):
        self.hip, self.lib, self.n = hip, hip.lib, case.n
        mask = hip.key_mask(case.n, case.key)
        assert np.array_equal(mask, np_key_mask(case.n, case.key))
        self.words, self.mask = place(hip, case.words, moved), place(hip, mask, moved)
        self.total = case.words.shape[0]

    def call(self, batch, fn):
        nbytes = int(self.lib.csgn_decrypt_scratch_bytes(batch, self.total))
        scratch = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device=self.hip.device)
        bits = torch.full((batch + 2 * GUARD,), 7, dtype=torch.uint8, device=self.hip.device)
        fn(bits[GUARD:].data_ptr(), scratch.data_ptr())
        h = self.hip.download(bits)
        assert (h[:GUARD] == 7).all() and (h[GUARD + batch:] == 7).all(), "bytes outside the bits were written"
        return h[GUARD:GUARD + batch]

    def uniform(self, batch, T):
        assert batch * T == self.total
        return self.call(batch, lambda b, s: check(self.lib.csgn_decrypt_uniform(
            self.n, batch, T, self.words.data_ptr(), self.mask.data_ptr(), b, s, self.hip.stream)))

    def ragged(self, off, bound=None):
        batch = len(off) - 1
        assert int(off[-1]) == self.total
        doff = self.hip.upload(np.asarray(off, dtype=np.uint64))
        if bound is None:
            return self.call(batch, lambda b, s: check(self.lib.csgn_decrypt_ragged(
                self.n, batch, self.total, self.words.data_ptr(), doff.data_ptr(), self.mask.data_ptr(), b, s,
                self.hip.stream)))
        return self.call(batch, lambda b, s: check(self.lib.csgn_decrypt_ragged_bounded(
            self.n, batch, self.total, bound, self.words.data_ptr(), doff.data_ptr(), self.mask.data_ptr(), b, s,
            self.hip.stream)))


def same(got, want, what):
    assert got.shape == want.shape, what
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, (what, "%d of %d bits wrong" % (wrong.size, want.size),
                             "%d never written" % int((got == 7).sum()), "first at", wrong[:8].tolist(),
                             got[wrong[:8]].tolist())


# ---------------------------------------------------------------------- a. every key position, every slot of pass 1

@pytest.mark.parametrize("n,d", list(CONTEXTS))
@pytest.mark.parametrize("loop", [0, 1])
def test_every_key_position_in_every_slot(hip, knobs, n, d, loop):
    """M >= 515 one-term ciphertexts (two full workgroups of the widest form and a tail of three), term p a near miss on
    position (p + p // d + r) % d, every 37th a hit; the rotations r are those after which every position has been
    missed in every pass of a segment workgroup and in the tail workgroup.  Four ways through the library: uniform
    single terms (the segment form writes the bits itself), CSR (bitmap + lane-per-ciphertext pass 2), CSR with the bound
    1 (the uniform kernels) and uniform ciphertexts of 3 terms."""
    knobs.set("CSGN_DEC_LOOP", loop)
    tab = Table(n, d)
    for moved, form in forms(n):
        assert form == CONTEXTS[(n, d)][1 if moved else 0] == pass1_form(n, moved)
        for r in slot_rotations(tab):
            c = slot_list(tab, r)
            want = c.want()
            assert 0 < want.sum() < c.batch
            dev = Device(hip, c, moved)
            same(dev.uniform(c.batch, 1), want, (n, loop, moved, r, "uniform T=1"))
            same(dev.ragged(c.off), want, (n, loop, moved, r, "ragged"))
            same(dev.ragged(c.off, bound=1), want, (n, loop, moved, r, "ragged, bound 1"))
            c3 = regroup(c, 3)
            same(Device(hip, c3, moved).uniform(c3.batch, 3), c3.want(), (n, loop, moved, r, "uniform T=3"))


# ---------------------------------------------------------------------- b. one hit at every position of a ciphertext

@pytest.mark.parametrize("n,d", [(63, 4), (1247, 16), (4096, 32)])
@pytest.mark.parametrize("loop", [0, 1])
def test_one_hit_at_every_position(hip, knobs, n, d, loop):
    """130 ciphertexts of 130 near misses, the hit of ciphertext b at term b: bit offsets 130 * b + b walk through every
    bit of a bitmap word, first and last term included.  No hit and two hits give 0.  The same words as a CSR batch
    with three empty ciphertexts (first, middle, last)."""
    knobs.set("CSGN_DEC_LOOP", loop)
    tab = Table(n, d)
    for hits in (0, 1, 2):
        c = every_position(tab, hits)
        want = c.want()
        assert (want == (hits == 1)).all()
        e = with_empties(c)
        want_e = e.want()
        assert want_e.size == 133 and want_e.sum() == want.sum()
        for moved, _ in forms(n):
            dev = Device(hip, c, moved)
            same(dev.uniform(c.batch, c.T), want, (n, loop, moved, hits, "uniform"))
            same(dev.ragged(c.off), want, (n, loop, moved, hits, "ragged"))
            same(dev.ragged(e.off), want_e, (n, loop, moved, hits, "ragged with empties"))
            same(dev.ragged(e.off, bound=c.T), want_e, (n, loop, moved, hits, "ragged with empties, bound 130"))


# ---------------------------------------------------------------------- c. long uniform batches at chunk edges

@pytest.mark.parametrize("n,d,T", [(63, 4, T) for T in LONG_T] + [(1247, 16, 4097)])
def test_long_uniform_batches_at_chunk_edges(hip, n, d, T):
    """T > 4096: zero_words, k_hits_parity_chunked (one atomicXor per ciphertext and chunk), k_partial_to_bits.  One
    ciphertext per position of P(T) -- the ends of the first bitmap words, either side of every 65 536-term chunk edge,
    the last two terms -- with its one hit there; T is odd, so no ciphertext but the first starts at a word edge, and
    the batch is odd.  T = 65 537 and 131 073 end in a chunk of one term.  A second hit across each edge gives 0; the
    batch in mirrored order puts the first-term hit behind, and the last-term hit in front of, another ciphertext."""
    tab = Table(n, d)
    for double, mirror in ((False, False), (True, False), (False, True)):
        c = long_uniform(tab, T, double, mirror)
        P = boundary_positions(T)
        want = c.want()
        assert c.batch % 2 == 1 and (want[:len(P)] == (not double)).all() and not want[len(P):].any()
        for moved, _ in forms(n):
            same(Device(hip, c, moved).uniform(c.batch, T), want, (n, T, double, mirror, moved))


# ---------------------------------------------------------------------- d. long ciphertexts inside a CSR batch

@pytest.mark.parametrize("q", range(RAGGED_RUNS))
def test_long_ragged_ciphertexts_at_chunk_edges(hip, q):
    """Counts 3, 0, 4096, 4097, 65537, 1, 131073, 0, 65535 at N = 63: the long ciphertexts (slots and chunk entries of
    k_hits_parity_chunks) start 3, 4, 6 and 7 bits into a bitmap word and hold one hit each, at the q-th position of
    their own P(T).  A bound above 4096 changes nothing."""
    c = long_ragged(Table(63, 4), q)
    want = c.want()
    assert want.tolist() == [int(t > LONG and q < len(boundary_positions(t))) for t in RAGGED_COUNTS]
    dev = Device(hip, c)
    same(dev.ragged(c.off), want, (q, "ragged"))
    same(dev.ragged(c.off, bound=max(RAGGED_COUNTS)), want, (q, "ragged, bound 131073"))
    same(dev.ragged(c.off, bound=LONG + 1000000), want, (q, "ragged, loose bound"))


# ---------------------------------------------------------------------- e. fused product and sum

@pytest.mark.parametrize("n,d", [(1247, 16), (129, 3)])
def test_fused_product_and_sum_on_near_misses(hip, n, d):
    """csgn_decrypt_product_uniform / csgn_decrypt_sum_uniform against np_decrypt of the product and the sum built in
    numpy; Dec(L) and Dec(R) take all four combinations."""
    lib = hip.lib
    tab = Table(n, d)
    dmask = hip.upload(hip.key_mask(n, tab.key))
    for t1, t2 in FUSED_SHAPES:
        L, R = fused_operands(tab, t1, t2)
        batch = L.shape[0]
        want = {True: np_bits(n, tab.key, np_mul(L, R), np.arange(batch + 1) * (t1 * t2)),
                False: np_bits(n, tab.key, np_add(L, R), np.arange(batch + 1) * (t1 + t2))}
        assert 0 < want[True].sum() < batch and 0 < want[False].sum() < batch
        dl_, dr_ = hip.upload(L.ravel()), hip.upload(R.ravel())
        for product, fn in ((True, lib.csgn_decrypt_product_uniform), (False, lib.csgn_decrypt_sum_uniform)):
            nbytes = int(lib.csgn_decrypt_combined_scratch_bytes(batch, t1, t2))
            scratch = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device=hip.device)
            bits = torch.full((batch + 2 * GUARD,), 7, dtype=torch.uint8, device=hip.device)
            check(fn(n, batch, t1, t2, dl_.data_ptr(), dr_.data_ptr(), dmask.data_ptr(), bits[GUARD:].data_ptr(),
                     scratch.data_ptr(), hip.stream))
            h = hip.download(bits)
            assert (h[:GUARD] == 7).all() and (h[GUARD + batch:] == 7).all()
            same(h[GUARD:GUARD + batch], want[product], (n, t1, t2, "product" if product else "sum"))


# ---------------------------------------------------------------------- f. the explicit-bitlen stream decrypt

@pytest.mark.parametrize("n,d", [(1247, 16), (4096, 32), (65, 4), (130, 5)])
def test_bitlen_stream_decrypt_on_near_misses(hip, n, d):
    """csgn_decrypt_bitlen with the canonical bitlen: every near miss of every fill as a one-term ciphertext (0), the
    hit (1), and the d near misses with the hit as one ciphertext (1, and csgn_decrypt_uniform's bit)."""
    lib = hip.lib
    tab = Table(n, d)
    dkey = hip.upload(tab.key)
    dmask = hip.upload(hip.key_mask(n, tab.key))

    def stream(v):
        v = np.ascontiguousarray(v, dtype=np.uint64).ravel()
        dv, dbl = hip.upload(v), hip.upload(canonical_bitlen(n, v.size // tab.dl))
        nbytes = int(lib.csgn_bitlen_scratch_bytes(v.size))
        scratch = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device=hip.device)
        bit = torch.full((1 + 2 * GUARD,), 7, dtype=torch.uint8, device=hip.device)
        check(lib.csgn_decrypt_bitlen(n, d, v.size, dv.data_ptr(), dbl.data_ptr(), dkey.data_ptr(),
                                      bit[GUARD:].data_ptr(), scratch.data_ptr(), hip.stream))
        h = hip.download(bit)
        assert (h[:GUARD] == 7).all() and (h[GUARD + 1:] == 7).all()
        return int(h[GUARD])

    for fill in FILLS:
        misses, hit = near_misses(n, tab.key, fill, 41)
        for i, m in enumerate(misses):
            assert stream(m) == 0 == np_decrypt(n, tab.key, m), (n, fill, i)
        assert stream(hit) == 1 == np_decrypt(n, tab.key, hit), (n, fill)
        both = np.concatenate([misses.ravel(), hit])
        assert stream(both) == 1 == np_decrypt(n, tab.key, both), (n, fill)
        assert stream(misses) == 0, (n, fill)
        assert int(hip.download(hip.decrypt_uniform(n, 1, d + 1, hip.upload(both), dmask))[0]) == 1, (n, fill)
