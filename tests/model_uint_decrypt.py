"""What the csgn_uint_decrypt tests share: include/csgn_hip.h's definition of the packed decryption -- bit j of word e =
Dec(element e of plane j), every bit tests/model_decrypt.py's np_bits, the definition bit by bit -- and the inputs: planes
of near misses (every key bit but one, the missing position rotating; model_decrypt.Table) with hits planted at the first
and last term of an element and on each side of every boundary the kernel has (a wave's 64-unit passes and its groups
of four, the chunks of every chunk size the tests set), so that the CPU tests (tests/test_uint_decrypt_cpu.py) check the
very words the GPU tests (tests/test_uint_decrypt_gpu.py) decrypt."""
import numpy as np

from tests.model import csr
from tests.model_decrypt import Table, np_bits, uniform_off

D_OF = {64: 4, 1247: 16, 1300: 4, 4096: 32}         # the key sizes of model_decrypt.CONTEXTS
SUM8 = (1, 2, 3, 5, 9, 17, 33, 65, 129)             # the planes of an 8-bit sum of fresh integers, and its carry
CHUNKS = (1, 7, 256, 0)                             # knob uint_decrypt_chunk in the tests; 0: by shape
CHUNK_BY_SHAPE = 1024                               # csgn_uint_decrypt.hip: kChunkByShape
LONG = 4096                                         # the most terms of one element of a ragged plane


def packed(n, key, planes, offs):
    """uint64[batch]: the OR over j of np_bits(plane j) << j."""
    v = np.zeros(len(offs[0]) - 1, dtype=np.uint64)
    for j, (w, off) in enumerate(zip(planes, offs)):
        v |= np_bits(n, key, w, off).astype(np.uint64) << np.uint64(j)
    return v


def edge_positions(T, U):
    """The terms of a T-term element where a hit goes: the first and the last, each side of the first edges of every
    chunk size (and of the last one inside T), and the terms that hold the units on each side of a pass (64 units) and
    of a group of four passes (256 units) counted from the element's first unit."""
    P = {0, T - 1}
    for c in (7, 256, CHUNK_BY_SHAPE):
        for edge in (c, 2 * c, (T - 1) // c * c):
            P |= {edge - 1, edge}
    for units in (64, 128, 256, 512):
        P |= {(units - 1) // U, units // U}
    return sorted(q for q in P if 0 <= q < T)


def hit_terms(count, e, j, salt, U):
    """Where the hits of element e of plane j go, `count` its terms: none, one or two of edge_positions in turn (two
    hits cancel), so that with three elements -- or three salts -- every plane has both bits."""
    if count == 0:
        return []
    P = edge_positions(count, U)
    k = (e + j + salt) % 3
    if k == 1 or (k == 2 and len(P) < 2):
        return []
    a = (e + j) % len(P)
    return [P[a]] if k == 0 else [P[a], P[(a + 1) % len(P)]]


def plane_words(tab, j, off, salt, U):
    """[terms, dL] of the plane with CSR offsets `off`: near misses (rotation j), the hits of hit_terms planted."""
    off = np.asarray(off, dtype=np.int64)
    total = int(off[-1])
    w = tab.misses(np.arange(total), r=j) if total else np.zeros((0, tab.dl), dtype=np.uint64)
    at = [int(off[e]) + q for e in range(len(off) - 1) for q in hit_terms(int(off[e + 1] - off[e]), e, j, salt, U)]
    if at:
        at = np.array(at, dtype=np.int64)
        w[at] = tab.hits(at)
    return w


class Planes:
    """One call's inputs and what it must give.  counts[j]: an int (uniform, that many terms per element) or a sequence
    of `batch` term counts (ragged)."""

    def __init__(self, n, batch, counts, salt=0, seed=41):
        self.n, self.batch = n, batch
        self.tab = Table(n, D_OF[n], seed)
        self.key = self.tab.key
        dl = self.tab.dl
        U = dl // 2 if dl % 2 == 0 else dl
        self.terms = [int(c) if np.isscalar(c) else 0 for c in counts]
        self.offs = [uniform_off(batch, c) if np.isscalar(c) else csr(list(c)) for c in counts]
        assert all(len(o) == batch + 1 for o in self.offs)
        self.bounds = [0 if np.isscalar(c) else int(max(c)) for c in counts]
        self.words = [plane_words(self.tab, j, off, salt, U) for j, off in enumerate(self.offs)]
        self.want = packed(n, self.key, self.words, self.offs)

    def plane_bits(self, j):
        return (self.want >> np.uint64(j)) & np.uint64(1)


def salts(batch):
    """The input sets of a case: with fewer than three elements a plane cannot hold both bits, three salts do."""
    return (0, 1, 2) if batch < 3 else (0,)


def has_both_bits(cases):
    """Every plane has a 0 and a 1 among the expected bits of the case's input sets."""
    w = len(cases[0].terms)
    for j in range(w):
        bits = np.concatenate([c.plane_bits(j) for c in cases])
        if not (bits.min() == 0 and bits.max() == 1):
            return False
    return True
