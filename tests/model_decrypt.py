"""What the decrypt tests share: include/csgn_hip.h's definition of decryption bit by bit in numpy (no packed mask:
nothing in common with the kernels' `(term & mask) == mask`), near-miss terms -- every key bit set but one --, a pure
Python copy of the host rule that picks the pass-1 form, and the batches built from the near misses, so that the CPU
tests (tests/test_decrypt_cpu.py) check the very words the GPU tests (tests/test_decrypt_gpu.py) decrypt.

Why near misses: tests/model.py's planted() clears only key[0] in its non-hits, so a kernel that ignores any other key
position still gives every bit planted() expects."""
from typing import NamedTuple, Optional

import numpy as np

from tests.model import const_term, csr, make_key, rand_terms

FILLS = ("bare", "ones", "rand")
CHUNK = 65536                                       # terms per chunk of the long pass 2 (csgn_decrypt.hip)
LONG = 4096                                         # a ciphertext of more terms is "long"


# -- the definition ----------------------------------------------------------------------------------------------------
def np_keybits(n, key, words):
    """bool[terms, d]: bit key[i] of every term.  Every term is unpacked to its n bits (bit p = word p // 64, bit
    63 - p % 64), 8192 terms at a time."""
    dl = (n + 63) // 64
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint64)).reshape(-1, dl)
    key = np.asarray(key, dtype=np.int64)
    out = np.empty((w.shape[0], key.size), dtype=bool)
    for s in range(0, w.shape[0], 8192):
        bits = np.unpackbits(w[s:s + 8192].astype(">u8").view(np.uint8), axis=1)[:, :n]
        out[s:s + 8192] = bits[:, key] != 0
    return out


def np_hits(n, key, words):
    """bool[terms]: AND over the key positions."""
    return np_keybits(n, key, words).all(axis=1)


def np_decrypt(n, key, words):
    """The plaintext of ONE ciphertext: XOR over its terms of the AND over the key positions; no terms: 0."""
    return int(np.count_nonzero(np_hits(n, key, words)) & 1)


def fold(hits, off):
    """uint8[batch]: XOR of `hits` (one bool per term) over each ciphertext of the CSR offsets `off`."""
    c = np.concatenate([[0], np.cumsum(hits, dtype=np.int64)])
    off = np.asarray(off, dtype=np.int64)
    return ((c[off[1:]] - c[off[:-1]]) & 1).astype(np.uint8)


def np_bits(n, key, words, off):
    """np_decrypt of every ciphertext of a CSR batch."""
    return fold(np_hits(n, key, words), off)


def mutant_bits(n, key, words, off):
    """uint8[d, batch]: row i = the bits of a decryption that ignores key position i (the mask minus bit key[i])."""
    kb = np_keybits(n, key, words)
    return np.stack([fold(np.delete(kb, i, axis=1).all(axis=1), off) for i in range(kb.shape[1])])


# -- near misses -------------------------------------------------------------------------------------------------------
def np_key_mask(n, key):
    m = np.zeros((n + 63) // 64, dtype=np.uint64)
    for k in key:
        m[int(k) // 64] |= np.uint64(1 << (63 - int(k) % 64))
    return m


def near_misses(n, key, fill, seed=0):
    """(misses[d, dL], hit[dL]): misses[i] has every key bit except key[i].  bare: nothing else is set (the mask minus
    one bit); ones: everything else is set (the unused low bits of the last word zero, as in every canonical term);
    rand: a random canonical term ORed with the mask.  `hit` is the same term with all key bits."""
    mask = np_key_mask(n, key)
    if fill == "bare":
        hit = mask.copy()
    elif fill == "ones":
        hit = const_term(n, 1)
    elif fill == "rand":
        hit = rand_terms(n, 1, 1, 7000 + seed)[0, 0] | mask
    else:
        raise ValueError(fill)
    misses = np.tile(hit, (len(key), 1))
    for i, k in enumerate(key):
        misses[i, int(k) // 64] &= ~np.uint64(1 << (63 - int(k) % 64))
    return misses, hit


def lanes(key):
    """The 32-bit lanes of a 16-byte unit that hold a key position."""
    return {(int(k) // 32) % 4 for k in key}


def lane_key(n, d, seed=41):
    """make_key at the first seed from `seed` on whose key has a position in each of the four 32-bit lanes of a 16-byte
    unit (d >= 4): a compare that drops one lane must then drop a key position."""
    while True:
        key = make_key(n, d, seed)
        if d < 4 or n < 128 or len(lanes(key)) == 4:
            return key
        seed += 1


class Table:
    """The near misses and hits of the three fills under one key, and the rotation every batch below uses: term number
    p is a near miss on key position (p + p // d + r) % d with fill p % 3, so positions rotate against the slots of a
    workgroup and against the fills."""

    def __init__(self, n, d, seed=41):
        self.n, self.d, self.dl = n, d, (n + 63) // 64
        self.key = lane_key(n, d, seed)
        pairs = [near_misses(n, self.key, f, seed) for f in FILLS]
        self.miss = np.stack([p[0] for p in pairs])             # [fill, position, dL]
        self.hit = np.stack([p[1] for p in pairs])              # [fill, dL]

    def position(self, p, r=0):
        p = np.asarray(p, dtype=np.int64)
        return (p + p // self.d + r) % self.d

    def misses(self, p, r=0):
        p = np.asarray(p, dtype=np.int64)
        return self.miss[p % 3, self.position(p, r)]

    def scattered(self, p, seed=97):
        """Near misses on random positions (one fixed stream, indexed by p): in a long ciphertext the rotation above
        gives every position nearly the same number of misses (T / d, even for most), and a decryption that ignores one
        position would turn an even number of them into hits."""
        p = np.asarray(p, dtype=np.int64)
        pos = np.random.default_rng(seed).integers(0, self.d, size=int(p.max()) + 1)
        return self.miss[p % 3, pos[p]]

    def hits(self, p):
        return self.hit[np.asarray(p, dtype=np.int64) % 3]


# -- the host rule that picks the pass-1 form (csgn_decrypt.hip: decrypt) ----------------------------------------------
def pass1_form(n, moved):
    """(unit bytes, U, K, TB).  16-byte units when dL is even and terms and mask are 16-byte aligned (`moved`: they
    start 8 bytes off).  Segment form: the smallest k <= 8 with 256k % U == 0 and (256k / U) % 8 == 0, U <= 64; else
    the looping form (K = 0) with its 256-term workgroups."""
    dl = (n + 63) // 64
    wide = dl % 2 == 0 and not moved
    U = dl // 2 if wide else dl
    K = 0
    if U <= 64:
        K = next((k for k in range(1, 9) if (256 * k) % U == 0 and (256 * k // U) % 8 == 0), 0)
    return (16 if wide else 8, U, K, 256 * K // U if K else 256)


def reachable_K():
    return sorted({pass1_form(64 * dl, moved)[2] for dl in range(1, 129) for moved in (False, True)} - {0})


# N / d -> the forms of the aligned call and of the call with terms and mask moved 8 bytes (None: dL is odd, the call
# is the same one).  K = 0: only the looping form exists.  K = 7 (U = 7, 14) is reached by no other test.
CONTEXTS = {
    (63, 4): ((8, 1, 1, 256), None),
    (128, 8): ((16, 1, 1, 256), (8, 2, 1, 128)),
    (129, 3): ((8, 3, 3, 256), None),
    (193, 6): ((16, 2, 1, 128), (8, 4, 1, 64)),
    (448, 7): ((8, 7, 7, 256), None),
    (896, 9): ((16, 7, 7, 256), (8, 14, 7, 128)),
    (1247, 16): ((16, 10, 5, 128), (8, 20, 5, 64)),
    (4096, 32): ((16, 32, 1, 8), (8, 64, 2, 8)),
    (704, 9): ((8, 11, 0, 256), None),
    (1300, 4): ((8, 21, 0, 256), None),
    (8320, 8): ((16, 65, 0, 256), (8, 130, 0, 256)),
}


def forms(n):
    """The (moved, form) pairs a context runs."""
    out = [(False, pass1_form(n, False))]
    if ((n + 63) // 64) % 2 == 0:
        out.append((True, pass1_form(n, True)))
    return out


# -- batches -----------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    label: str
    n: int
    key: np.ndarray
    words: np.ndarray                       # [terms, dL]
    off: np.ndarray                         # CSR offsets, batch + 1
    T: Optional[int]                        # the term count of every ciphertext of a uniform batch, None: CSR only
    planted: tuple                          # the term numbers that hold a hit put there on purpose (boundary positions)

    @property
    def batch(self):
        return len(self.off) - 1

    def want(self):
        return np_bits(self.n, self.key, self.words, self.off)


def uniform_off(batch, T):
    return np.arange(batch + 1, dtype=np.uint64) * np.uint64(T)


# a. every key position in every slot of pass 1
def slot_terms(n):
    """M: two full workgroups of the widest form and a ragged tail, at least 515 (64 workgroups of TB = 8)."""
    return max([515] + [2 * f[3] + 3 for _, f in forms(n)])


def slot_coverage(tab, form, M, r, hit_at):
    """Where the near misses of the list with rotation r land in a pass-1 launch of `form`: the set of (position, pass j
    of the segment workgroup) and (position, "tail": the last, partial workgroup).  The miss on position i is in the
    unit that holds bit key[i]."""
    unit_bytes, U, K, TB = form
    p = np.array([q for q in range(M) if q not in hit_at], dtype=np.int64)
    pos = tab.position(p, r)
    unit = (tab.key[pos].astype(np.int64) // 64) // (unit_bytes // 8)
    got = set()
    if K:
        got |= set(zip(pos.tolist(), (((p % TB) * U + unit) // 256).tolist()))
    tail = p >= (M // TB) * TB
    got |= set((int(i), "tail") for i in pos[tail])
    return got


def slot_need(tab, form):
    _, _, K, _ = form
    return {(i, j) for i in range(tab.d) for j in list(range(K)) + ["tail"]}


def slot_hits(M):
    return set(range(36, M, 37))            # every 37th term is the hit of its fill


def slot_rotations(tab):
    """The rotations r (fewest first found, r = 0 always) after which every form of the context has seen the miss on
    every key position in every pass and in the tail workgroup: a tail of 3 terms cannot hold d positions at once."""
    M = slot_terms(tab.n)
    need = [(f, slot_need(tab, f)) for _, f in forms(tab.n)]
    seen = [set() for _ in need]
    rs = []
    for r in range(4 * tab.d):
        new = [slot_coverage(tab, f, M, r, slot_hits(M)) for f, _ in need]
        if r == 0 or any(n_ - s for n_, s in zip(new, seen)):
            rs.append(r)
            for s, n_ in zip(seen, new):
                s |= n_
        if all(s >= nd for s, (_, nd) in zip(seen, need)):
            return rs
    raise AssertionError(("no set of rotations covers every slot", tab.n, tab.d))


def slot_list(tab, r):
    """M one-term ciphertexts: term p a near miss on position (p + p // d + r) % d, every 37th the hit of its fill."""
    M = slot_terms(tab.n)
    p = np.arange(M)
    w = tab.misses(p, r)
    h = np.array(sorted(slot_hits(M)), dtype=np.int64)
    w[h] = tab.hits(h)
    return Case("slots r=%d" % r, tab.n, tab.key, w, uniform_off(M, 1), 1, tuple(h.tolist()))


def regroup(case, T):
    """The same terms as a uniform batch of T-term ciphertexts (the remainder dropped)."""
    b = case.words.shape[0] // T
    return case._replace(label=case.label + " T=%d" % T, words=case.words[:b * T], off=uniform_off(b, T), T=T,
                         planted=tuple(q for q in case.planted if q < b * T))


# b. one hit at every position of a ciphertext
def every_position(tab, hits, T=130):
    """T ciphertexts of T near misses; hits = 1: a single hit at term b of ciphertext b (uniform offsets T * b walk
    through every bit offset of a bitmap word); 0: none; 2: hits at b and (b + 1) % T."""
    p = np.arange(T * T)
    w = tab.misses(p)
    at = []
    for k in range(hits):
        at += [b * T + (b + k) % T for b in range(T)]
    at = np.array(sorted(at), dtype=np.int64)
    w[at] = tab.hits(at)
    return Case("every position, %d hits" % hits, tab.n, tab.key, w, uniform_off(T, T), T, tuple(at.tolist()))


def with_empties(case, at=(0, 65, 130)):
    """The same words as a CSR batch with an empty ciphertext in front of ciphertexts `at` (130: behind the last)."""
    counts = np.diff(case.off.astype(np.int64)).tolist()
    for a in sorted(at, reverse=True):
        counts.insert(a, 0)
    return case._replace(label=case.label + " + empties", off=csr(counts), T=None)


# c. / d. long ciphertexts: hits at the edges of bitmap words and of the 65 536-term chunks
def boundary_positions(T):
    """P(T): terms 0, 1, 62, 63, 64, 65; either side of every chunk edge inside T; T - 2 and T - 1."""
    P = {0, 1, 62, 63, 64, 65, T - 2, T - 1}
    for c in range(1, (T + CHUNK - 1) // CHUNK):
        P |= {CHUNK * c - 1, CHUNK * c, CHUNK * c + 1}
    return sorted(q for q in P if 0 <= q < T)


LONG_T = (4097, 65535, 65537, 131073)


def long_uniform(tab, T, double, mirror=False):
    """One ciphertext per position of P(T), near misses everywhere and one hit at that position; the batch is made odd
    by a ciphertext without a hit.  double: a second hit on the other side of the edge (p + 1, or p - 1 at the end).
    mirror: P(T) from its end, so that the ciphertext whose hit is its first term FOLLOWS one (whose last chunk must not
    take that bit) and the one whose hit is its last term is followed by one (which must not take that bit either)."""
    P = boundary_positions(T)[::-1] if mirror else boundary_positions(T)
    batch = len(P) | 1
    w = tab.scattered(np.arange(batch * T))
    at = [b * T + q for b, q in enumerate(P)]
    if double:
        at += [b * T + (q + 1 if q + 1 < T else q - 1) for b, q in enumerate(P)]
    at = np.array(sorted(at), dtype=np.int64)
    w[at] = tab.hits(at)
    return Case("long uniform T=%d%s%s" % (T, " double" if double else "", " mirror" if mirror else ""), tab.n, tab.key, w, uniform_off(batch, T), T,
                tuple(at.tolist()))


RAGGED_COUNTS = (3, 0, 4096, 4097, 65537, 1, 131073, 0, 65535)
RAGGED_RUNS = max(len(boundary_positions(t)) for t in RAGGED_COUNTS if t > LONG)
# the position stream of run q: with seven ciphertexts that hold terms, one stream in eight leaves some key position with
# an even number of misses in every ciphertext; these do not (tests/test_decrypt_cpu.py asserts it)
RAGGED_SEEDS = tuple(97 + q for q in range(RAGGED_RUNS))


def long_ragged(tab, q):
    """One CSR batch: every long ciphertext (> 4096 terms) has one hit, at the q-th position of its own P(T) (none if
    P(T) is shorter); the short ones hold near misses only.  The long ones start at bit offsets 3, 4, 6 and 7 mod 64."""
    off = csr(list(RAGGED_COUNTS))
    w = tab.scattered(np.arange(int(off[-1])), RAGGED_SEEDS[q])
    at = []
    for b, t in enumerate(RAGGED_COUNTS):
        if t > LONG and q < len(boundary_positions(t)):
            at.append(int(off[b]) + boundary_positions(t)[q])
    at = np.array(at, dtype=np.int64)
    w[at] = tab.hits(at)
    return Case("long ragged q=%d" % q, tab.n, tab.key, w, off, None, tuple(at.tolist()))


def without_hit(case, term):
    """The case with the planted hit at `term` turned into a near miss of the same fill."""
    w = case.words.copy()
    tab = Table(case.n, len(case.key))
    assert np.array_equal(tab.key, case.key) and np.array_equal(w[term], tab.hits(term))
    w[term] = tab.misses(np.array([term]))[0]
    return case._replace(words=w, planted=tuple(q for q in case.planted if q != term))


# e. operands of the fused product / sum decrypt
FUSED_SHAPES = ((1, 1), (5, 7), (33, 9))


def fused_operands(tab, t1, t2, batch=12):
    """L[batch, t1, dL]: near misses and, in two elements of three, one hit; R[batch, t2, dL]: near misses and
    b % 4 hits (at most t2).  Dec(L) and Dec(R) each take both values, in every combination."""
    L = tab.misses(np.arange(batch * t1)).reshape(batch, t1, tab.dl)
    R = tab.misses(np.arange(batch * t2), r=1).reshape(batch, t2, tab.dl)
    for b in range(batch):
        if b % 3:
            L[b, b % t1] = tab.hits(b)
        for k in range(min(b % 4, t2)):
            R[b, (b + 2 * k) % t2] = tab.hits(b + k)
    return L, R
