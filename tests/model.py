"""What the tests share: the numpy restatement of include/csgn_hip.h's definitions (gates, integer steps, comparisons
with a public constant, lookup tables, table reads, gather), the same definitions composed over the oracle's and the
compiled reference's operators, term-count formulas, key / layout / ctypes helpers, and the `lib` and `hip` fixtures.
The codes are literal values, as in include/csgn_hip.h, so that the tests do not depend on csgn_amd/capi.py."""
import ctypes as C
import json

import numpy as np
import pytest

from csgn_amd.capi import check
from oracle.binding import canonical_bitlen, glibc_draws

NOT, XNOR, NAND, OR, NOR, MUX, ADD_PLAIN, MUL_PLAIN = range(1, 9)
GATES = {"not": NOT, "xnor": XNOR, "nand": NAND, "or": OR, "nor": NOR, "mux": MUX, "add_plain": ADD_PLAIN,
         "mul_plain": MUL_PLAIN}
ADD_HALF, ADD_FULL, EQ_STEP, LT_FIRST, LT_STEP = range(1, 6)
STEPS = {"add_half": ADD_HALF, "add_full": ADD_FULL, "eq_step": EQ_STEP, "lt_first": LT_FIRST, "lt_step": LT_STEP}
EQ, NE, LT, LE, GT, GE = range(1, 7)
CMPS = {"eq": EQ, "ne": NE, "lt": LT, "le": LE, "gt": GT, "ge": GE}
CLEAR = {EQ: np.equal, NE: np.not_equal, LT: np.less, LE: np.less_equal, GT: np.greater, GE: np.greater_equal}
OK, INVALID, UNSUPPORTED, NO_DEVICE = 0, -1, -2, -3
MASK64 = (1 << 64) - 1
LIMIT = 1 << 62

# csgn_small_op: out = left + right (kind 0) or left * right (kind 1), t1 / t2 terms a side
SMALL_OP = np.dtype([("left", "<u8"), ("right", "<u8"), ("out", "<u8"), ("t1", "<u4"), ("t2", "<u4"),
                     ("kind", "<u4"), ("reserved", "<u4")])


@pytest.fixture(scope="module")
def lib():
    from csgn_amd import build, capi
    build.build_hip()
    return capi.load_library()


@pytest.fixture(scope="module")
def hip():
    from csgn_amd.batch import HipPath
    return HipPath(0)


# -- term arrays and the gates, in numpy, on uniform batches: words[batch, terms, dL] ----------------------------------
def const_term(n, bit):
    dl = (n + 63) // 64
    t = np.full(dl, MASK64 if bit else 0, dtype=np.uint64)
    if n % 64 and bit:
        t[-1] = np.uint64((MASK64 << (64 - n % 64)) & MASK64)
    return t


def np_add(x, y):
    return np.concatenate([x, y], axis=1)


def np_mul(x, y):
    b, t1, dl = x.shape
    return (x[:, :, None, :] & y[:, None, :, :]).reshape(b, t1 * y.shape[1], dl)


def np_gate(n, gate, a=None, b=None, sel=None, plain=None):
    """Words of one gate over a uniform batch, by the table of include/csgn_hip.h."""
    batch = a.shape[0]
    one = np.broadcast_to(const_term(n, 1), (batch, 1, a.shape[2]))
    if plain is not None:
        pc = np.where((np.asarray(plain) & 1).astype(bool)[:, None, None], one, np.uint64(0))
    if gate == NOT:
        return np_add(a, one)
    if gate == XNOR:
        return np_add(np_add(a, b), one)
    if gate == NAND:
        return np_add(np_mul(a, b), one)
    if gate == OR:
        return np_add(np_add(a, b), np_mul(a, b))
    if gate == NOR:
        return np_add(np_add(np_add(a, b), np_mul(a, b)), one)
    if gate == MUX:
        return np_add(np_mul(sel, np_add(a, b)), b)
    if gate == ADD_PLAIN:
        return np_add(a, pc)
    if gate == MUL_PLAIN:
        return np_mul(a, pc)
    raise ValueError(gate)


def gate_clear(gate, a, b=0, s=0, p=0):
    return {NOT: 1 - a, XNOR: 1 - (a ^ b), NAND: 1 - (a & b), OR: a | b, NOR: 1 - (a | b),
            MUX: a if s else b, ADD_PLAIN: a ^ p, MUL_PLAIN: a & p}[gate]


def rand_terms(n, batch, terms, seed):
    """Random canonical terms (the unused low bits of the last word zero)."""
    dl = (n + 63) // 64
    w = np.random.default_rng(seed).integers(0, 2**64, size=(batch, terms, dl), dtype=np.uint64)
    w[:, :, -1] &= const_term(n, 1)[-1]
    return w


def compose_gate(ops, n, gate, a, b=None, sel=None, p=0):
    """The same definition for ONE element through `ops` = (add, mul) on flat word arrays: the compiled reference's
    operators or the oracle's.  Order of the operands exactly as in the table."""
    add, mul = ops
    one, pc = const_term(n, 1), const_term(n, p)
    if gate == NOT:
        return add(a, one)
    if gate == XNOR:
        return add(add(a, b), one)
    if gate == NAND:
        return add(mul(a, b), one)
    if gate == OR:
        return add(add(a, b), mul(a, b))
    if gate == NOR:
        return add(add(add(a, b), mul(a, b)), one)
    if gate == MUX:
        return add(mul(sel, add(a, b)), b)
    if gate == ADD_PLAIN:
        return add(a, pc)
    if gate == MUL_PLAIN:
        return mul(a, pc)
    raise ValueError(gate)


def oracle_ops(oracle, n):
    return (lambda x, y: oracle.add(x, y)[0], lambda x, y: oracle.mul(n, x, y)[0])


def ref_ops(ref, n, d):
    dl = (n + 63) // 64

    def bl(x):
        return canonical_bitlen(n, len(x) // dl)

    return (lambda x, y: ref.add(n, d, x, bl(x), y, bl(y))[0], lambda x, y: ref.mul(n, d, x, bl(x), y, bl(y))[0])


def gate_terms(gate, ts, ta, tb):
    return {NOT: ta + 1, XNOR: ta + tb + 1, NAND: ta * tb + 1, OR: ta + tb + ta * tb, NOR: ta + tb + ta * tb + 1,
            MUX: ts * (ta + tb) + tb, ADD_PLAIN: ta + 1, MUL_PLAIN: ta}[gate]


# -- the per-bit integer steps -----------------------------------------------------------------------------------------
def np_step(n, step, x, a, b):
    """Outputs of one step over uniform batches (words[batch, terms, dL]): (out0,) or (sum, carry) for the ADD steps."""
    one = np.broadcast_to(const_term(n, 1), (a.shape[0], 1, a.shape[2]))
    if step == ADD_HALF:
        return np_add(a, b), np_mul(a, b)
    if step == ADD_FULL:
        return np_add(np_add(a, b), x), np_add(np_mul(a, b), np_mul(np_add(a, b), x))
    if step == EQ_STEP:
        return (np_mul(x, np_add(np_add(a, b), one)),)
    if step == LT_FIRST:
        return (np_mul(np_add(a, one), b),)
    if step == LT_STEP:
        return (np_add(np_mul(np_add(a, b), np_add(b, x)), x),)
    raise ValueError(step)


def compose_step(ops, n, step, x, a, b):
    """The same definition for ONE element through `ops` = (add, mul) on flat word arrays."""
    add, mul = ops
    one = const_term(n, 1)
    if step == ADD_HALF:
        return add(a, b), mul(a, b)
    if step == ADD_FULL:
        return add(add(a, b), x), add(mul(a, b), mul(add(a, b), x))
    if step == EQ_STEP:
        return (mul(x, add(add(a, b), one)),)
    if step == LT_FIRST:
        return (mul(add(a, one), b),)
    if step == LT_STEP:
        return (add(mul(add(a, b), add(b, x)), x),)
    raise ValueError(step)


def step_terms(step, tx, ta, tb):
    return {ADD_HALF: (ta + tb, ta * tb), ADD_FULL: (ta + tb + tx, ta * tb + (ta + tb) * tx),
            EQ_STEP: (tx * (ta + tb + 1),), LT_FIRST: ((ta + 1) * tb,),
            LT_STEP: ((ta + tb) * (tb + tx) + tx,)}[step]


# -- whole operations, composed from the steps in numpy (planes: list of words[batch, 1, dL], bit 0 first) -------------
def np_not(n, x):
    return np_add(x, np.broadcast_to(const_term(n, 1), (x.shape[0], 1, x.shape[2])))


def np_uint_add(n, a, b):
    w = len(a)
    s0, c = np_step(n, ADD_HALF, None, a[0], b[0])
    out = [s0]
    for j in range(1, w):
        s, c = np_step(n, ADD_FULL, c, a[j], b[j])
        out.append(s)
    return out


def np_uint_sub(n, a, b):
    c = np.broadcast_to(const_term(n, 1), (a[0].shape[0], 1, a[0].shape[2]))
    out = []
    for j in range(len(a)):
        s, c = np_step(n, ADD_FULL, c, a[j], np_not(n, b[j]))
        out.append(s)
    return out


def np_uint_eq(n, a, b):
    e = np_not(n, np_add(a[0], b[0]))                               # logicXnor
    for j in range(1, len(a)):
        (e,) = np_step(n, EQ_STEP, e, a[j], b[j])
    return e


def np_uint_lt(n, a, b):
    (lt,) = np_step(n, LT_FIRST, None, a[0], b[0])
    for j in range(1, len(a)):
        (lt,) = np_step(n, LT_STEP, lt, a[j], b[j])
    return lt


def np_uint_select(n, s, a, b):
    return [np_add(np_mul(s, np_add(aj, bj)), bj) for aj, bj in zip(a, b)]   # logicMux


# -- comparisons with a public constant, over any (add, mul, one, zero) ------------------------------------------------
def lowest(k, bit, w):
    return next(j for j in range(w) if (k >> j) & 1 == bit)


def compose_plain(cmp, planes, k, add, mul, one, zero):
    """include/csgn_hip.h's table, in exactly its order."""
    w = len(planes)
    nt = lambda j: add(planes[j], one)                                       # logicNot
    base = {NE: EQ, LE: GT, GE: LT}.get(cmp, cmp)
    if base == EQ:
        g = lambda j: planes[j] if (k >> j) & 1 else nt(j)
        r = g(0)
        for j in range(1, w):
            r = mul(r, g(j))
    elif base == LT:
        if k == 0:
            r = zero
        else:
            m = lowest(k, 1, w)
            r = nt(m)
            for j in range(m + 1, w):
                r = add(mul(r, planes[j]), nt(j)) if (k >> j) & 1 else mul(r, nt(j))
    else:
        if k == (1 << w) - 1:
            r = zero
        else:
            m = lowest(k, 0, w)
            r = planes[m]
            for j in range(m + 1, w):
                r = mul(r, planes[j]) if (k >> j) & 1 else add(mul(r, nt(j)), planes[j])
    return add(r, one) if cmp != base else r


def np_plain(n, cmp, planes, k):
    """Words of one comparison over uniform planes (words[batch, t_j, dL], bit 0 first)."""
    batch, _, dl = planes[0].shape
    one = np.broadcast_to(const_term(n, 1), (batch, 1, dl))
    zero = np.broadcast_to(const_term(n, 0), (batch, 1, dl))
    return compose_plain(cmp, planes, k, np_add, np_mul, one, zero)


def plain_terms(cmp, w, k, t):
    """The same composition over term counts (Python integers: no overflow); 0 past 2^62."""
    counts = compose_plain(cmp, list(t), k, lambda x, y: x + y, lambda x, y: x * y, 1, 1)
    return counts if counts < LIMIT else 0


def full_width_cases(w):
    """(cmp, k) pairs at widths up to 64 whose result over fresh 1-term planes stays at most 4096 terms: EQ / NE with few
    zero bits in k, LT / GE at the top (2w terms) and at 2^(w-1), GT / LE just below the top, and the ZERO constants (LT
    at 0, GT at the top).  Picked by plain_terms: GT at small k is the expensive end (2^w terms at k = 0)."""
    top = (1 << w) - 1
    ks = {0, 1, top, top - 1, 1 << (w - 1), top ^ (1 << (w - 1)), top ^ 0x2D5, top ^ 0x3FF, top ^ (0b1011 << (w - 5)),
          top ^ ((1 << (w - 1)) | 1), (1 << (w - 1)) | 1}
    cases = sorted((c, k) for k in ks for c in CMPS.values() if 0 < plain_terms(c, w, k, [1] * w) <= 4096)
    for must in ((EQ, top), (NE, top ^ 0x3FF), (LT, top), (GE, top), (LT, 1 << (w - 1)), (GE, 1 << (w - 1)), (LT, 0),
                 (GT, top - 1), (LE, top - 1), (GT, top), (GT, top ^ 0x2D5)):
        assert must in cases, must
    return cases


# -- bit planes encrypted and decrypted by the oracle ------------------------------------------------------------------
def encrypt_planes(oracle, n, key, values, w, seed):
    dl = (n + 63) // 64
    count = len(values)
    out = []
    for j in range(w):
        bits = ((np.asarray(values, dtype=np.uint64) >> np.uint64(j)) & np.uint64(1)).astype(np.uint8)
        out.append(oracle.encrypt_seq(n, key, bits, glibc_draws(seed * 100 + j, count * (n + 2)))[0].reshape(count, 1, dl))
    return out


def decrypt_bits(oracle, n, key, words):
    return np.array([oracle.decrypt_canonical(n, key, words[e].ravel()) for e in range(words.shape[0])], dtype=bool)


def decrypt_value(oracle, n, key, outs):
    v = np.zeros(outs[0].shape[0], dtype=np.uint64)
    for j, o in enumerate(outs):
        v |= decrypt_bits(oracle, n, key, o).astype(np.uint64) << np.uint64(j)
    return v


# -- lookup tables: the tables the tests use, and the definition over any (add, mul, one, zero) ------------------------
def aes_sbox():
    """The AES S-box from its definition: the inverse in GF(2^8) mod x^8 + x^4 + x^3 + x + 1, then the affine map."""
    def gmul(a, b):
        r = 0
        while b:
            if b & 1:
                r ^= a
            a = ((a << 1) ^ 0x11B) if a & 0x80 else a << 1
            b >>= 1
        return r

    inv = [0] * 256
    for a in range(1, 256):
        inv[a] = next(b for b in range(1, 256) if gmul(a, b) == 1)
    rot = lambda x, s: ((x << s) | (x >> (8 - s))) & 0xFF
    return [inv[x] ^ rot(inv[x], 1) ^ rot(inv[x], 2) ^ rot(inv[x], 3) ^ rot(inv[x], 4) ^ 0x63 for x in range(256)]


def random_table(w, m, seed):
    rng = np.random.default_rng(seed)
    if m == 64:
        return [int(v) for v in rng.integers(0, 2**64 - 1, 1 << w, dtype=np.uint64, endpoint=True)]
    return [int(v) for v in rng.integers(0, 1 << m, 1 << w)]


def mul4x4():
    """Two-input 4x4-bit multiply: index a + (b << 4), 8-bit product."""
    return [(x & 15) * (x >> 4) for x in range(256)]


def np_anf(table, w):
    anf = [int(v) for v in table]
    for i in range(w):
        for x in range(1 << w):
            if (x >> i) & 1:
                anf[x] ^= anf[x ^ (1 << i)]
    return anf


def compose_lut(planes, table, w, m, add, mul, one, zero):
    """include/csgn_hip.h's definition, in exactly its order: one value per output bit."""
    anf = np_anf(table, w)
    outs = []
    for j in range(m):
        r = None
        for S in range(1 << w):
            if not (anf[S] >> j) & 1:
                continue
            mono = one
            first = True
            for i in range(w):
                if (S >> i) & 1:
                    mono = planes[i] if first else mul(mono, planes[i])
                    first = False
            r = mono if r is None else add(r, mono)
        outs.append(zero if r is None else r)
    return outs


def np_lut(n, planes, table, m):
    """Words of every output over uniform planes (words[batch, t_i, dL], bit 0 first)."""
    batch, _, dl = planes[0].shape
    one = np.broadcast_to(const_term(n, 1), (batch, 1, dl))
    zero = np.broadcast_to(const_term(n, 0), (batch, 1, dl))
    return compose_lut(planes, table, len(planes), m, np_add, np_mul, one, zero)


def lut_terms(table, w, m, t):
    return compose_lut(list(t), table, w, m, lambda x, y: x + y, lambda x, y: x * y, 1, 1)


def c_terms(lib, table, w, m, t):
    out = (C.c_uint64 * m)()
    rc = lib.csgn_uint_lut_terms(w, m, u64s(table), u64s(t), out)
    return rc, list(out)


# -- table reads at encrypted indices, over any (add, mul, one, zero) --------------------------------------------------
def compose_read(index, rows, add, mul, one, zero):
    """include/csgn_hip.h's definition, in exactly its order.  index: the v index planes; rows[r][j]: plane j of table
    row r.  One value per table plane."""
    out = None
    for r in range(len(rows)):
        eq = compose_plain(EQ, index, r, add, mul, one, zero)
        prods = [mul(eq, d) for d in rows[r]]
        out = prods if out is None else [add(o, p) for o, p in zip(out, prods)]
    return out


def np_read(n, index, table):
    """Words of every output over uniform planes: index[k] = words[batch, s_k, dL], table[j] = words[rows, t_j, dL]."""
    batch, _, dl = index[0].shape
    one = np.broadcast_to(const_term(n, 1), (batch, 1, dl))
    zero = np.broadcast_to(const_term(n, 0), (batch, 1, dl))
    rows = [[np.broadcast_to(d[r:r + 1], (batch,) + d.shape[1:]) for d in table] for r in range(table[0].shape[0])]
    return compose_read(index, rows, np_add, np_mul, one, zero)


def np_read_fast(n, index, table):
    """np_read's words with every output concatenated once (a left-nested sum of concatenations is one
    concatenation): linear in the output, for the large shapes of the device tests."""
    outs = [[] for _ in table]
    for r in range(table[0].shape[0]):
        eq = np_plain(n, EQ, index, r)
        for j, d in enumerate(table):
            outs[j].append(np_mul(eq, np.broadcast_to(d[r:r + 1], (eq.shape[0],) + d.shape[1:])))
    return [np.concatenate(o, axis=1) for o in outs]


def read_terms(s, rows):
    """E by the definition itself: the EQ terms of every row."""
    return sum(int(np.prod([(sk if (r >> k) & 1 else sk + 1) for k, sk in enumerate(s)], dtype=object))
               for r in range(rows))


def c_E(lib, v, s, rows):
    return int(lib.csgn_uint_read_terms(v, u64s(s) if s is not None else None, rows))


# -- gather, tile and broadcast ----------------------------------------------------------------------------------------
def tile_index(count_in, count_out):
    return np.arange(count_out, dtype=np.uint64) % np.uint64(max(count_in, 1))


def np_gather_offsets(src_off, idx):
    """Output offsets: exclusive prefix sums of the gathered elements' term counts (count_out + 1 entries)."""
    src_off = np.asarray(src_off, dtype=np.uint64)
    idx = np.asarray(idx, dtype=np.int64)
    sizes = (src_off[idx + 1] - src_off[idx]) if len(idx) else np.zeros(0, dtype=np.uint64)
    return np.concatenate([[0], np.cumsum(sizes, dtype=np.uint64)]).astype(np.uint64)


def np_gather(words, src_off, idx, dl):
    """Words and offsets of the gather of a CSR batch (`words`: total terms * dl words)."""
    out_off = np_gather_offsets(src_off, idx)
    parts = [words[int(src_off[i]) * dl:int(src_off[i + 1]) * dl] for i in np.asarray(idx, dtype=np.int64)]
    out = np.concatenate(parts).astype(np.uint64) if parts else np.zeros(0, dtype=np.uint64)
    assert len(out) == int(out_off[-1]) * dl
    return out, out_off


def np_gather_uniform(words, t, idx, dl):
    elems = np.asarray(words, dtype=np.uint64).reshape(-1, t * dl)
    return elems[np.asarray(idx, dtype=np.int64)].ravel()


# -- keys, layouts, fresh ciphertexts and ctypes arrays ----------------------------------------------------------------
def u64s(xs):
    return (C.c_uint64 * max(len(xs), 1))(*[int(x) for x in xs])


def make_key(n, d, seed):
    rng = np.random.default_rng(seed)
    return rng.permutation(n)[:d].astype(np.uint64)


def csr(counts):
    off = np.zeros(len(counts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(counts, dtype=np.uint64))
    return off


def planted(oracle, n, key, terms, hits, seed):
    dl = oracle.default_len(n)
    v = oracle.synth(seed, n, 0, terms * dl).reshape(terms, dl)
    v[:hits] |= oracle.key_mask(n, key)
    w, b = int(key[0]) // 64, 63 - int(key[0]) % 64
    v[hits:, w] &= ~np.uint64(1 << b)
    rng = np.random.default_rng(seed)
    rng.shuffle(v, axis=0)
    return np.ascontiguousarray(v.reshape(-1))


def explicit_randomness(n, key, bit, draws):
    """Map the reference's rand() stream (src/SecretKey.cpp:35-80) onto the explicit
    arguments of csgn_encrypt_explicit.  Returns (rnd words, chosen, last, draws used)."""
    dl = (n + 63) // 64
    keyset = set(int(k) for k in key)
    rnd = np.zeros(dl, dtype=np.uint64)
    pos = 0

    def setbit(i, v):
        if v:
            rnd[i // 64] |= np.uint64(1 << (63 - i % 64))

    if bit & 1:
        for i in range(n):
            if i not in keyset:
                setbit(i, int(draws[pos]) % 2)
                pos += 1
        return rnd, 0, 0, pos
    chosen = int(key[int(draws[pos]) % len(key)])
    pos += 1
    others = []
    for i in range(n):
        if i == chosen:
            continue
        v = int(draws[pos]) % 2
        pos += 1
        setbit(i, v)
        if i in keyset:
            others.append(v)
    last = 0
    if not (others and all(others)):
        last = int(draws[pos]) % 2
        pos += 1
    return rnd, chosen, last, pos


# -- circuits described through the C ABI ------------------------------------------------------------------------------
FAKE_PTR = 0x1000                                   # a device pointer the host passes never read


class Described:
    """A circuit described through the C ABI and, beside it, the same description as Python tuples."""

    def __init__(self, lib, n, batch, mask_ptr=FAKE_PTR):
        self.lib, self.n, self.batch, self.mask_ptr = lib, n, batch, mask_ptr
        self.dl = int(lib.csgn_default_len(n))
        self.c = C.c_void_p()
        check(lib.csgn_circuit_create(n, batch, C.byref(self.c)))
        self.terms = []                             # per value
        self.nodes = []                             # ("in",) / ("add", a, b) / ("mul", a, b) per value
        self.decrypts = []                          # value ids, in bits_id order
        self.outputs = set()

    def close(self):
        self.lib.csgn_circuit_destroy(self.c)

    def _new(self, fn, *args):
        v = C.c_uint32()
        check(fn(self.c, *args, C.byref(v)))
        return v.value

    def input(self, terms=1):
        v = self._new(self.lib.csgn_circuit_input, terms)
        self.terms.append(terms)
        self.nodes.append(("in",))
        return v

    def add(self, a, b):
        v = self._new(self.lib.csgn_circuit_add, a, b)
        self.terms.append(self.terms[a] + self.terms[b])
        self.nodes.append(("add", a, b))
        return v

    def mul(self, a, b):
        v = self._new(self.lib.csgn_circuit_mul, a, b)
        self.terms.append(self.terms[a] * self.terms[b])
        self.nodes.append(("mul", a, b))
        return v

    def decrypt(self, a):
        bid = self._new(self.lib.csgn_circuit_decrypt, a, self.mask_ptr)
        assert bid == len(self.decrypts)
        self.decrypts.append(a)
        return bid

    def output(self, v):
        check(self.lib.csgn_circuit_output(self.c, v))
        self.outputs.add(v)

    def plan(self, flags):
        check(self.lib.csgn_circuit_optimize(self.c, flags))
        buf = C.create_string_buffer(1 << 22)
        check(self.lib.csgn_circuit_plan_json(self.c, buf, len(buf)))
        return json.loads(buf.value.decode())


def random_circuit(lib, seed, n, batch, mask_ptr=FAKE_PTR, max_terms=400):
    rng = np.random.default_rng(seed)
    d = Described(lib, n, batch, mask_ptr)
    for _ in range(int(rng.integers(2, 6))):
        d.input(int(rng.integers(1, 4)))
    for _ in range(int(rng.integers(3, 14))):
        k = len(d.terms)
        # mostly chains (the newest value and something else), sometimes two old values: shared sub-expressions
        a = k - 1 if rng.random() < 0.6 else int(rng.integers(0, k))
        b = int(rng.integers(0, k))
        if rng.random() < 0.45 and d.terms[a] * d.terms[b] <= max_terms:
            d.mul(a, b)
        elif d.terms[a] + d.terms[b] <= max_terms:
            d.add(a, b)
    k = len(d.terms)
    for v in sorted(set(int(x) for x in rng.integers(0, k, size=int(rng.integers(1, 4))))):
        d.decrypt(v)
    if rng.random() < 0.5:
        d.decrypt(k - 1)
    for v in sorted(set(int(x) for x in rng.integers(0, k, size=int(rng.integers(0, 3))))):
        d.output(v)
    return d


def config5(lib, n, batch, levels=16, mask_ptr=FAKE_PTR):
    d = Described(lib, n, batch, mask_ptr)
    ins = [d.input(1) for _ in range(1 + levels // 2 + 2 * (levels // 2))]
    x, k = ins[0], 1
    for level in range(1, levels + 1):
        if level % 2:
            x = d.add(x, ins[k]); k += 1
        else:
            x = d.mul(x, d.add(ins[k], ins[k + 1])); k += 2
    d.decrypt(x)
    return d, x


def evaluate(d, inputs):
    """Every value of the description, element by element: [batch, terms, dl] uint64 arrays."""
    vals = []
    for node in d.nodes:
        if node[0] == "in":
            vals.append(inputs[len(vals)])
        elif node[0] == "add":
            vals.append(np.concatenate([vals[node[1]], vals[node[2]]], axis=1))
        else:
            a, b = vals[node[1]], vals[node[2]]
            vals.append((a[:, :, None, :] & b[:, None, :, :]).reshape(d.batch, -1, d.dl))
    return vals


def decrypt_masked(vals, mask):
    hits = np.all((vals & mask) == mask, axis=2)               # [batch, terms]
    return (hits.sum(axis=1) & 1).astype(np.uint8)


def execute(d, plan, inputs, mask):
    """Run the PLAN: kept nodes only, in order, every read and write at the plan's byte offsets and pitches."""
    block = np.zeros(plan["bytes"] // 8 + 8, dtype=np.uint64)
    rng = np.random.default_rng(5)
    block[:] = rng.integers(0, 2 ** 63, size=block.size, dtype=np.uint64)       # stale bytes must never matter
    dl, B = d.dl, d.batch

    def view(v):
        pv = plan["values"][v]
        base, pitch, t = pv["offset"] // 8, pv["pitch"], d.terms[v]
        assert pv["offset"] % 8 == 0 and pitch >= t * dl
        idx = base + np.arange(B)[:, None] * pitch + np.arange(t * dl)[None, :]
        return idx

    def read(v):
        pv = plan["values"][v]
        assert pv["region"] and pv["parent"] < 0 and pv["pitch"] == d.terms[v] * dl, f"value {v} is read but not dense"
        return block[view(v)].reshape(B, d.terms[v], dl)

    def write(v, words):
        block[view(v)] = words.reshape(B, -1)

    for v, node in enumerate(d.nodes):
        if node[0] == "in":
            assert plan["values"][v]["addressable"]
            write(v, inputs[v])
    def copy_operand(op, side):
        """operand `side` of add `op` into its slice of the sum (what the add's own copy, or the prologue launch, does)"""
        ta = d.terms[op["a"]]
        out = plan["values"][op["out"]]
        base, pitch = out["offset"] // 8, out["pitch"]
        v = op["b"] if side else op["a"]
        idx = base + (ta * dl if side else 0) + np.arange(B)[:, None] * pitch + np.arange(d.terms[v] * dl)[None, :]
        block[idx] = read(v).reshape(B, -1)

    # the prologue: every hoisted copy (its source is an input) before the first node
    for op in plan["ops"]:
        if op["kind"] == 0 and not op["elided"]:
            for side, key in ((0, "hoist_a"), (1, "hoist_b")):
                if op[key]:
                    assert d.nodes[op["b"] if side else op["a"]][0] == "in" and not op["placed_b" if side else "placed_a"]
                    copy_operand(op, side)
    bits = {}
    for i, op in enumerate(plan["ops"]):
        if op["elided"]:
            continue
        if op["kind"] == 1:
            a, b = read(op["a"]), read(op["b"])
            write(op["out"], (a[:, :, None, :] & b[:, None, :, :]).reshape(B, -1, dl))
        elif op["kind"] == 0:
            ta = d.terms[op["a"]]
            out = plan["values"][op["out"]]
            base, pitch = out["offset"] // 8, out["pitch"]
            if op["placed_a"]:
                pa = plan["values"][op["a"]]
                assert pa["parent"] == op["out"] and pa["offset"] == out["offset"] and pa["pitch"] == pitch
            elif not op["hoist_a"]:
                copy_operand(op, 0)
            if not op["placed_b"] and not op["hoist_b"]:
                copy_operand(op, 1)
            elif op["placed_b"]:
                pb = plan["values"][op["b"]]
                assert pb["parent"] == op["out"] and pb["offset"] == out["offset"] + ta * dl * 8 and pb["pitch"] == pitch
        elif op["kind"] == 2:
            def ev(ei):
                e = plan["exprs"][ei]
                if e["kind"] < 0:
                    return decrypt_masked(read(e["value"]), mask)
                l, r = ev(e["l"]), ev(e["r"])
                return (l & r) if e["kind"] == 1 else (l ^ r)
            bid = sum(1 for o in plan["ops"][:i] if o["kind"] == 2)
            bits[bid] = ev(op["expr"]) if op["expr"] >= 0 else decrypt_masked(read(op["a"]), mask)
    return block, bits, read


# ---------------------------------------------------------------- caller outputs inside guard words (GPU tests)

FILL = np.uint64(0xA5A5A5A5A5A5A5A5)        # neither ZERO nor ONE nor a word a random term is likely to hold
GUARD_WORDS = 64                            # 512 bytes either side: the outputs keep a fresh tensor's alignment


class GuardedOutputs:
    """Outputs of exactly the documented sizes, each inside a larger tensor whose every word holds FILL.  `outs` are the
    views a wrapper of csgn_amd/batch.py takes as `out` / `outs`; check(wants) then asserts, output by output, that the
    words equal the numpy definition and that the guard words before and after still hold FILL.  A form that leaves a
    range unwritten shows as "never written" (the wanted words there are not FILL), one that writes wrong words or past
    its end as wrong words or a broken guard: a fresh tensor of the caching allocator tells none of these apart."""

    def __init__(self, hip, sizes, shift=0):
        self.hip = hip
        self.sizes = [int(s) for s in sizes]
        self.first = GUARD_WORDS + int(shift)            # shift = 1: the outputs start 8 bytes off a 16-byte boundary
        self.whole = [hip.upload(np.full(s + 2 * GUARD_WORDS + int(shift), FILL, dtype=np.uint64)) for s in self.sizes]
        self.outs = [t[self.first:self.first + s] for t, s in zip(self.whole, self.sizes)]

    def check(self, wants, what=None):
        assert len(wants) == len(self.sizes), (what, len(wants), len(self.sizes))
        got = []
        for j, (t, s, want) in enumerate(zip(self.whole, self.sizes, wants)):
            a = self.hip.download(t)
            want = np.asarray(want, dtype=np.uint64).ravel()
            assert want.size == s, (what, j, "the output is not of the documented size", want.size, s)
            g = a[self.first:self.first + s]
            wrong = g != want
            if wrong.any():
                at = int(np.flatnonzero(wrong)[0])
                never = int(np.count_nonzero(wrong & (g == FILL)))
                raise AssertionError((what, "output %d" % j, "%d of %d words wrong" % (int(wrong.sum()), s),
                                      "%d of them never written" % never, "first at word %d" % at,
                                      hex(int(g[at])), hex(int(want[at]))))
            assert (a[:self.first] == FILL).all(), (what, j, "words in front of the output were written")
            assert (a[self.first + s:] == FILL).all(), (what, j, "words behind the output were written")
            got.append(g)
        return got
