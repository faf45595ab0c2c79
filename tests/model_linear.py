"""The model of csgn_uint_linear (include/csgn_hip.h): a public matrix over F2 applied to a bit-sliced encrypted
integer.  The definition from tests/model.py's np_add and const_term; the same definition over any `add`; the terms
table and the decode by position; the clear value; certfhe/UInt.h's F2Matrix builders restated; and the kernel's grid
(tile, plane, unit) replayed from csgn_uint_linear_plan's figures."""
import numpy as np

from tests.model import LIMIT, const_term, np_add

ONE, ZERO = "one", "zero"               # the decode's constant planes (in_width and in_width + 1 in the C ABI)


def bits_of(mask):
    return [i for i in range(64) if (mask >> i) & 1]


# -- the definition ----------------------------------------------------------------------------------------------------
def compose_linear(planes, rows, constant, add, one, zero):
    """include/csgn_hip.h's definition in exactly its order, over any `add`: one value per row."""
    outs = []
    for j, row in enumerate(rows):
        r = None
        for i in bits_of(row):
            r = planes[i] if r is None else add(r, planes[i])
        if (constant >> j) & 1:
            r = one if r is None else add(r, one)
        outs.append(zero if r is None else r)
    return outs


def np_linear(n, planes, rows, constant=0):
    """Words of every output plane over uniform planes (words[batch, t_i, dL], bit 0 first)."""
    batch, _, dl = planes[0].shape
    one = np.broadcast_to(const_term(n, 1), (batch, 1, dl))
    zero = np.broadcast_to(const_term(n, 0), (batch, 1, dl))
    return [np.ascontiguousarray(o) for o in compose_linear(planes, rows, constant, np_add, one, zero)]


# -- the terms table and the decode by position ------------------------------------------------------------------------
def linear_terms(ta, row, cbit):
    """T_j; 0 where the C ABI refuses (a zero count, a row bit past the planes, 2^62 or more)."""
    if not 1 <= len(ta) <= 64 or row >> len(ta) or cbit not in (0, 1) or any(t == 0 or t >= LIMIT for t in ta):
        return 0
    total = sum(ta[i] for i in bits_of(row)) + cbit if row else 1
    return total if total < LIMIT else 0


def linear_decode(ta, row, cbit, q):
    """(plane, term) that output term q of the row copies; plane ONE / ZERO for the constant."""
    for i in bits_of(row):
        if q < ta[i]:
            return i, q
        q -= ta[i]
    assert q == 0 and (cbit or row == 0)
    return (ONE if cbit else ZERO), 0


def symbolic_linear(ta, rows, constant):
    """The definition over lists of (plane, term) labels: what the decode must give term for term."""
    planes = [[(i, x) for x in range(t)] for i, t in enumerate(ta)]
    return compose_linear(planes, rows, constant, lambda x, y: x + y, [(ONE, 0)], [(ZERO, 0)])


# -- the clear value ---------------------------------------------------------------------------------------------------
def clear_linear(rows, constant, x):
    y = 0
    for j, row in enumerate(rows):
        y |= (bin(row & x).count("1") & 1) << j
    return y ^ constant


def compose_rows(outer, inner):
    """Rows of x -> outer(inner(x)) over F2."""
    out = []
    for row in outer:
        r = 0
        for i in bits_of(row):
            r ^= inner[i]
        out.append(r)
    return out


# -- F2Matrix's builders, restated ---------------------------------------------------------------------------------------
def low(w):
    return (1 << w) - 1


def m_identity(w):
    return [1 << j for j in range(w)]


def m_shift_left(w, s):
    return [1 << (j - s) if j >= s else 0 for j in range(w)]


def m_shift_right(w, s):
    return [1 << (j + s) if j + s < w else 0 for j in range(w)]


def m_rotate_left(w, s):
    return [1 << ((j - s) % w) for j in range(w)]


def m_rotate_right(w, s):
    return [1 << ((j + s) % w) for j in range(w)]


def m_mask(w, k):
    return [(1 << j) if (k >> j) & 1 else 0 for j in range(w)]


def m_xor(a, b):
    return [x ^ y for x, y in zip(a, b)]


def from_columns(w, image):
    """Rows of the linear map whose image of the basis vector 1 << i is image(i)."""
    cols = [image(i) for i in range(w)]
    return [sum(((cols[i] >> j) & 1) << i for i in range(w)) for j in range(w)]


def clmul(a, k):
    r = 0
    for i in bits_of(k):
        r ^= a << i
    return r


def m_clmul(w, k):
    return from_columns(w, lambda i: clmul(1 << i, k) & low(w))


def gf_mul(w, a, k, poly):
    r = 0
    for _ in range(w):
        if k & 1:
            r ^= a
        k >>= 1
        a <<= 1
        if a >> w:
            a = (a & low(w)) ^ (poly & low(w))
    return r


def m_gf_mul(w, k, poly):
    return from_columns(w, lambda i: gf_mul(w, 1 << i, k, poly))


def m_gray_encode(w):
    return m_xor(m_identity(w), m_shift_right(w, 1))


def m_gray_decode(w):
    return [low(w) & ~low(j) for j in range(w)]


def sigma0_256():
    """SHA-256's small sigma 0: rotr(a, 7) ^ rotr(a, 18) ^ (a >> 3)."""
    return m_xor(m_xor(m_rotate_right(32, 7), m_rotate_right(32, 18)), m_shift_right(32, 3))


def mix_columns():
    """AES MixColumns on one 32-bit column, byte c at bits 8c .. 8c + 7: out_c = 2 a_c ^ 3 a_{c+1} ^ a_{c+2} ^ a_{c+3}."""
    def image(i):
        c, x = divmod(i, 8)
        v = 1 << x
        out = 0
        for r in range(4):
            f = [2, 3, 1, 1][(c - r) % 4]
            out |= gf_mul(8, v, f, 0x11B) << (8 * r)
        return out
    return from_columns(32, image)


def crc32_step8():
    """The CRC-32 (reflected, 0xEDB88320) register advanced by eight zero message bits."""
    def image(i):
        c = 1 << i
        for _ in range(8):
            c = (c >> 1) ^ (0xEDB88320 if c & 1 else 0)
        return c
    return from_columns(32, image)


def random_rows(w_in, w_out, seed):
    rng = np.random.default_rng(seed)
    return [int(x) & low(w_in) for x in rng.integers(0, 2**64, w_out, dtype=np.uint64)]


# -- the kernel's grid, replayed from the plan -------------------------------------------------------------------------
def replay_grid(ta, rows, constant, batch, U, G, launch_blocks):
    """Every lane of every launch of k_uint_linear at U units a term and G elements a tile, as csgn_uint_linear.hip
    places them: returns (count[j]: per-unit write counts of output plane j as int arrays, launches, workgroups per
    tile) and asserts every source index in range.  Sources are decoded by linear_decode, not by the kernel's own
    search: the words are compared on the device; here it is the coverage."""
    T = [linear_terms(ta, r, (constant >> j) & 1) for j, r in enumerate(rows)]
    PU = [t * U for t in T]
    blocks = [-(-G * pu // 256) for pu in PU]
    first = np.concatenate([[0], np.cumsum(blocks)])
    per = int(first[-1])
    tiles = -(-batch // G)
    per_launch = max(1, launch_blocks // per)
    count = [np.zeros(batch * pu, dtype=np.int64) for pu in PU]
    launches = 0
    for t0 in range(0, tiles, per_launch):
        nt = min(per_launch, tiles - t0)
        e_base = t0 * G
        ne = min(batch - e_base, nt * G)
        launches += 1
        for bid in range(nt * per):
            tile, wb = divmod(bid, per)
            p = int(np.searchsorted(first, wb, side="right")) - 1
            assert 0 <= p < len(rows)
            e0 = tile * G
            assert e0 < ne
            ge = min(G, ne - e0)
            off = (wb - int(first[p])) * 256 + np.arange(256)
            off = off[off < ge * PU[p]]
            if off.size == 0:
                continue
            el, r = off // PU[p], off % PU[p]
            e = e_base + e0 + el
            assert e.max() < batch
            for q in np.unique(r // U):                              # the source of every term this workgroup touches
                plane, term = linear_decode(ta, rows[p], (constant >> p) & 1, int(q))
                if plane in (ONE, ZERO):
                    plane, term = 0, 0                               # the unconditional load: the element's first unit
                assert 0 <= plane < len(ta) and 0 <= term < ta[plane]
                assert (int(e.max()) * ta[plane] + term + 1) * U <= batch * ta[plane] * U
            np.add.at(count[p], (e_base + e0) * PU[p] + off, 1)
    return count, launches, per


# -- the shapes of tests/test_uint_linear_gpu.py, which tests/test_uint_linear_cpu.py replays on the host ---------------
NS = (64, 1247, 1300)                   # one 8-byte unit a term; 16-byte units (10 a term); 8-byte units (21 a term)


def term_counts(w, mode):
    return [1] * w if mode == "ones" else [1 + i for i in range(w)]          # (1, 2, 3, ...)


def small_rows(w):
    """(rows, constant): a single bit; all ones; zero; zero with the constant; the all-ones row again, with the
    constant; the single bit with the constant; the top bit alone; every second bit."""
    full = low(w)
    rows = [1, full, 0, 0, full, 1, 1 << (w - 1), full & 0x55]
    return rows, 0b00111000


def gpu_shapes():
    """(name, ta, rows, constant, batches) at every n of NS unless the name says otherwise."""
    shapes = []
    for w in (1, 2, 3, 5):
        for mode in ("ones", "ramp"):
            rows, constant = small_rows(w)
            shapes.append(("w%d-%s" % (w, mode), term_counts(w, mode), rows, constant, (1, 3, 257)))
    # segment ends at units 3, 73, 74, 79 and 81 of an element at n = 64: inside a wave, and past a wave inside a workgroup
    shapes.append(("boundaries", [3, 70, 1, 5, 2], [0b11111, 0b11010, 0b00110], 0b010, (1, 7, 40)))
    return shapes


DENSE = ("dense64", [1] * 64, random_rows(64, 64, 64), 0x8000000000000001 | (0xF0 << 24), (2, 33))
