"""Every place where the host cuts one call into several launches, with the second and later launches really run.

A launch takes at most kMaxBlocks256 = (2^32 - 1) / 256 workgroups (csgn_device.h), about 16.7 M, and no shape a test
can hold comes near that, so knob launch_blocks lowers the limit: 15 reproduces the production geometry (kMaxBlocks256
is 15 mod 16, so a launch boundary of the flat ragged kernels falls inside a workgroup's range of 2, 4, 8 or 16 chunks),
16 is the aligned geometry, 48 a third residue with fewer launches.  Every case runs once with the knob unset and once
per cap, into outputs of exactly the documented size between guard words (tests/model.py, GuardedOutputs), and every
run's words must equal the model of the operation's own GPU test -- not merely one another.  A launch that gets a wrong
e0 / row0 / col0 / block_base / u0 writes one slice twice and leaves another holding the fill word.

The launch counts beside the shapes follow from the host code's arithmetic (launch_groups in csgn_device.h and the
callers named in each test); "a + b" means a full launches and one of b groups, tiles, workgroups or units.
Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from tests import test_matmul_gpu as mm
from tests import test_uint_find_gpu as fg
from tests import test_uint_lut_gpu as lg
from tests import test_uint_read_gpu as rg
from tests.model import (GuardedOutputs, csr, hip, lut_terms, np_gather, np_gather_uniform, np_lut,  # noqa: F401
                         np_read_fast, rand_terms, read_terms)
from tests.model_find import find_terms
from tests.model_matmul import np_matmul

pytestmark = pytest.mark.gpu

CAPS = (15, 16, 48)
# 16-byte units (even dL) and 8-byte units (odd dL) at nearly the same units a term, so both widths plan the same groups
WIDE_N, NARROW_N = 4096, 2100           # dL = 64: U = 32;  dL = 33: U = 33


def each_cap(knobs, call, caps=CAPS):
    """call(cap) with the knob unset (cap 0: the one launch every other test runs), then at every cap."""
    knobs.unset("launch_blocks")
    call(0)
    for cap in caps:
        knobs.set("launch_blocks", cap)
        call(cap)
    knobs.unset("launch_blocks")


# ------------------------------------------------------------------------------ launch_groups: elements of a batch

BATCH = 301                             # no multiple of any group size below (2, 3, 4)


@pytest.mark.parametrize("n", [WIDE_N, NARROW_N])
@pytest.mark.parametrize("tmode", ["fresh", "multi"])
def test_lut_element_groups(hip, knobs, n, tmode):
    """k_uint_lut: e0 moves every plane and output pointer.  Tables whose algebraic normal form holds every monomial, so
    the term counts, and with them the elements a workgroup takes, are fixed:
    fresh, 5 planes, 2 outputs of 32 terms: G = 2 at U = 32 (what the subset tables leave room for), G = 3 at U = 33;
    multi, planes of 3 and 4 terms, 4 outputs of 20 terms: G = 3 (8192 units a workgroup / 80 U).
    One workgroup a group.  G = 2: 151 groups, 10 + 1 launches at cap 15, 9 + 7 at 16, 3 + 7 at 48;
    G = 3: 101 groups, 6 + 11 at 15, 6 + 5 at 16, 2 + 5 at 48."""
    ts, m = ([1] * 5, 2) if tmode == "fresh" else ([3, 4], 4)
    table = [(1 << m) - 1] + [0] * ((1 << len(ts)) - 1)
    assert lut_terms(table, len(ts), m, ts) == ([32, 32] if tmode == "fresh" else [20] * 4)
    planes = [rand_terms(n, BATCH, t, 2000 + 7 * i + t) for i, t in enumerate(ts)]
    want = [x.ravel() for x in np_lut(n, planes, table, m)]
    knobs.set("uint_lut_fused", 1)
    each_cap(knobs, lambda cap: lg.run(hip, n, planes, table, m, want))


@pytest.mark.parametrize("n", [WIDE_N, NARROW_N])
@pytest.mark.parametrize("tmode", ["fresh", "multi"])
def test_read_element_groups(hip, knobs, n, tmode):
    """k_uint_read: e0 moves every index and output pointer.
    fresh: 3 index planes, 8 rows (E = 27), table planes of 1 and 2 terms: 81 U units an element, G = 3;
    multi: index planes of 2 and 1 terms, 3 rows of 4 (E = 13), table planes of 2 and 3 terms: 65 U units, G = 3.
    One workgroup a group, 101 groups: 6 + 11 launches at cap 15, 6 + 5 at 16, 2 + 5 at 48."""
    s, rows, t = ([1, 1, 1], 8, [1, 2]) if tmode == "fresh" else ([2, 1], 3, [2, 3])
    assert read_terms(s, rows) == (27 if tmode == "fresh" else 13)
    index = [rand_terms(n, BATCH, sk, 2100 + k) for k, sk in enumerate(s)]
    table = [rand_terms(n, rows, tj, 2110 + j) for j, tj in enumerate(t)]
    want = [x.ravel() for x in np_read_fast(n, index, table)]
    knobs.set("uint_read_fused", 1)
    each_cap(knobs, lambda cap: rg.run(hip, n, index, table, want))


@pytest.mark.parametrize("n", [WIDE_N, NARROW_N])
@pytest.mark.parametrize("tmode", ["fresh", "multi"])
def test_find_element_groups(hip, knobs, n, tmode):
    """k_uint_find: e0 moves the query and output pointers; 5 rows, every row in every launch.
    fresh: 2 planes (P = 9), two 1-term value planes and member: G = 4 elements by RP = 4 rows a workgroup, 2 workgroups
    a group, 76 groups: 10 + 6 launches at cap 15, 9 + 4 at 16, 3 + 4 at 48;
    multi: keys of 2 and 1 terms, queries of 1 and 2 (P = 16), one value plane and member: G = 2, RP = 4, 2 workgroups a
    group, 151 groups: 21 + 4 at 15, 18 + 7 at 16, 6 + 7 at 48."""
    u, s = ([1, 1], [1, 1]) if tmode == "fresh" else ([2, 1], [1, 2])
    t = [1, 1] if tmode == "fresh" else [1]
    assert find_terms(u, s) == (9 if tmode == "fresh" else 16)
    rows = 5
    keys = [rand_terms(n, rows, uk, 2200 + k) for k, uk in enumerate(u)]
    query = [rand_terms(n, BATCH, sk, 2210 + k) for k, sk in enumerate(s)]
    values = [rand_terms(n, rows, tj, 2220 + j) for j, tj in enumerate(t)]
    want = fg.definition(n, keys, query, values, True)
    knobs.set("uint_find_form", 1)
    knobs.unset("uint_find_rparts")
    each_cap(knobs, lambda cap: fg.run(hip, n, keys, query, values, True, want))


@pytest.mark.parametrize("n", [63, 65])                     # dL = 1: 8-byte units;  dL = 2: one 16-byte unit a term
def test_find_rows_split_by_the_launch_cap(hip, knobs, n):
    """k_uint_find with uint_find_rparts unset: the rows of one launch come from the cap.  37 rows as in
    test_find_rows_split_over_launches (tests/test_uint_find_gpu.py); five planes of 3, 3, 3, 3 and 2 terms on both sides
    give P = 7^4 * 5 = 12005, six ranges of q, so a row part is six workgroups; RP = 2 rows a part, 19 parts.
    Cap 15 and 16: 2 parts, 4 rows a launch, 9 + 1 row; cap 48: 8 parts, 16 rows a launch, 2 + 5 rows."""
    u = s = [3, 3, 3, 3, 2]
    assert find_terms(u, s) == 12005
    rows, batch = 37, 1
    keys = [rand_terms(n, rows, uk, 2300 + k) for k, uk in enumerate(u)]
    query = [rand_terms(n, batch, sk, 2310 + k) for k, sk in enumerate(s)]
    values = [rand_terms(n, rows, 1, 2320 + j) for j in range(2)]
    want = fg.definition(n, keys, query, values, True)
    knobs.set("uint_find_form", 1)
    knobs.unset("uint_find_rparts")
    each_cap(knobs, lambda cap: fg.run(hip, n, keys, query, values, True, want))


# ------------------------------------------------------------------------------ k_matmul: rows, columns, minE

def matmul_each_cap(hip, knobs, n, a, b, rows, inner, cols, caps=CAPS):
    want = np_matmul(a, b, rows, inner, cols)
    bt = mm.transpose_b(b, inner, cols)
    knobs.set("matmul_form", 1)
    for transposed in (False, True):
        each_cap(knobs, lambda cap: mm.run(hip, n, a, bt if transposed else b, rows, inner, cols, transposed, want),
                 caps)


@pytest.mark.parametrize("n", [65, 129])                    # one 16-byte unit a term; three 8-byte units
@pytest.mark.parametrize("rows", [13, 37, 401])
def test_matmul_row_groups(hip, knobs, n, rows):
    """Rows through launch_groups: row0 / nrows of a later launch.  cols = 3, inner = 3 of fresh terms: an 8 x 2 tile, one
    part of e, two column tiles, so a group of 8 rows is 2 workgroups.
    13 rows (2 groups): 1 + 1 launches at cap 2, one launch from cap 5 on;
    37 rows (5 groups, the last of 5 rows): 4 + 1 at cap 2, 2 + 1 at cap 5, one launch from cap 15 on;
    401 rows (51 groups, the last of 1 row): 51 at cap 2, 25 + 1 at 5, 7 + 2 at 15, 6 + 3 at 16, 2 + 3 at 48."""
    inner, cols = 3, 3
    a = rand_terms(n, rows * inner, 1, 2400 + rows)
    b = rand_terms(n, inner * cols, 1, 2410 + n)
    matmul_each_cap(hip, knobs, n, a, b, rows, inner, cols, caps=(2, 5) + CAPS)


@pytest.mark.parametrize("n", [65, 129])
@pytest.mark.parametrize("terms", [(1, 1), (2, 2)], ids=["fresh", "t2_2"])
def test_matmul_column_tiles_and_min_e(hip, knobs, n, terms):
    """Column tiles over launches (col0 / ncols / ctiles of a later launch) and the minE rule.  One row, inner = 300,
    tiles of 1 x 8 columns.
    cols = 37 (5 tiles, the last of 5 columns) at matmul_epart = 1: the cap lengthens the parts of e to
    minE = ceil(300 / cap) = 20, 19, 7, which leaves 15, 16, 43 parts: one tile a launch, 5 launches at every cap.
    cols = 37 with matmul_epart unset: the shape's own 2 to 8 parts; one launch, but 5 at cap 15 and 2 + 1 at cap 16
    for the (2, 2) terms at n = 129 (8 parts).
    cols = 401 (51 tiles, the last of 1 column) with matmul_epart unset, several tiles a launch:
    fresh, 2 parts a tile: 7 + 1 launches at cap 15 (7 tiles each), 6 + 1 at 16, 2 + 1 at 48;
    (2, 2) at n = 65, 3 parts: 10 + 1 at 15 and 16 (5 tiles each), 3 + 1 at 48;
    (2, 2) at n = 129, 8 parts: 51 at 15, 25 + 1 at 16, 8 + 1 at 48."""
    inner = 300
    for cols, epart in [(37, 1), (37, 0), (401, 0)]:
        a = rand_terms(n, inner, terms[0], 2500 + n)
        b = rand_terms(n, inner * cols, terms[1], 2510 + cols)
        knobs.set("matmul_epart", epart)
        matmul_each_cap(hip, knobs, n, a, b, 1, inner, cols)
    knobs.unset("matmul_epart")


# ------------------------------------------------------------------------------ the stream kernels' unit splits

def words(seed, count):
    return np.random.default_rng(seed).integers(0, 1 << 64, size=count, dtype=np.uint64)


TERMS = 3001                            # of every ragged output below


def ragged_sizes(seed, count, total=TERMS):
    """`count` sizes of 0 to 5 terms, empty ones among them, and one large element that brings the sum to `total`."""
    sizes = np.random.default_rng(seed).integers(0, 6, size=count)
    sizes[::7] = 0
    sizes[5] = 0
    sizes[5] = total - int(sizes.sum())                   # (the sum without element 5)
    assert sizes[5] > 256
    return sizes


# 1247: dL = 20, 10 units of 16 bytes a term; 1300: dL = 21, 21 units of 8 bytes.  A launch is cap * 256 units: 3840,
# 4096 or 12288, so terms straddle the launch boundaries (3840 is a multiple of 10 but not of 21).
STREAM_NS = [1247, 1300]
# 3001 terms: 30010 units at 1247: 7 + 3130 units at cap 15, 7 + 1338 at 16, 2 + 5434 at 48;
#             63021 units at 1300: 16 + 1581 at cap 15, 15 + 1581 at 16, 5 + 1581 at 48


@pytest.mark.parametrize("n", STREAM_NS)
def test_gather_planes_block_base(hip, knobs, n):
    """k_gather: block_base of a later launch.  Two planes of 1 and 3 terms, 3001 output elements, 1024 units a
    workgroup: 30 + 88 = 118 workgroups at 1247 (7 + 13 at cap 15, 7 + 6 at 16, 2 + 22 at 48), 62 + 185 = 247 at 1300
    (16 + 7, 15 + 7, 5 + 7).  The second plane starts inside a launch at every cap but 15 at 1247."""
    dl = (n + 63) // 64
    terms, count_in, count_out = [1, 3], 97, 3001
    planes = [words(n + 31 * j, count_in * t * dl) for j, t in enumerate(terms)]
    dev = [hip.upload(p) for p in planes]
    idx = np.random.default_rng(n).integers(0, count_in, size=count_out).astype(np.uint64)
    d_idx = hip.upload(idx)
    wants = [np_gather_uniform(planes[j], t, idx, dl) for j, t in enumerate(terms)]

    def call(cap):
        guarded = GuardedOutputs(hip, [x.size for x in wants])
        hip.gather_planes(n, dev, terms, count_in, count_out, d_idx, guarded.outs)
        torch.cuda.synchronize()
        guarded.check(wants, ("gather_planes", n, cap))

    each_cap(knobs, call)


@pytest.mark.parametrize("n", STREAM_NS)
@pytest.mark.parametrize("chunks", [1, 8, 16])
def test_gather_ragged_unit_base(hip, knobs, n, chunks):
    """k_gather_ragged: unit_base and the launch's own end (its total_units argument).  1000 source elements gathered
    in a random order, 3001 terms (STREAM_NS above for the launches).  ragged_c = 8 and 16: a workgroup owns 2048 or
    4096 units, more than the 3840 of a launch at cap 15 allow it, and exactly one launch's worth at cap 16 with ragged_c = 16."""
    dl = (n + 63) // 64
    sizes = ragged_sizes(n, 1000)
    src_off = csr(sizes)
    src = words(n + 7, TERMS * dl)
    idx = np.random.default_rng(n + 1).permutation(len(sizes))
    want, want_off = np_gather(src, src_off, idx, dl)
    d_src, d_off, d_idx = hip.upload(src), hip.upload(src_off), hip.upload(idx.astype(np.uint64))
    knobs.set("ragged_c", chunks)

    def call(cap):
        guarded = []

        def place(n_words):
            guarded.append(GuardedOutputs(hip, [n_words]))
            return guarded[0].outs[0]

        _, got_off = hip.gather_ragged(n, len(sizes), d_src, d_off, len(idx), d_idx, out=place)
        torch.cuda.synchronize()
        assert np.array_equal(hip.download(got_off), want_off), cap
        guarded[0].check([want], ("gather_ragged", n, chunks, cap))

    each_cap(knobs, call)


@pytest.mark.parametrize("n", STREAM_NS)
@pytest.mark.parametrize("chunks", [1, 8, 16])
def test_add_ragged_unit_base(hip, knobs, oracle, n, chunks):
    """k_add_ragged_flat through csgn_add_ragged_bounded without bounds (the CSR kernel): unit_base and the launch's own
    end.  400 pairs, 3001 terms of output, every pair's words from the oracle's add."""
    dl = (n + 63) // 64
    t1s = ragged_sizes(n + 2, 400, 1400)
    t2s = ragged_sizes(n + 3, 400, TERMS - 1400)[::-1].copy()
    off_l, off_r = csr(t1s), csr(t2s)
    left = rand_terms(n, 1, int(off_l[-1]), 2600 + n).ravel()
    right = rand_terms(n, 1, int(off_r[-1]), 2601 + n).ravel()
    want = np.concatenate([oracle.add(left[int(off_l[p]) * dl:int(off_l[p + 1]) * dl],
                                      right[int(off_r[p]) * dl:int(off_r[p + 1]) * dl])[0] for p in range(len(t1s))])
    assert want.size == TERMS * dl
    d_l, d_r, d_ol, d_or = hip.upload(left), hip.upload(right), hip.upload(off_l), hip.upload(off_r)
    knobs.set("ragged_c", chunks)

    def call(cap):
        guarded = GuardedOutputs(hip, [want.size])
        off_out = hip.empty_words(len(t1s) + 1)
        assert hip.lib.csgn_add_ragged_bounded(n, len(t1s), 0, 0, d_l.data_ptr(), d_ol.data_ptr(), d_r.data_ptr(),
                                               d_or.data_ptr(), guarded.outs[0].data_ptr(), off_out.data_ptr(), TERMS,
                                               hip.stream) == 0
        torch.cuda.synchronize()
        assert np.array_equal(hip.download(off_out), off_l + off_r), cap
        guarded.check([want], ("add_ragged", n, chunks, cap))

    each_cap(knobs, call)


@pytest.mark.parametrize("n", STREAM_NS)
def test_mul_1x1_stream_unit_base(hip, knobs, oracle, n):
    """k_and_stream through csgn_mul_uniform: u0 moves both operand pointers and the output pointer.  3001 pairs of
    fresh terms, every pair's words from the oracle's multiply."""
    dl = (n + 63) // 64
    left, right = rand_terms(n, TERMS, 1, 2700 + n), rand_terms(n, TERMS, 1, 2701 + n)
    want = np.concatenate([oracle.mul(n, left[p].ravel(), right[p].ravel())[0] for p in range(TERMS)])
    assert want.size == TERMS * dl
    assert hip.lib.csgn_mul_uniform_kernel(n, TERMS, 1, 1) == b"k_and_stream"
    d_l, d_r = hip.upload(left.ravel()), hip.upload(right.ravel())

    def call(cap):
        guarded = GuardedOutputs(hip, [want.size])
        hip.mul_uniform(n, TERMS, 1, 1, d_l, d_r, out=guarded.outs[0])
        torch.cuda.synchronize()
        guarded.check([want], ("mul 1x1", n, cap))

    each_cap(knobs, call)
