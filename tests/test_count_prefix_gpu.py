"""Running counts of encrypted bits on the device (csgn_count_prefix), word for word against the definition of
include/csgn_hip.h (pinned against the oracle and the reference in tests/test_count_prefix_cpu.py), inclusive and
exclusive and in both input layouts, through caller outputs of exactly the documented size between guard words; the
split of the ranks over workgroups wherever the rows' borders fall, the LDS budget, several elements a workgroup, the
8-byte path of misaligned operands, the host's split into launches, graph capture, decryptions.  Run with
`pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import INVALID, GuardedOutputs, decrypt_bits, hip, rand_terms  # noqa: F401
from tests.model_count_prefix import block_words, np_count_prefix, prefix_offset, row_inputs, split_block

pytestmark = pytest.mark.gpu

SCANS = (False, True)


def offset_upload(hip, words, shift):
    """`words` on the device, `shift` words past a fresh tensor's start."""
    whole = hip.upload(np.concatenate([np.zeros(shift, dtype=np.uint64), words.ravel()]))
    return whole[shift:]


def upload_inputs(hip, x, count, g, layout, shift=0):
    if layout == "planes":
        planes = x.reshape(count, g, x.shape[1], -1)
        return [offset_upload(hip, np.ascontiguousarray(planes[:, i]), shift) for i in range(g)]
    return [offset_upload(hip, x, shift)]


def run(hip, n, count, g, x, js, exclusive, wants, layout, shift=0):
    """One csgn_count_prefix into blocks of exactly the documented sizes between guard words (tests/model.py,
    GuardedOutputs), checked word for word and for writes outside them."""
    ins = upload_inputs(hip, x, count, g, layout, shift)
    guarded = GuardedOutputs(hip, [w.size for w in wants], shift=shift)
    hip.count_prefix(n, count, g, x.shape[1], ins, js, exclusive=exclusive, outs=guarded.outs)
    torch.cuda.synchronize()
    guarded.check(wants, (n, count, g, x.shape[1], js, exclusive, layout, shift))


def layouts_of(g):
    return ("grouped", "planes") if 2 <= g <= 64 else ("grouped",)


def planes_of(g, js, exclusive):
    """The planes of js the scan has: 2^j within the last row's inputs."""
    return [j for j in js if (1 << j) <= g - (1 if exclusive else 0)]


class Reference:
    """x and the wanted blocks of both scans, computed once for a shape."""

    def __init__(self, n, count, g, t, js, seed):
        self.n, self.count, self.g, self.t = n, count, g, t
        self.x = rand_terms(n, count * g, t, seed)
        self.scans = []
        for ex in SCANS:
            have = planes_of(g, js, ex)
            if have:
                rows = np_count_prefix(self.x, g, have, ex)
                self.scans.append((ex, have, [block_words(r) for r in rows]))

    def check(self, hip, layouts=None, shift=0):
        for ex, js, wants in self.scans:
            for layout in layouts or layouts_of(self.g):
                run(hip, self.n, self.count, self.g, self.x, js, ex, wants, layout, shift)


WORDS = [(1, 1, 3, [0]), (3, 2, 1, [0, 1]), (2, 3, 2, [0, 1]), (5, 5, 2, [0, 1, 2]), (2, 8, 1, [0, 1, 2, 3]),
         (1, 9, 2, [1, 2]), (1, 12, 1, [2, 3]), (2, 64, 1, [0, 1, 6]), (1, 65, 1, [1, 6])]


# 63: dL = 1; 65 and 1247: even dL, 16-byte units; 129: odd dL, the 8-byte kernel; 4096: 32 units a term
@pytest.mark.parametrize("n", [63, 65, 129, 1247, 4096])
@pytest.mark.parametrize("shape", WORDS, ids=lambda s: "c%d_g%d_t%d_%s" % (s[0], s[1], s[2], "".join(map(str, s[3]))))
def test_prefix_words(hip, knobs, n, shape):
    """Every plane kind: the copy of the prefix (plane 0), pairs, subsets of 4 and 8, and plane 6: for g = 64 rows 0..62
    are ZERO and row 63 is one term (exclusive: the plane does not exist), for g = 65 the last row has 65 terms (exclusive:
    one); fresh and multi-term inputs (the digits)."""
    count, g, t, js = shape
    Reference(n, count, g, t, js, 100 + n + g).check(hip)


def test_prefix_offsets_of_the_words_case():
    """What the shapes above rest on: plane 6 of g = 64 is 63 ZERO rows and one term, of g = 65 64 ZERO rows and 65."""
    assert [prefix_offset(64, 1, 6, 0, r) for r in (62, 63, 64)] == [62, 63, 64]
    assert [prefix_offset(65, 1, 6, 0, r) for r in (63, 64, 65)] == [63, 64, 64 + 65]
    assert prefix_offset(65, 1, 6, 1, 65) == 65 and prefix_offset(64, 1, 6, 1, 64) == 0


def test_prefix_is_count_of_the_gathered_prefixes(hip, knobs):
    """Against the library itself: csgn_gather of the first n_r inputs of every element and csgn_count over them (both
    unchanged code) give row r's words."""
    n, count, g, t, js = 1247, 3, 8, 2, [0, 1, 2]
    dl = (n + 63) // 64
    x = rand_terms(n, count * g, t, 150)
    dx = hip.upload(x.ravel())
    for ex in SCANS:
        have = planes_of(g, js, ex)
        blocks = [hip.download(b) for b in hip.count_prefix(n, count, g, t, [dx], have, exclusive=ex)]
        torch.cuda.synchronize()
        for j, block in zip(have, blocks):
            rows = split_block(block, g, t, j, ex, count, dl)
            for r in range(g):
                nr = row_inputs(r, ex)
                if (1 << j) > nr:
                    assert rows[r].shape == (count, 1, dl) and not rows[r].any(), (ex, j, r)
                    continue
                idx = np.array([q * g + i for q in range(count) for i in range(nr)], dtype=np.uint64)
                prefix = hip.gather(n, count * g, dx, t, count * nr, index=hip.upload(idx))
                want = hip.download(hip.count(n, count, nr, t, [prefix], [j])[0])
                assert np.array_equal(rows[r].ravel(), want), (ex, j, r)


@pytest.mark.parametrize("shape", [(3, 60, 1, [1]), (1, 20, 2, [1, 2])], ids=["c3_g60_t1_1", "c1_g20_t2_12"])
def test_prefix_rank_split(hip, knobs, shape):
    """The ranks of a plane's rows laid end to end, cut by the shape's own rule and into parts of 1, 7, 59, 60 and 4096
    ranks.  g = 60 at plane 1, inclusive: rows of 0, 1, 3, ... ranks end at C(n + 1, 3) = 1, 4, 10, 20, 35, 56, 84 ...;
    parts of 7 begin inside a row (7, 14), exactly at a row's end (35 = 5 * 7, 56 = 8 * 7, 84 = 12 * 7) and one past it
    (21 = 20 + 1); parts of 1 put a border everywhere.  C(61, 3) = 35 990 = 5141 * 7 + 3 = 610 * 59 = 599 * 60 + 50: the
    last part would end past the last rank, or ends on it; 4096 is cut to the 1023 pairs the rank records hold."""
    count, g, t, js = shape
    ref = Reference(63, count, g, t, js, 200 + g)
    ref.check(hip)
    for cpart in (1, 7, 59, 60, 4096):
        knobs.set("count_cpart", cpart)
        ref.check(hip)
    knobs.unset("count_cpart")


# The cases of test_count_unit_slices_and_unstaged_inputs (tests/test_count_gpu.py) at plane 1, here against a budget
# of 49 152 bytes for the inputs of the LAST row: whole terms, slices of units, or nothing staged; a workgroup of an
# early part stages the few inputs below its last row, a late one all of them.
BUDGET = [(4096, 0, 24, 8), (4096, 1, 24, 8), (5000, 0, 24, 8), (2048, 0, 130, 2)]


@pytest.mark.parametrize("case", BUDGET, ids=lambda c: "n%d_s%d_g%d_t%d" % c)
def test_prefix_unit_slices_and_unstaged_inputs(hip, knobs, case):
    n, shift, g, t = case
    Reference(n, 1, g, t, [1], 300 + g).check(hip, shift=shift)


@pytest.mark.parametrize("n,count,t,js", [(63, 4099, 2, [0, 1, 2]), (63, 16401, 2, [0, 1, 2]), (1247, 4099, 1, [1, 2])],
                         ids=["n63_c4099", "n63_c16401", "n1247_c4099"])
def test_prefix_element_groups(hip, knobs, n, count, t, js):
    """Groups of 5 bits, thousands of them: a workgroup takes EG elements, doubled while every plane of EG elements
    stays within 16 384 units, the inputs fit the LDS budget and at least 2048 groups of elements remain.  Every count
    leaves a last group of ONE element."""
    Reference(n, count, 5, t, js, 250 + n).check(hip)


@pytest.mark.parametrize("n", [65, 1247])
def test_prefix_misaligned_operands_take_the_8_byte_path(hip, knobs, n):
    """Inputs and outputs one word off a 16-byte boundary at even dL: the same words, by 8-byte units."""
    for count, g, t, js in [(3, 5, 2, [1, 2]), (1, 64, 1, [1])]:
        Reference(n, count, g, t, js, 400 + n + g).check(hip, shift=1)


@pytest.mark.parametrize("cap", [15, 16, 255])
def test_prefix_launches(hip, knobs, cap):
    """The host cuts the call's workgroups, in order, into launches of launch_blocks (knob) each.  (7, 33, 1, [1]) at
    parts of 7 ranks is 7 * 855 workgroups inclusive (C(34, 3) = 5984 = 854 * 7 + 6): launches end inside a row and
    inside an element; by its own rule it is a few workgroups an element."""
    knobs.set("launch_blocks", cap)
    ref = Reference(63, 7, 33, 1, [1], 500)
    ref.check(hip)
    knobs.set("count_cpart", 7)
    ref.check(hip)
    knobs.unset("count_cpart")
    Reference(1247, 1, 40, 1, [0, 1], 501).check(hip, layouts=("grouped",))


def test_prefix_graph_capture_and_replay(hip):
    n, count, g, t, js = 1247, 37, 6, 2, [0, 1, 2]
    x = rand_terms(n, count * g, t, 600)
    want = [block_words(r) for r in np_count_prefix(x, g, js, False)]
    dx = hip.upload(x.ravel())
    outs = [hip.empty_words(w.size) for w in want]
    call = lambda: hip.count_prefix(n, count, g, t, [dx], js, outs=outs)  # noqa: E731
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        call()                                                        # warm-up outside the capture
    st.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        call()
    for o in outs:
        o.fill_(-1)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for j in range(len(want)):
        assert np.array_equal(hip.download(outs[j]), want[j]), j


def encrypt_bits(oracle, n, key, bits, seed):
    flat = np.ascontiguousarray(bits, dtype=np.uint8).ravel()
    dl = (n + 63) // 64
    return oracle.encrypt_seq(n, key, flat, glibc_draws(seed, flat.size * (n + 2)))[0].reshape(flat.size, 1, dl)


@pytest.mark.parametrize("g,layout", [(5, "grouped"), (5, "planes"), (12, "grouped"), (12, "planes")])
def test_prefix_decrypts(hip, knobs, oracle, g, layout):
    """Oracle-encrypted bits, every feasible plane, both scans: row r decrypts to the number of ones among its prefix.
    The plane layout is an integer as a UIntBatch hands it over: input i is the batch of bit i."""
    n, d = 127, 8
    dl = (n + 63) // 64
    key, _ = oracle.keygen(n, d, glibc_draws(900 + g, 64 * d + 64))
    if g == 5:
        values = np.arange(32, dtype=np.uint64)
    else:
        values = np.random.default_rng(g).integers(0, 1 << g, 20).astype(np.uint64)
        values[:2] = [0, (1 << g) - 1]
    count = len(values)
    bits = ((values[:, None] >> np.arange(g, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)   # [count, g]
    if layout == "planes":
        ins = [hip.upload(encrypt_bits(oracle, n, key, bits[:, i], 910 + i).ravel()) for i in range(g)]
    else:
        ins = [hip.upload(encrypt_bits(oracle, n, key, bits, 910).ravel())]
    for ex in SCANS:
        js = planes_of(g, range(7), ex)
        blocks = hip.count_prefix(n, count, g, 1, ins, js, exclusive=ex)
        torch.cuda.synchronize()
        rows = [split_block(hip.download(b), g, 1, j, ex, count, dl) for j, b in zip(js, blocks)]
        for r in range(g):
            got = np.zeros(count, dtype=np.uint64)
            for x, j in enumerate(js):
                got |= decrypt_bits(oracle, n, key, rows[x][r]).astype(np.uint64) << np.uint64(j)
            want = bits[:, :row_inputs(r, ex)].sum(axis=1).astype(np.uint64) & np.uint64((1 << len(js)) - 1)
            assert np.array_equal(got, want), (ex, r)


def test_prefix_argument_errors(hip):
    """With a device: what is refused is refused before anything is launched, and the outputs stay as they were."""
    lib = hip.lib
    n, count, g = 1247, 2, 8
    dl = (n + 63) // 64
    dx = hip.upload(rand_terms(n, count * g, 1, 700).ravel())
    guarded = GuardedOutputs(hip, [count * prefix_offset(g, 1, 1, 0, g) * dl])
    h_in = (C.c_void_p * 1)(dx.data_ptr())
    h_out = (C.c_void_p * 1)(guarded.outs[0].data_ptr())

    def call(n=n, count=count, g=g, t=1, ex=0, n_in=1, js=(1,), h_in=h_in, h_out=h_out):
        h_js = (C.c_uint64 * max(len(js), 1))(*js)
        return lib.csgn_count_prefix(n, count, g, t, ex, h_in, n_in, len(js), h_js, h_out, hip.stream)

    for bad in [dict(n=0), dict(count=0), dict(g=0), dict(t=0), dict(ex=2), dict(n_in=2), dict(js=()), dict(js=(4,)),
                dict(g=2, ex=1, js=(1,)), dict(js=(1, 1)), dict(h_in=None), dict(h_out=None),
                dict(h_in=(C.c_void_p * 1)(None)), dict(h_out=(C.c_void_p * 1)(None))]:
        assert call(**bad) == INVALID, bad
    torch.cuda.synchronize()
    untouched = np.full(guarded.sizes[0], 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    guarded.check([untouched], "refused calls")
    with pytest.raises(AssertionError):
        hip.count_prefix(n, count, g, 1, [dx], [4])
