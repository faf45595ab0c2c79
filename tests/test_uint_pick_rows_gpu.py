"""Encrypted arrays whose rows differ in size read at encrypted indices on the device (csgn_uint_pick_rows), word for word
against the definition of include/csgn_hip.h (tests/model_pick_rows.py's np_pick_rows_fast, pinned against the reference
and the oracle in tests/test_uint_pick_rows_cpu.py), in both forms the knob uint_pick_rows_form selects with the form's
name asserted, every run into caller outputs between guard words: the shapes, the row tables, the index planes, the
widths and the batches; the host's split into launches; operands 8 bytes off a 16-byte boundary; the chain from
csgn_uint_write's outputs with every decryption; graph capture.  Run with `pytest -m gpu` on an MI355X.

No test of this file passes an argument it expects to be refused: refusals are csgn_uint_pick_rows_check's, a host
function, and are tested without a GPU (tests/test_uint_pick_rows_args_cpu.py).  Every shape here is asserted ACCEPTED by
that check before it is launched."""
import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import GuardedOutputs, decrypt_value, encrypt_planes, hip, rand_terms, u64s  # noqa: F401
from tests.model_pick_rows import clear_pick_rows, np_pick_rows_fast, out_terms, write_shaped
from tests.model_write import np_write_fast

pytestmark = pytest.mark.gpu

MAX_BYTES = 48 << 20                    # of one call's outputs

N_BITS = [63, 65, 129, 1247]            # 63 and 129: odd dL, the 8-byte-unit kernel
SHAPES = [(1, 1), (1, 2), (2, 3), (3, 5), (3, 8), (4, 16), (7, 128)]


def mixed_terms(v, seed):
    """index planes of 1..3 terms, not all fresh"""
    s = [int(x) for x in np.random.default_rng(seed).integers(1, 4, v)]
    if s == [1] * v:
        s[0] = 2
    return s


def tables(s, n, seed):
    """The row tables by name: what csgn_uint_write leaves, random 1..5, constant, one row of 40 terms among rows of 1."""
    rng = np.random.default_rng(seed)
    lone = [1] * n
    lone[n // 2] = 40
    return {"written": write_shaped(s, n), "random": [int(x) for x in rng.integers(1, 6, n)], "constant": [3] * n,
            "lone": lone}


def out_bytes(n_bits, s, T, batch):
    return batch * sum(out_terms(s, t) for t in T) * ((n_bits + 63) // 64) * 8


def operands(n_bits, s, T, batch, seed):
    index = [rand_terms(n_bits, batch, sk, seed + 7 * k + sk) for k, sk in enumerate(s)]
    arrays = [rand_terms(n_bits, batch, sum(t), seed + 500 + 13 * j) for j, t in enumerate(T)]
    return index, arrays


def upload(hip, words, shift):
    """The words on the device, `shift` words (8 bytes each) past a fresh tensor's 16-byte-aligned start."""
    whole = hip.upload(np.concatenate([np.zeros(shift, dtype=np.uint64), words.ravel()]))
    return whole[shift:]


def accepted(hip, n_bits, batch, s, T):
    flat = [t for plane in T for t in plane]
    return hip.lib.csgn_uint_pick_rows_check(n_bits, batch, len(s), u64s(s), len(T[0]), len(T), u64s(flat)) == 0


def form_name(hip, n_bits, batch, s, T):
    flat = [t for plane in T for t in plane]
    return hip.lib.csgn_uint_pick_rows_kernel(n_bits, batch, len(s), u64s(s), len(T[0]), len(T), u64s(flat))


def run(hip, n_bits, index, arrays, T, want, shift=0):
    """index[k]: words[batch, s_k, dL], arrays[j]: words[batch, A_j, dL] (host arrays).  The outputs are caller tensors of
    exactly the documented sizes between guard words, checked word for word against `want` and for writes outside them
    (tests/model.py, GuardedOutputs)."""
    s = [p.shape[1] for p in index]
    assert accepted(hip, n_bits, index[0].shape[0], s, T)
    dx = [upload(hip, p, shift) for p in index]
    da = [upload(hip, p, shift) for p in arrays]
    guarded = GuardedOutputs(hip, [x.size for x in want], shift=shift)
    if shift:
        assert all(t.data_ptr() % 16 == 8 for t in dx + da + guarded.outs)
    hip.uint_pick_rows(n_bits, index[0].shape[0], dx, s, len(T[0]), da, T, outs=guarded.outs)
    torch.cuda.synchronize()
    return guarded.check(want, (n_bits, s, len(T[0]), len(T), shift))


def check_forms(hip, knobs, n_bits, index, arrays, T, shift=0):
    """Both forms against one computation of the definition's words."""
    want = [x.ravel() for x in np_pick_rows_fast(n_bits, index, arrays, T)]
    assert sum(x.nbytes for x in want) <= MAX_BYTES
    s = [p.shape[1] for p in index]
    for form in (0, 1):
        knobs.set("uint_pick_rows_form", form)
        assert form_name(hip, n_bits, index[0].shape[0], s, T) == (b"k_uint_pick_rows" if form else b"composed")
        run(hip, n_bits, index, arrays, T, want, shift)                 # GuardedOutputs.check asserts every word
    return want


def word_cases(n_bits, v, n):
    """(s, T, batch) at one shape: fresh index planes and mixed ones of 1..3 terms ((7, 128): fresh only, batch 1); per
    index the four kinds of table on one plane each (w = 1), three planes of DIFFERENT tables (w = 3) and, up to
    v = 3, 64 planes that deal the four kinds (w = 64).  The batch is 3, or fewer where three would pass 48 MB."""
    cases = []
    big = (v, n) == (7, 128)
    for s in ([1] * v,) if big else ([1] * v, mixed_terms(v, 100 * v + n + n_bits)):
        kinds = tables(s, n, 17 * v + n)
        planes = [[t] for t in kinds.values()] + [[kinds["written"], kinds["random"], kinds["lone"]]]
        if v <= 3:
            planes.append([list(kinds.values())[j % 4] for j in range(64)])
        for T in planes:
            one = out_bytes(n_bits, s, T, 1)
            if one > MAX_BYTES:
                T, one = T[:1], out_bytes(n_bits, s, T[:1], 1)          # three planes of (7, 128) at N = 1247: one
            batch = 1 if big else min(3, MAX_BYTES // one)
            assert batch >= 1, ("one element passes 48 MB", n_bits, s, n)
            cases.append((s, T, batch))
    return cases


@pytest.mark.parametrize("n_bits", N_BITS)
@pytest.mark.parametrize("v,n", SHAPES)
def test_pick_rows_words(hip, knobs, n_bits, v, n):
    widths = set()
    for i, (s, T, batch) in enumerate(word_cases(n_bits, v, n)):
        widths.add(len(T))
        index, arrays = operands(n_bits, s, T, batch, 300 + i)
        check_forms(hip, knobs, n_bits, index, arrays, T)
    assert {1, 3} <= widths or (v, n) == (7, 128)
    assert 64 in widths or v > 3


@pytest.mark.parametrize("batch", [1, 3, 4099])
def test_pick_rows_batches(hip, knobs, batch):
    """(v, n) = (2, 3) at N = 65, three planes of different tables.  A workgroup owns 64 elements at most (ReadTile), so
    4099 elements are 65 groups of workgroups or more, the last one short."""
    n_bits, n = 65, 3
    for s in ([1, 1], [1, 2]):
        kinds = tables(s, n, 5)
        T = [kinds["written"], kinds["random"], kinds["lone"]]
        index, arrays = operands(n_bits, s, T, batch, 700)
        check_forms(hip, knobs, n_bits, index, arrays, T)


@pytest.mark.parametrize("n_bits,tmode", [(63, "1"), (1247, "1"), (1247, "mixed")])
def test_pick_rows_batch_split_over_launches(hip, knobs, n_bits, tmode):
    """Knob launch_blocks lowers the workgroups of one launch, so launch_groups cuts the batch into several launches, each
    with its own index, array and output offsets (the arrays advance by e0 * A_j terms, the outputs by e0 * Tout_j).  325
    elements are 6 groups of at most 64 or more: at one workgroup a launch the host issues at least 6 launches, at two
    at least 3; the last is not full."""
    v, n, batch = 2, 3, 325
    s = [1] * v if tmode == "1" else [2, 1]
    kinds = tables(s, n, 9)
    T = [kinds["written"], kinds["lone"], kinds["random"]]
    index, arrays = operands(n_bits, s, T, batch, 800)
    want = [x.ravel() for x in np_pick_rows_fast(n_bits, index, arrays, T)]
    assert sum(x.nbytes for x in want) <= MAX_BYTES
    knobs.set("uint_pick_rows_form", 1)
    assert form_name(hip, n_bits, batch, s, T) == b"k_uint_pick_rows"
    for blocks in (1, 2, 7):
        knobs.set("launch_blocks", blocks)
        run(hip, n_bits, index, arrays, T, want)


@pytest.mark.parametrize("n_bits", [65, 1247])
def test_pick_rows_misaligned_operands(hip, knobs, n_bits):
    """Every operand and output pointer 8 bytes off a 16-byte boundary: dL is even, so only the pointers send the call
    down the 8-byte-unit path."""
    for s in ([1, 1, 1], [2, 1, 3]):
        kinds = tables(s, 5, 11)
        T = [kinds["written"], kinds["random"], kinds["lone"]]
        index, arrays = operands(n_bits, s, T, 3, 900)
        check_forms(hip, knobs, n_bits, index, arrays, T, shift=1)


@pytest.mark.parametrize("v", [1, 2, 3])
def test_pick_rows_reads_what_write_wrote(hip, knobs, oracle, v):
    """csgn_uint_write's output tensors go straight into csgn_uint_pick_rows, in both forms: every (write index, read
    index) pair in one batch decrypts to the value where the indices agree, to the array's own row elsewhere and to 0
    where the read index is >= n; and the words are the model's of the model's write."""
    n_bits, d, w = 127, 8, 3
    key, _ = oracle.keygen(n_bits, d, glibc_draws(570 + v, 64 * d + 64))
    rng = np.random.default_rng(v)
    for n in sorted({1, (1 << v) - 1, 1 << v}):
        wr = np.repeat(np.arange(1 << v, dtype=np.uint64), 1 << v)
        rd = np.tile(np.arange(1 << v, dtype=np.uint64), 1 << v)
        batch = len(wr)
        table = rng.integers(0, 1 << w, (batch, n)).astype(np.uint64)
        vals = rng.integers(0, 1 << w, batch).astype(np.uint64)
        wi = encrypt_planes(oracle, n_bits, key, wr, v, 580 + v)
        ri = encrypt_planes(oracle, n_bits, key, rd, v, 583 + v)
        value = encrypt_planes(oracle, n_bits, key, vals, w, 585 + v)
        a = encrypt_planes(oracle, n_bits, key, table.ravel(), w, 590 + w + n)
        T = [write_shaped([1] * v, n)] * w
        written = np_write_fast(n_bits, wi, value, a, n)
        want = [x.ravel() for x in np_pick_rows_fast(n_bits, ri, written, T)]
        d_written = hip.uint_write(n_bits, batch, [hip.upload(p.ravel()) for p in wi], [1] * v, n,
                                   [hip.upload(p.ravel()) for p in value], [1] * w,
                                   [hip.upload(p.ravel()) for p in a], [1] * w)
        d_ri = [hip.upload(p.ravel()) for p in ri]
        assert accepted(hip, n_bits, batch, [1] * v, T)
        for form in (0, 1):
            knobs.set("uint_pick_rows_form", form)
            assert form_name(hip, n_bits, batch, [1] * v, T) == (b"k_uint_pick_rows" if form else b"composed")
            guarded = GuardedOutputs(hip, [x.size for x in want])
            hip.uint_pick_rows(n_bits, batch, d_ri, [1] * v, n, d_written, T, outs=guarded.outs)
            torch.cuda.synchronize()
            outs = guarded.check(want, ("chain", v, n, form))
            dl = (n_bits + 63) // 64
            got = decrypt_value(oracle, n_bits, key, [o.reshape(batch, -1, dl) for o in outs])
            for e in range(batch):
                after = [int(x) for x in table[e]]
                if wr[e] < n:
                    after[int(wr[e])] = int(vals[e])
                assert int(got[e]) == clear_pick_rows(n, after, int(rd[e])), (v, n, form, e)


def test_pick_rows_graph_capture_and_replay(hip, knobs):
    """A warm call fills the calling thread's table cache; the same call is then captured (nothing is uploaded under
    capture) and replayed into outputs that hold the fill again."""
    n_bits, v, n, batch = 1247, 5, 32, 5
    s = [1] * v
    kinds = tables(s, n, 21)
    T = [kinds["written"]] * 4 + [kinds["random"], kinds["lone"]]
    index, arrays = operands(n_bits, s, T, batch, 1400)
    want = [x.ravel() for x in np_pick_rows_fast(n_bits, index, arrays, T)]
    assert sum(x.nbytes for x in want) <= MAX_BYTES
    knobs.set("uint_pick_rows_form", 1)
    assert accepted(hip, n_bits, batch, s, T) and form_name(hip, n_bits, batch, s, T) == b"k_uint_pick_rows"
    dx = [hip.upload(p.ravel()) for p in index]
    da = [hip.upload(p.ravel()) for p in arrays]
    st = torch.cuda.Stream()
    warm = [hip.empty_words(x.size) for x in want]
    with torch.cuda.stream(st):
        hip.uint_pick_rows(n_bits, batch, dx, s, n, da, T, warm)               # warm-up outside the capture
    st.synchronize()
    guarded = GuardedOutputs(hip, [x.size for x in want])                      # fresh outputs for the replay
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        hip.uint_pick_rows(n_bits, batch, dx, s, n, da, T, guarded.outs)
    torch.cuda.synchronize()
    fresh = GuardedOutputs(hip, [x.size for x in want])
    for whole, again in zip(guarded.whole, fresh.whole):
        whole.copy_(again)                                                     # every word back to the fill
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    guarded.check(want, "replay")
