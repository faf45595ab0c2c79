"""The (slot + 1)-th row whose encrypted mask bit is set on the device (csgn_uint_nth), word for word against the
definition of include/csgn_hip.h (pinned against the reference and the oracle in tests/test_uint_nth_cpu.py): both mask
layouts, both unit sizes, the fresh path and the digit path, the host's split into launches, moved pointers, aliased
rows, graph capture; decryptions.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import GuardedOutputs, decrypt_bits, decrypt_value, encrypt_planes, hip, rand_terms, u64s  # noqa: F401
from tests.model_nth import label_terms, np_nth_fast, nth_terms
from tests.test_alignment_gpu import Case, Out, check_case, outs_for, place_all, views, words_of
from tests.test_uint_first_gpu import COMBOS, MAX_BYTES, label_set, terms_of

pytestmark = pytest.mark.gpu


def bits_of(g, t, slot, labels):
    return [] if labels is None else [i for i in range(64) if label_terms(g, t, slot, labels, i)]


def slots_of(g):
    return sorted({0, 1, g // 2, g - 1} & set(range(g)))


def operands(n, batch, g, tm, t, grouped, seed):
    """mask: ONE array words[batch * g, tm, dL] (grouped) or g arrays words[batch, tm, dL]; values: words[batch * g,
    t_j, dL].  Returns (mask, values, mask rows, value rows) -- the last two what the definition takes."""
    values = [rand_terms(n, batch * g, tj, seed + 100 + 11 * j) for j, tj in enumerate(t)]
    value_rows = [[d[r::g] for d in values] for r in range(g)]
    if grouped:
        mask = [rand_terms(n, batch * g, tm, seed)]
        mask_rows = [mask[0][r::g] for r in range(g)]
    else:
        mask = [rand_terms(n, batch, tm, seed + 3 * r) for r in range(g)]
        mask_rows = mask
    return mask, values, mask_rows, value_rows


def definition(mask_rows, value_rows, slot, valid, labels, bits):
    outs, stream, lab = np_nth_fast(mask_rows, value_rows, slot, labels)
    return [x.ravel() for x in outs] + ([stream.ravel()] if valid else []) + [lab[i].ravel() for i in bits]


def run(hip, n, batch, g, slot, mask, tm, values, valid, labels, bits, want=None):
    """The outputs, valid (when asked for) and the label planes, downloaded.  With `want` (the definition's words, one
    array per output) they are caller tensors of exactly those sizes between guard words, checked word for word and for
    writes outside them (tests/model.py, GuardedOutputs)."""
    dm = [hip.upload(p.ravel()) for p in mask]
    dv = [hip.upload(p.ravel()) for p in values]
    w = len(values)
    guarded = GuardedOutputs(hip, [x.size for x in want]) if want is not None else None
    if guarded:
        v = guarded.outs[w] if valid else False
        outs, got_valid, lab = hip.uint_nth(n, batch, g, slot, dm, tm, dv, terms_of(values), outs=guarded.outs[:w],
                                            valid=v, labels=labels, label_bits=bits,
                                            label_outs=guarded.outs[w + bool(valid):])
    else:
        outs, got_valid, lab = hip.uint_nth(n, batch, g, slot, dm, tm, dv, terms_of(values), valid=bool(valid),
                                            labels=labels, label_bits=bits)
    torch.cuda.synchronize()
    if guarded:
        return guarded.check(want, (g, slot, tm, terms_of(values), valid, labels))
    return ([hip.download(o) for o in outs] + ([hip.download(got_valid)] if valid else []) +
            [hip.download(o) for o in lab])


def out_bytes(n, batch, g, tm, slot, t, valid, labels, bits):
    Q = nth_terms(g, tm, slot, g)
    return batch * ((n + 63) // 64) * 8 * (Q * (sum(t) + bool(valid)) +
                                           sum(label_terms(g, tm, slot, labels, i) for i in bits))


# 63 and 129: odd dL, the 8-byte-unit kernel; 5 -> 6 rows: one -> two subset tables; t = 3 stops at g = 5
WORDS = [(n, g, tm, slot) for n in (63, 65, 129, 1247, 4096) for g in (1, 2, 3, 5, 6, 8) for tm in (1, 2, 3)
         for slot in slots_of(g) if tm < 3 or g <= 5]


@pytest.mark.parametrize("n,g,tm,slot", WORDS)
def test_nth_words(hip, n, g, tm, slot):
    rng = np.random.default_rng(g * 100 + n + tm)
    batch = 2
    ran = 0
    for ci, (w, valid, lmode, grouped) in enumerate(COMBOS):
        grouped = g == 1 or grouped
        labels = label_set(lmode, g)
        bits = bits_of(g, tm, slot, labels)
        if not (w or valid or bits):
            continue                                                  # no label plane from the slot on, nothing else
        t = [int(x) for x in rng.integers(1, 4, w)]
        if out_bytes(n, batch, g, tm, slot, t, valid, labels, bits) > MAX_BYTES:
            continue
        mask, values, mask_rows, value_rows = operands(n, batch, g, tm, t, grouped, 400 + 13 * ci + slot)
        run(hip, n, batch, g, slot, mask, tm, values, valid, labels, bits,
            definition(mask_rows, value_rows, slot, valid, labels, bits))
        ran += 1
    assert ran >= 4, (ran, g, tm, slot)         # the calls of width 0 and 1 always fit


@pytest.mark.parametrize("g,slot,grouped,n", [(11, 2, True, 63), (11, 2, False, 1247), (17, 14, True, 63),
                                              (17, 16, False, 129), (64, 61, False, 65), (64, 63, False, 1247)])
def test_nth_large_groups(hip, g, slot, grouped, n):
    """Fresh masks of 11 rows (three subset tables), of 17 (past the subset tables and the 16-bit subsets of the LDS
    list: the digit path) and of 64 in the plane layout (rows up to 63; Q = 2017 at slot 61, 1 at slot 63), one value
    plane, valid and the index labels."""
    batch, t = 2, [2]
    labels = label_set("index", g)
    bits = bits_of(g, 1, slot, labels)
    assert out_bytes(n, batch, g, 1, slot, t, True, labels, bits) <= MAX_BYTES
    assert (g, slot) != (64, 61) or nth_terms(g, 1, slot, g) == 2017
    mask, values, mask_rows, value_rows = operands(n, batch, g, 1, t, grouped, 800 + g)
    run(hip, n, batch, g, slot, mask, 1, values, True, labels, bits,
        definition(mask_rows, value_rows, slot, True, labels, bits))


@pytest.mark.parametrize("batch", [1, 257, 4099])
@pytest.mark.parametrize("tm", [1, 2])
def test_nth_batches(hip, batch, tm):
    """Partial last element groups and many groups a launch, on the fresh and on the digit path."""
    n, g, slot = 65, 4, 1
    labels = label_set("index", g)
    bits = bits_of(g, tm, slot, labels)
    mask, values, mask_rows, value_rows = operands(n, batch, g, tm, [1, 2], tm == 1, 900)
    run(hip, n, batch, g, slot, mask, tm, values, True, labels, bits,
        definition(mask_rows, value_rows, slot, True, labels, bits))


@pytest.mark.parametrize("n", [5248, 5184])
def test_nth_short_last_unit_slice(hip, n):
    """g = 10: two subset tables of 32 entries.  N = 5248 is 41 units of 16 bytes a term: 64 x 16 x 41 = 41 984 B pass
    the 32 768-byte budget, so subset_plan cuts the terms into two slices of 21 units, the last one 20 units long.
    N = 5184 (81 words, odd) is 81 units of 8 bytes: 64 x 8 x 81 = 41 472 B, slices of 41 and 40 units."""
    g, batch, slot, t = 10, 2, 3, [1, 2]
    labels = label_set("onehot", g)
    bits = bits_of(g, 1, slot, labels)
    for grouped in (True, False):
        mask, values, mask_rows, value_rows = operands(n, batch, g, 1, t, grouped, 1000 + grouped)
        run(hip, n, batch, g, slot, mask, 1, values, True, labels, bits,
            definition(mask_rows, value_rows, slot, True, labels, bits))


@pytest.mark.parametrize("n", [63, 1247])
@pytest.mark.parametrize("tm", [1, 2])
def test_nth_batch_split_over_launches(hip, knobs, n, tm):
    """Knob launch_blocks at 1, 2 and 5 cuts the batch into launches of 1, 2 and 5 element groups (one workgroup a
    group at these shapes), each from its own mask, value and output offsets.  389 elements, a prime: whatever the
    groups' size (2..64), the last group and so the last launch is not full.  The words are those of the one launch."""
    g, batch, slot = 3, 389, 1
    labels = label_set("index", g)
    bits = bits_of(g, tm, slot, labels)
    for grouped in (True, False):
        mask, values, mask_rows, value_rows = operands(n, batch, g, tm, [1, 2], grouped, 1100 + grouped)
        want = definition(mask_rows, value_rows, slot, True, labels, bits)
        knobs.unset("launch_blocks")
        run(hip, n, batch, g, slot, mask, tm, values, True, labels, bits, want)
        for blocks in (1, 2, 5):
            knobs.set("launch_blocks", blocks)
            run(hip, n, batch, g, slot, mask, tm, values, True, labels, bits, want)
    knobs.unset("launch_blocks")


def nth_case(hip, n, batch, g, tm, slot, t, seed):
    """The plane layout with valid and the index labels: five pointer classes."""
    labels = label_set("index", g)
    bits = bits_of(g, tm, slot, labels)
    mask, values, mask_rows, value_rows = operands(n, batch, g, tm, t, False, seed)
    want = definition(mask_rows, value_rows, slot, True, labels, bits)
    w = len(t)

    def call(moved):
        outs = outs_for(hip, want[:w], moved, "out")
        valid = Out(hip, want[w].size, "valid" in moved)
        lab = outs_for(hip, want[w + 1:], moved, "label_out")
        hip.uint_nth(n, batch, g, slot, place_all(hip, mask, moved, "mask"), tm, place_all(hip, values, moved, "values"),
                     t, outs=views(outs), valid=valid.view, labels=labels, label_bits=bits, label_outs=views(lab))
        return words_of(outs + [valid] + lab)

    return Case(["mask", "values", "out", "valid", "label_out"],
                {"mask": g, "values": w, "out": w, "label_out": len(bits)}, call, want)


@pytest.mark.parametrize("n", [1247, 4096])
@pytest.mark.parametrize("tm", [1, 2])
def test_nth_pointer_arrays(hip, n, tm):
    """Every pointer class one word off a 16-byte boundary, each alone, then the middle member of each array alone,
    then all of them: the 8-byte-unit kernel, the words of the aligned call (tests/test_alignment_gpu.py's method)."""
    check_case(nth_case(hip, n, 3, 4, tm, 1, [1, 2, 1], 1200 + n))


@pytest.mark.parametrize("tm", [1, 2])
def test_nth_aliased_rows(hip, tm):
    """The plane layout with every row the SAME batch (inputs may alias in any way)."""
    n, g, batch, slot = 1247, 5, 3, 2
    m = rand_terms(n, batch, tm, 1300)
    values = [rand_terms(n, batch * g, 2, 1301)]
    value_rows = [[values[0][r::g]] for r in range(g)]
    labels = label_set("onehot", g)
    bits = bits_of(g, tm, slot, labels)
    want = definition([m] * g, value_rows, slot, True, labels, bits)
    dm, dv = hip.upload(m.ravel()), [hip.upload(values[0].ravel())]
    guarded = GuardedOutputs(hip, [x.size for x in want])
    hip.uint_nth(n, batch, g, slot, [dm] * g, tm, dv, [2], outs=guarded.outs[:1], valid=guarded.outs[1], labels=labels,
                 label_bits=bits, label_outs=guarded.outs[2:])
    torch.cuda.synchronize()
    guarded.check(want, "aliased rows")


def test_nth_graph_capture_and_replay(hip):
    n, g, w, batch, slot = 1247, 6, 4, 37, 2
    t = [1 + j % 2 for j in range(w)]
    labels = label_set("index", g)
    bits = bits_of(g, 1, slot, labels)
    mask, values, mask_rows, value_rows = operands(n, batch, g, 1, t, True, 1400)
    want = definition(mask_rows, value_rows, slot, True, labels, bits)
    dm = [hip.upload(p.ravel()) for p in mask]
    dv = [hip.upload(p.ravel()) for p in values]
    outs = [hip.empty_words(x.size) for x in want]
    call = lambda: hip.uint_nth(n, batch, g, slot, dm, 1, dv, t, outs=outs[:w], valid=outs[w], labels=labels,  # noqa: E731
                                label_bits=bits, label_outs=outs[w + 1:])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        call()                                                        # warm-up outside the capture
    st.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        call()
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for j in range(len(want)):
        assert np.array_equal(hip.download(outs[j]), want[j]), j


# -- decryptions -------------------------------------------------------------------------------------------------------
def shaped(n, outs, batch):
    return [o.reshape(batch, -1, (n + 63) // 64) for o in outs]


def test_nth_decrypts(hip, oracle):
    """nthWhere for slots 0 .. g-1 returns the set rows in order, valid_s is count > s and the index labels name the
    row, over random masks that include all-zero groups, in both layouts; slot 0 decrypts as csgn_uint_first."""
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(701, 64 * d + 64))
    rng = np.random.default_rng(702)
    for g, w, batch, grouped in [(1, 3, 5, True), (3, 4, 100, True), (4, 8, 333, False), (8, 5, 40, True)]:
        bitsm = rng.integers(0, 2, (batch, g)).astype(np.uint64)
        bitsm[::3] = 0                                                # all-zero groups
        vals = rng.integers(0, 1 << w, (batch, g)).astype(np.uint64)
        if grouped:
            mask = [encrypt_planes(oracle, n, key, bitsm.ravel(), 1, 710 + g)[0]]
        else:
            mask = [encrypt_planes(oracle, n, key, bitsm[:, r].copy(), 1, 710 + g + r)[0] for r in range(g)]
        values = encrypt_planes(oracle, n, key, vals.ravel(), w, 730 + g)
        labels = label_set("index", g)
        set_rows = [[r for r in range(g) if m[r]] for m in bitsm]
        for slot in range(g):
            bits = bits_of(g, 1, slot, labels)
            got = shaped(n, run(hip, n, batch, g, slot, mask, 1, values, True, labels, bits), batch)
            nth = [rows[slot] if len(rows) > slot else None for rows in set_rows]
            assert [int(x) for x in decrypt_value(oracle, n, key, got[:w])] == \
                [0 if r is None else int(vals[e, r]) for e, r in enumerate(nth)], (g, slot)
            assert [int(b) for b in decrypt_bits(oracle, n, key, got[w])] == [int(len(rows) > slot) for rows in set_rows]
            index = np.zeros(batch, dtype=np.uint64)
            for i, words in zip(bits, got[w + 1:]):
                index |= decrypt_bits(oracle, n, key, words).astype(np.uint64) << np.uint64(i)
            assert [int(x) for x in index] == [r or 0 for r in nth], (g, slot)
            if slot == 0:
                dm = [hip.upload(p.ravel()) for p in mask]
                dv = [hip.upload(p.ravel()) for p in values]
                f_outs, f_any, _ = hip.uint_first(n, batch, g, dm, [1] * g, dv, [1] * w, any=True)
                torch.cuda.synchronize()
                first = shaped(n, [hip.download(o) for o in f_outs] + [hip.download(f_any)], batch)
                assert np.array_equal(decrypt_value(oracle, n, key, first[:w]), decrypt_value(oracle, n, key, got[:w]))
                assert np.array_equal(decrypt_bits(oracle, n, key, first[w]), decrypt_bits(oracle, n, key, got[w]))


def test_nth_argument_errors(hip):
    lib = hip.lib
    buf = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    out = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    ptrs = (C.c_void_p * 64)(*([buf.data_ptr()] * 64))
    nullp = (C.c_void_p * 64)(*([buf.data_ptr()] * 3 + [None] + [buf.data_ptr()] * 60))
    one = u64s([1] * 64)
    index = u64s(range(64))
    st = hip.stream

    def nth(n=1247, batch=1, g=4, slot=1, m=ptrs, nm=4, tm=1, w=4, d=ptrs, t=one, out=ptrs, valid=None, nl=0, L=None,
            lb=None, lo=None):
        return lib.csgn_uint_nth(n, batch, g, slot, m, nm, tm, w, d, t, out, valid, nl, L, lb, lo, st)

    lab = dict(nl=2, L=index, lb=u64s([0, 1]), lo=ptrs)
    assert nth(n=0) == -1                                             # n_bits
    assert nth(g=0) == -1 and nth(g=65) == -1 and nth(slot=4) == -1   # group, slot
    assert nth(nm=3) == -1 and nth(g=1, slot=0, nm=1, w=65) == -1     # n_mask; value width
    assert nth(nl=65) == -1 and nth(w=0) == -1                        # label planes; nothing asked for
    for arg in ("m", "d", "t", "out"):                                # host pointers
        assert nth(**{arg: None}) == -1, arg
    for arg in ("L", "lb", "lo"):
        assert nth(**dict(lab, **{arg: None})) == -1, arg
    assert nth(tm=0) == -1 and nth(t=u64s([1, 0, 1, 1])) == -1        # 0 terms
    assert nth(g=64, nm=64, slot=0) == -1                             # 2^62
    assert nth(**dict(lab, lb=u64s([1, 0]))) == -1 and nth(**dict(lab, lb=u64s([1, 2]))) == -1     # label bits
    for arg in ("m", "d", "out"):                                     # a null device pointer inside each host array
        assert nth(**{arg: nullp}) == -1, arg
        assert b"null device pointer" in lib.csgn_last_error(), arg
    assert nth(**dict(lab, nl=4, L=u64s([15] * 4), lb=u64s([0, 1, 2, 3]), lo=nullp)) == -1
    assert b"null device pointer" in lib.csgn_last_error()
    assert nth(g=27, nm=27, slot=0, w=1) == -2                        # 2^31 words
    assert nth(g=24, nm=24, slot=0, w=1, t=u64s([7])) == -2
    assert nth(g=27, nm=27, slot=0, w=0, valid=out.data_ptr()) == -2
    assert nth(g=8, nm=8, batch=1 << 50) == -2                        # batch
    assert nth(batch=0) == 0                                          # empty batch
    assert nth(batch=0, m=nullp, d=nullp, out=nullp, **dict(lab, lo=nullp)) == 0
    assert nth(batch=0, w=0, d=None, t=None, out=None, valid=out.data_ptr()) == 0
