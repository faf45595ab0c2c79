"""The first row whose encrypted mask bit is set on the device (csgn_uint_first), word for word against the definition
of include/csgn_hip.h (pinned against the reference and the oracle in tests/test_uint_first_cpu.py): both mask layouts,
both unit sizes, the fresh path and the digit path, the host's split into launches, moved pointers, aliased rows, graph
capture; decryptions; cross-checks against gates and gathers.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import (GATES, GuardedOutputs, const_term, decrypt_bits, decrypt_value, encrypt_planes, hip, rand_terms,
                         u64s)
from tests.model_first import first_terms, label_terms, np_first_fast
from tests.test_alignment_gpu import Case, Out, check_case, outs_for, place_all, views, words_of

pytestmark = pytest.mark.gpu

MAX_BYTES = 48 << 20                    # of one call's outputs: the numpy side, not the device, is the limit


def terms_of(planes):
    return [p.shape[1] for p in planes]


def label_set(mode, g):
    return {"none": None, "index": list(range(g)), "onehot": [1 << r for r in range(g)]}[mode]


def bits_of(s, labels):
    return [] if labels is None else [i for i in range(64) if label_terms(s, labels, i)]


def operands(n, batch, g, s, t, grouped, seed):
    """mask: ONE array words[batch * g, s, dL] (grouped) or g arrays words[batch, s_r, dL]; values: words[batch * g,
    t_j, dL].  Returns (mask, values, mask rows, value rows) -- the last two what the definition takes."""
    values = [rand_terms(n, batch * g, tj, seed + 100 + 11 * j) for j, tj in enumerate(t)]
    value_rows = [[d[r::g] for d in values] for r in range(g)]
    if grouped:
        assert len(set(s)) == 1
        mask = [rand_terms(n, batch * g, s[0], seed)]
        mask_rows = [mask[0][r::g] for r in range(g)]
    else:
        mask = [rand_terms(n, batch, sr, seed + 3 * r) for r, sr in enumerate(s)]
        mask_rows = mask
    return mask, values, mask_rows, value_rows


def definition(n, mask_rows, value_rows, any_, labels, bits):
    outs, stream, lab = np_first_fast(n, mask_rows, value_rows, labels)
    return [x.ravel() for x in outs] + ([stream.ravel()] if any_ else []) + [lab[i].ravel() for i in bits]


def run(hip, n, batch, g, mask, s, values, any_, labels, bits, want=None):
    """The outputs, any (when asked for) and the label planes, downloaded.  With `want` (the definition's words, one
    array per output) they are caller tensors of exactly those sizes between guard words, checked word for word and for
    writes outside them (tests/model.py, GuardedOutputs)."""
    dm = [hip.upload(p.ravel()) for p in mask]
    dv = [hip.upload(p.ravel()) for p in values]
    w = len(values)
    guarded = GuardedOutputs(hip, [x.size for x in want]) if want is not None else None
    if guarded:
        a = guarded.outs[w] if any_ else False
        outs, got_any, lab = hip.uint_first(n, batch, g, dm, s, dv, terms_of(values), outs=guarded.outs[:w], any=a,
                                            labels=labels, label_bits=bits, label_outs=guarded.outs[w + bool(any_):])
    else:
        outs, got_any, lab = hip.uint_first(n, batch, g, dm, s, dv, terms_of(values), any=bool(any_), labels=labels,
                                            label_bits=bits)
    torch.cuda.synchronize()
    if guarded:
        return guarded.check(want, (g, s, terms_of(values), any_, labels))
    return [hip.download(o) for o in outs] + ([hip.download(got_any)] if any_ else []) + [hip.download(o) for o in lab]


def out_bytes(n, batch, s, t, any_, labels, bits):
    Q = first_terms(s, len(s))
    return batch * ((n + 63) // 64) * 8 * (Q * (sum(t) + bool(any_)) + sum(label_terms(s, labels, i) for i in bits))


def mask_terms(tmode, g, rng):
    return [int(tmode)] * g if tmode in ("1", "2") else [int(x) for x in rng.integers(1, 4, g)]


# (value width, any, labels, grouped layout where the term counts allow it): every width with and without any, every
# label set with and without values, both layouts
COMBOS = [(0, True, "none", True), (0, False, "index", False), (0, True, "onehot", False), (0, False, "onehot", True),
          (1, False, "none", False), (1, True, "index", True), (1, True, "none", True), (1, False, "onehot", False),
          (8, True, "onehot", True), (8, False, "none", False), (8, False, "index", True),
          (64, True, "index", False), (64, False, "none", True)]

# 63 and 129: odd dL, the 8-byte-unit kernel; 5 -> 6 rows: one -> two subset tables.  Mixed terms at g = 8 reach
# 4^8 - 1 entries: 67 MB at N = 4096, so they stop at g = 6 there.
WORDS = [(n, g, tmode) for n in (63, 65, 129, 1247, 4096) for g in (1, 2, 3, 5, 6, 8) for tmode in ("1", "2", "mixed")
         if not (tmode == "mixed" and g == 8 and n == 4096)]


@pytest.mark.parametrize("n,g,tmode", WORDS)
def test_first_words(hip, n, g, tmode):
    rng = np.random.default_rng(g * 100 + n + len(tmode))
    batch = 2
    s = mask_terms(tmode, g, rng)
    ran = 0
    for ci, (w, any_, lmode, grouped) in enumerate(COMBOS):
        grouped = g == 1 or (grouped and len(set(s)) == 1)
        labels = label_set(lmode, g)
        bits = bits_of(s, labels)
        if not (w or any_ or bits):
            continue                                                  # g = 1: the index label 0 has no plane
        t = [int(x) for x in rng.integers(1, 4, w)]
        if out_bytes(n, batch, s, t, any_, labels, bits) > MAX_BYTES:
            continue
        mask, values, mask_rows, value_rows = operands(n, batch, g, s, t, grouped, 400 + 13 * ci)
        run(hip, n, batch, g, mask, s, values, any_, labels, bits, definition(n, mask_rows, value_rows, any_, labels, bits))
        ran += 1
    assert ran >= 4, (ran, s)           # the calls of width 0 and 1 always fit


@pytest.mark.parametrize("g,n", [(11, 63), (11, 1247), (17, 63), (17, 129)])
def test_first_large_groups(hip, g, n):
    """Fresh masks of 11 rows (three subset tables) and of 17 (past the subset tables and the 16-bit subsets of the LDS
    list: the digit path, Q = 131 071), one value plane, any and the index labels; grouped at 11, planes at 17."""
    batch, s, t = 2, [1] * g, [1]
    labels = label_set("index", g)
    bits = bits_of(s, labels)
    assert out_bytes(n, batch, s, t, True, labels, bits) <= MAX_BYTES
    mask, values, mask_rows, value_rows = operands(n, batch, g, s, t, g == 11, 800 + g)
    run(hip, n, batch, g, mask, s, values, True, labels, bits, definition(n, mask_rows, value_rows, True, labels, bits))


@pytest.mark.parametrize("batch", [1, 257, 4099])
@pytest.mark.parametrize("tmode", ["1", "mixed"])
def test_first_batches(hip, batch, tmode):
    """Partial last element groups and many groups a launch, on the fresh and on the digit path."""
    n, g = 65, 4
    s = [1] * g if tmode == "1" else [2, 1, 3, 1]
    labels = label_set("index", g)
    bits = bits_of(s, labels)
    mask, values, mask_rows, value_rows = operands(n, batch, g, s, [1, 2], tmode == "1", 900)
    run(hip, n, batch, g, mask, s, values, True, labels, bits, definition(n, mask_rows, value_rows, True, labels, bits))


@pytest.mark.parametrize("n", [5248, 5184])
def test_first_short_last_unit_slice(hip, n):
    """g = 10: two subset tables of 32 entries.  N = 5248 is 41 units of 16 bytes a term: 64 x 16 x 41 = 41 984 B pass
    the 32 768-byte budget, so subset_plan cuts the terms into two slices of 21 units, the last one 20 units long.
    N = 5184 (81 words, odd) is 81 units of 8 bytes: 64 x 8 x 81 = 41 472 B, slices of 41 and 40 units."""
    g, batch, s, t = 10, 2, [1] * 10, [1, 2]
    labels = label_set("onehot", g)
    bits = bits_of(s, labels)
    for grouped in (True, False):
        mask, values, mask_rows, value_rows = operands(n, batch, g, s, t, grouped, 1000 + grouped)
        run(hip, n, batch, g, mask, s, values, True, labels, bits,
            definition(n, mask_rows, value_rows, True, labels, bits))


@pytest.mark.parametrize("n", [63, 1247])
@pytest.mark.parametrize("tmode", ["1", "mixed"])
def test_first_batch_split_over_launches(hip, knobs, n, tmode):
    """Knob launch_blocks at 1, 2 and 5 cuts the batch into launches of 1, 2 and 5 element groups (one workgroup a
    group at these shapes), each from its own mask, value and output offsets.  389 elements, a prime: whatever the
    groups' size (2..64), the last group and so the last launch is not full.  The words are those of the one launch."""
    g, batch = 3, 389
    s = [1] * g if tmode == "1" else [2, 1, 3]
    labels = label_set("index", g)
    bits = bits_of(s, labels)
    for grouped in (tmode == "1", False):
        mask, values, mask_rows, value_rows = operands(n, batch, g, s, [1, 2], grouped, 1100 + grouped)
        want = definition(n, mask_rows, value_rows, True, labels, bits)
        knobs.unset("launch_blocks")
        run(hip, n, batch, g, mask, s, values, True, labels, bits, want)
        for blocks in (1, 2, 5):
            knobs.set("launch_blocks", blocks)
            run(hip, n, batch, g, mask, s, values, True, labels, bits, want)
    knobs.unset("launch_blocks")


def first_case(hip, n, batch, s, t, seed):
    """The plane layout with any and the index labels: five pointer classes."""
    g = len(s)
    labels = label_set("index", g)
    bits = bits_of(s, labels)
    mask, values, mask_rows, value_rows = operands(n, batch, g, s, t, False, seed)
    want = definition(n, mask_rows, value_rows, True, labels, bits)
    w = len(t)

    def call(moved):
        outs = outs_for(hip, want[:w], moved, "out")
        any_ = Out(hip, want[w].size, "any" in moved)
        lab = outs_for(hip, want[w + 1:], moved, "label_out")
        hip.uint_first(n, batch, g, place_all(hip, mask, moved, "mask"), s, place_all(hip, values, moved, "values"), t,
                       outs=views(outs), any=any_.view, labels=labels, label_bits=bits, label_outs=views(lab))
        return words_of(outs + [any_] + lab)

    return Case(["mask", "values", "out", "any", "label_out"],
                {"mask": g, "values": w, "out": w, "label_out": len(bits)}, call, want)


@pytest.mark.parametrize("n", [1247, 4096])
@pytest.mark.parametrize("tmode", ["1", "mixed"])
def test_first_pointer_arrays(hip, n, tmode):
    """Every pointer class one word off a 16-byte boundary, each alone, then the middle member of each array alone,
    then all of them: the 8-byte-unit kernel, the words of the aligned call (tests/test_alignment_gpu.py's method)."""
    check_case(first_case(hip, n, 3, [1, 1, 1, 1] if tmode == "1" else [2, 1, 3, 1], [1, 2, 1], 1200 + n))


@pytest.mark.parametrize("tmode", ["1", "2"])
def test_first_aliased_rows(hip, tmode):
    """The plane layout with every row the SAME batch (inputs may alias in any way): F_r = n * ... * n * m."""
    n, g, batch = 1247, 5, 3
    s = [int(tmode)] * g
    m = rand_terms(n, batch, s[0], 1300)
    values = [rand_terms(n, batch * g, 2, 1301)]
    value_rows = [[values[0][r::g]] for r in range(g)]
    labels = label_set("onehot", g)
    bits = bits_of(s, labels)
    want = definition(n, [m] * g, value_rows, True, labels, bits)
    dm, dv = hip.upload(m.ravel()), [hip.upload(values[0].ravel())]
    guarded = GuardedOutputs(hip, [x.size for x in want])
    hip.uint_first(n, batch, g, [dm] * g, s, dv, [2], outs=guarded.outs[:1], any=guarded.outs[1], labels=labels,
                   label_bits=bits, label_outs=guarded.outs[2:])
    torch.cuda.synchronize()
    guarded.check(want, "aliased rows")


def test_first_graph_capture_and_replay(hip):
    n, g, w, batch = 1247, 6, 4, 37
    s, t = [1] * g, [1 + j % 2 for j in range(w)]
    labels = label_set("index", g)
    bits = bits_of(s, labels)
    mask, values, mask_rows, value_rows = operands(n, batch, g, s, t, True, 1400)
    want = definition(n, mask_rows, value_rows, True, labels, bits)
    dm = [hip.upload(p.ravel()) for p in mask]
    dv = [hip.upload(p.ravel()) for p in values]
    outs = [hip.empty_words(x.size) for x in want]
    call = lambda: hip.uint_first(n, batch, g, dm, s, dv, t, outs=outs[:w], any=outs[w], labels=labels,  # noqa: E731
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


def first_set(masks, g):
    return [next((r for r in range(g) if m[r]), None) for m in masks]


def test_first_decrypts(hip, oracle):
    """firstWhere, any and firstIndex over random masks that include all-zero groups, in both layouts."""
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
        bits = bits_of([1] * g, labels)
        got = shaped(n, run(hip, n, batch, g, mask, [1] * g, values, True, labels, bits), batch)
        first = first_set(bitsm, g)
        assert any(r is None for r in first) and any(r not in (None, 0) for r in first) or g == 1
        assert [int(x) for x in decrypt_value(oracle, n, key, got[:w])] == \
            [0 if r is None else int(vals[e, r]) for e, r in enumerate(first)], g
        assert [int(b) for b in decrypt_bits(oracle, n, key, got[w])] == [int(r is not None) for r in first], g
        index = np.zeros(batch, dtype=np.uint64)
        for i, words in zip(bits, got[w + 1:]):
            index |= decrypt_bits(oracle, n, key, words).astype(np.uint64) << np.uint64(i)
        assert [int(x) for x in index] == [r or 0 for r in first], g


def test_any_matches_the_gates(hip, oracle):
    """any decrypts to what logicNot(prod of logicNot(m_r)) decrypts to, through the gate and multiply launchers."""
    n, d, g, batch = 127, 8, 4, 64
    key, _ = oracle.keygen(n, d, glibc_draws(741, 64 * d + 64))
    bitsm = np.random.default_rng(742).integers(0, 2, (batch, g)).astype(np.uint64)
    bitsm[:4] = 0
    mask = [encrypt_planes(oracle, n, key, bitsm[:, r].copy(), 1, 743 + r)[0] for r in range(g)]
    (any_,) = shaped(n, run(hip, n, batch, g, mask, [1] * g, [], True, None, []), batch)
    dm = [hip.upload(p.ravel()) for p in mask]
    nots = [hip.gate_uniform(n, GATES["not"], batch, m, 1) for m in dm]
    prod, terms = nots[0], 2
    for x in nots[1:]:
        prod = hip.mul_uniform(n, batch, terms, 2, prod, x)
        terms *= 2
    via = hip.gate_uniform(n, GATES["not"], batch, prod, terms)
    torch.cuda.synchronize()
    (via,) = shaped(n, [hip.download(via)], batch)
    want = [bool(m.any()) for m in bitsm]
    assert list(decrypt_bits(oracle, n, key, any_)) == want
    assert list(decrypt_bits(oracle, n, key, via)) == want


def test_trivial_one_hot_mask_matches_gather(hip, oracle):
    """A trivially encrypted one-hot mask (one ONE / ZERO term per row) gives what a gather of the chosen rows gives."""
    n, d, g, w, batch = 1247, 16, 6, 5, 50
    key, _ = oracle.keygen(n, d, glibc_draws(751, 64 * d + 64))
    rng = np.random.default_rng(752)
    chosen = rng.integers(0, g, batch)
    vals = rng.integers(0, 1 << w, batch * g).astype(np.uint64)
    mask = [np.stack([const_term(n, int(r == chosen[e])) for e in range(batch) for r in range(g)]).reshape(batch * g, 1, -1)]
    values = encrypt_planes(oracle, n, key, vals, w, 753)
    got = decrypt_value(oracle, n, key, shaped(n, run(hip, n, batch, g, mask, [1] * g, values, False, None, []), batch))
    dv = [hip.upload(p.ravel()) for p in values]
    idx = (np.arange(batch) * g + chosen).astype(np.uint64)
    gouts = hip.gather_planes(n, dv, [1] * w, batch * g, batch, hip.upload(idx))
    torch.cuda.synchronize()
    via_gather = decrypt_value(oracle, n, key, shaped(n, [hip.download(o) for o in gouts], batch))
    assert np.array_equal(got, via_gather)
    assert np.array_equal(got, vals[idx.astype(np.int64)])


def test_first_argument_errors(hip):
    lib = hip.lib
    buf = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    out = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    ptrs = (C.c_void_p * 64)(*([buf.data_ptr()] * 64))
    nullp = (C.c_void_p * 64)(*([buf.data_ptr()] * 3 + [None] + [buf.data_ptr()] * 60))
    one = u64s([1] * 64)
    index = u64s(range(64))
    st = hip.stream

    def first(n=1247, batch=1, g=4, m=ptrs, nm=4, s=one, w=4, d=ptrs, t=one, out=ptrs, any_=None, nl=0, L=None, lb=None,
              lo=None):
        return lib.csgn_uint_first(n, batch, g, m, nm, s, w, d, t, out, any_, nl, L, lb, lo, st)

    lab = dict(nl=2, L=index, lb=u64s([0, 1]), lo=ptrs)
    assert first(n=0) == -1                                           # n_bits
    assert first(g=0) == -1 and first(g=65) == -1                     # group
    assert first(nm=3) == -1 and first(g=1, nm=1, w=65) == -1         # n_mask; value width
    assert first(nl=65) == -1 and first(w=0) == -1                    # label planes; nothing asked for
    for arg in ("m", "s", "d", "t", "out"):                           # host pointers
        assert first(**{arg: None}) == -1, arg
    for arg in ("L", "lb", "lo"):
        assert first(**dict(lab, **{arg: None})) == -1, arg
    assert first(s=u64s([1, 0, 1, 1])) == -1 and first(t=u64s([1, 0, 1, 1])) == -1     # 0 terms
    assert first(g=64, nm=64) == -1                                   # 2^62
    assert first(**dict(lab, lb=u64s([1, 0]))) == -1 and first(**dict(lab, lb=u64s([1, 2]))) == -1     # label bits
    assert first(nm=1, s=u64s([1, 1, 2, 1])) == -1                    # the grouped layout takes one count
    for arg in ("m", "d", "out"):                                     # a null device pointer inside each host array
        assert first(**{arg: nullp}) == -1, arg
        assert b"null device pointer" in lib.csgn_last_error(), arg
    assert first(**dict(lab, nl=4, L=u64s([15] * 4), lb=u64s([0, 1, 2, 3]), lo=nullp)) == -1
    assert b"null device pointer" in lib.csgn_last_error()
    assert first(g=27, nm=27, w=1) == -2                              # 2^31 words
    assert first(g=24, nm=24, w=1, t=u64s([7])) == -2
    assert first(g=27, nm=27, w=0, any_=out.data_ptr()) == -2
    assert first(g=8, nm=8, batch=1 << 50) == -2                      # batch
    assert first(batch=0) == 0                                        # empty batch
    assert first(batch=0, m=nullp, d=nullp, out=nullp, **dict(lab, lo=nullp)) == 0
    assert first(batch=0, w=0, d=None, t=None, out=None, any_=out.data_ptr()) == 0
