"""Encrypted bits counted into encrypted integers on the device (csgn_count), word for word against the definition of
include/csgn_hip.h (pinned against the oracle and the reference in tests/test_count_cpu.py), in every form the knob
count_form selects and in both input layouts, through caller outputs of exactly the documented size between guard
words; the split of the combination ranks over workgroups, the LDS budget, the 8-byte path of misaligned operands, the
host's split into launches, decryptions.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import GuardedOutputs, decrypt_value, hip, rand_terms  # noqa: F401
from tests.model_count import np_count, popcount_planes

pytestmark = pytest.mark.gpu

FORMS = (-1, 0, 1)


def offset_upload(hip, words, shift):
    """`words` on the device, `shift` words past a fresh tensor's start."""
    whole = hip.upload(np.concatenate([np.zeros(shift, dtype=np.uint64), words.ravel()]))
    return whole[shift:]


def run(hip, n, count, g, x, js, wants, layout, shift=0):
    """One csgn_count into outputs of exactly the documented sizes between guard words (tests/model.py,
    GuardedOutputs), checked word for word and for writes outside them."""
    t = x.shape[1]
    if layout == "planes":
        planes = x.reshape(count, g, t, -1)
        ins = [offset_upload(hip, np.ascontiguousarray(planes[:, i]), shift) for i in range(g)]
    else:
        ins = [offset_upload(hip, x, shift)]
    guarded = GuardedOutputs(hip, [w.size for w in wants], shift=shift)
    hip.count(n, count, g, t, ins, js, outs=guarded.outs)
    torch.cuda.synchronize()
    guarded.check(wants, (n, count, g, t, js, layout, shift))


def layouts_of(g):
    return ("grouped", "planes") if 2 <= g <= 64 else ("grouped",)


def check_forms(hip, knobs, n, count, g, t, js, seed, forms=FORMS, layouts=None, shift=0, x=None, wants=None):
    """The reference once, then every form in every layout; returns (x, wants) for a caller that runs more knobs."""
    if x is None:
        x = rand_terms(n, count * g, t, seed)
        wants = np_count(x, g, js)
    for layout in layouts or layouts_of(g):
        for form in forms:
            knobs.set("count_form", form)
            run(hip, n, count, g, x, js, wants, layout, shift)
    return x, wants


WORDS = [(1, 1, 3, [0]), (3, 2, 1, [0, 1]), (2, 3, 2, [0, 1]), (5, 5, 2, [0, 1, 2]), (2, 8, 1, [0, 1, 2, 3]),
         (1, 9, 2, [1, 2]), (1, 12, 1, [2, 3]), (2, 64, 1, [0, 1, 6]), (1, 65, 1, [1, 6])]


# 63: dL = 1; 65 and 1247: even dL, 16-byte units; 129: odd dL, the 8-byte kernel; 4096: 32 units a term
@pytest.mark.parametrize("n", [63, 65, 129, 1247, 4096])
@pytest.mark.parametrize("shape", WORDS, ids=lambda s: "c%d_g%d_t%d_%s" % (s[0], s[1], s[2], "".join(map(str, s[3]))))
def test_count_words(hip, knobs, n, shape):
    """Every plane kind: the concatenation (plane 0), pairs, subsets of 4 and 8, and plane 6 -- subsets of 64 -- as one
    term (g = 64) and as 65 (g = 65); fresh and multi-term inputs (the digits)."""
    count, g, t, js = shape
    check_forms(hip, knobs, n, count, g, t, js, 100 + n + g)


@pytest.mark.parametrize("n", [63, 1247])
def test_count_rank_split(hip, knobs, n):
    """g = 200 at plane 1 is 19 900 subsets; the row i_1 = 0 holds 199 of them.  By the shape's own rule, and with parts
    of 1, 7, 199, 200 and 4096 ranks: a part starts inside a row of i_1, exactly at a row's end (199), one past it, and
    the last part would end past the last subset (19 900 = 2842 * 7 + 6; 4096 is cut to the 2048 subsets of 2 the
    subset table holds: ten parts, the last of 1468)."""
    count, g, t, js = 3, 200, 1, [1]
    x, wants = check_forms(hip, knobs, n, count, g, t, js, 200 + n)
    for cpart in (1, 7, 199, 200, 4096):
        knobs.set("count_cpart", cpart)
        check_forms(hip, knobs, n, count, g, t, js, 0, forms=(1,), x=x, wants=wants)
    knobs.unset("count_cpart")


def test_count_rank_split_with_digits(hip, knobs):
    """g = 40, t = 2, planes 1 and 2 at parts of 1000 ranks: plane 1 is one part of 780, plane 2 is 91 390 subsets of
    16 terms in 92 parts (the subset table holds 1024 subsets of 4); the digits and a split together."""
    knobs.set("count_cpart", 1000)
    check_forms(hip, knobs, 63, 1, 40, 2, [1, 2], 210, forms=(1,))
    knobs.unset("count_cpart")
    check_forms(hip, knobs, 63, 1, 40, 2, [1, 2], 210, forms=(-1,), layouts=("grouped",))


@pytest.mark.parametrize("n,count,t,js", [(63, 4099, 2, [0, 1, 2]), (63, 16401, 2, [0, 1, 2]), (1247, 4099, 1, [1, 2])],
                         ids=["n63_eg2", "n63_eg8", "n1247_eg2"])
def test_count_element_groups(hip, knobs, n, count, t, js):
    """Groups of 5 bits, thousands of them: a workgroup takes EG elements, doubled while every plane of EG elements is
    at most 16 384 units, the inputs fit the LDS budget and at least 2048 groups of elements remain.  n = 63, t = 2: the
    largest plane is 80 units an element; 4099 elements give EG = 2 (2050 groups; 4 would leave 1025), 16 401 give
    EG = 8 (2051 groups).  n = 1247, t = 1: 100 units, EG = 2.  Every count leaves a last group of ONE element."""
    check_forms(hip, knobs, n, count, 5, t, js, 250 + n)


# What count_fused (csgn_count.hip) plans for each case, by its own arithmetic.  ub = bytes a unit, U = units a term,
# gt = g * t input terms of an element.  The inputs are staged whole when gt U ub <= 57344; otherwise fit =
# 57344 / (gt ub) units; fit >= 16: chunks = ceil(U / fit) slices of KC = ceil(U / chunks) units, the last of
# U - (chunks - 1) KC; fit < 16: nothing is staged and every factor is read from memory.
#   (n, shift, g, t)         U  ub   gt   bytes    fit  slices         layouts
#   (4096, 0, 24, 8)         32 16   192  98304    18   16 + 16        both
#   (4096, 1, 24, 8)         64  8   192  98304    37   32 + 32        both
#   (5000, 0, 24, 8)         79  8   192  121344   37   27 + 27 + 25   both (a short last slice: kc < KC)
#   (2048, 0, 130, 2)        16 16   260  66560    13   unstaged       grouped
#   (2048, 0, 64, 4)         16 16   256  65536    14   unstaged       both (the plane layout's pointers, unstaged)
BUDGET = [(4096, 0, 24, 8), (4096, 1, 24, 8), (5000, 0, 24, 8), (2048, 0, 130, 2), (2048, 0, 64, 4)]


@pytest.mark.parametrize("case", BUDGET, ids=lambda c: "n%d_s%d_g%d_t%d" % c)
def test_count_unit_slices_and_unstaged_inputs(hip, knobs, case):
    """Inputs past the LDS budget at plane 1 (17 664 terms for g = 24, t = 8): slices of units (chunk, k0, and kc < KC
    on a short last slice), and factors read from memory once a slice would be under 16 units."""
    n, shift, g, t = case
    check_forms(hip, knobs, n, 1, g, t, [1], 300 + g, forms=(-1, 1), shift=shift)


@pytest.mark.parametrize("n", [65, 1247])
def test_count_misaligned_operands_take_the_8_byte_path(hip, knobs, n):
    """Inputs and outputs one word off a 16-byte boundary at even dL: the same words, by 8-byte units."""
    for count, g, t, js in [(3, 5, 2, [1, 2]), (1, 64, 1, [1])]:
        check_forms(hip, knobs, n, count, g, t, js, 400 + n + g, shift=1)


@pytest.mark.parametrize("cap", [15, 16, 255])
def test_count_launches(hip, knobs, cap):
    """The host cuts the call's workgroups, in order, into launches of launch_blocks (knob) each.  (7, 33, 1, [1]) is 7
    workgroups by its own rule (one launch) and 7 * 76 = 532 at parts of 7 ranks (528 = 75 * 7 + 3): launches end
    inside an element.  (1, 200, 1, [1]) at parts of 7 is 2843 workgroups of one element: 190, 178 and 12 launches."""
    knobs.set("launch_blocks", cap)
    x, wants = check_forms(hip, knobs, 63, 7, 33, 1, [1], 500, forms=(1,))
    knobs.set("count_cpart", 7)
    check_forms(hip, knobs, 63, 7, 33, 1, [1], 0, forms=(1,), x=x, wants=wants)
    check_forms(hip, knobs, 1247, 1, 200, 1, [1], 501, forms=(1,), layouts=("grouped",))


def encrypt_bits(oracle, n, key, bits, seed):
    flat = np.ascontiguousarray(bits, dtype=np.uint8).ravel()
    dl = (n + 63) // 64
    return oracle.encrypt_seq(n, key, flat, glibc_draws(seed, flat.size * (n + 2)))[0].reshape(flat.size, 1, dl)


@pytest.mark.parametrize("g,layout", [(5, "grouped"), (12, "grouped"), (12, "planes")])
def test_count_decrypts(hip, knobs, oracle, g, layout):
    """Oracle-encrypted bits, every feasible plane, in every form: the planes decrypt to the popcount.  The plane layout
    is a 12-bit integer as a UIntBatch hands it over: input i is the batch of bit i."""
    n, d = 127, 8
    dl = (n + 63) // 64
    key, _ = oracle.keygen(n, d, glibc_draws(700 + g, 64 * d + 64))
    if g == 5:
        values = np.arange(32, dtype=np.uint64)
    else:
        values = np.random.default_rng(g).integers(0, 1 << g, 20).astype(np.uint64)
        values[:2] = [0, (1 << g) - 1]
    count = len(values)
    js = [j for j in range(7) if (1 << j) <= g]
    bits = ((values[:, None] >> np.arange(g, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)   # [count, g]
    if layout == "planes":
        ins = [hip.upload(encrypt_bits(oracle, n, key, bits[:, i], 710 + i).ravel()) for i in range(g)]
    else:
        ins = [hip.upload(encrypt_bits(oracle, n, key, bits, 710).ravel())]
    for form in FORMS:
        knobs.set("count_form", form)
        outs = hip.count(n, count, g, 1, ins, js)
        torch.cuda.synchronize()
        words = [hip.download(o).reshape(count, -1, dl) for o in outs]
        assert np.array_equal(decrypt_value(oracle, n, key, words), popcount_planes(values, len(js))), form


def test_count_dispatch_names(hip, knobs):
    lib = hip.lib
    js = (C.c_uint64 * 2)(1, 2)
    knobs.unset("count_form")
    assert lib.csgn_count_kernel(1247, 256, 64, 1, 1, 2, js) == b"k_count"
    assert lib.csgn_count_kernel(1247, 256, 64, 1, 64, 2, js) == b"k_count"
    knobs.set("count_form", 0)
    assert lib.csgn_count_kernel(1247, 256, 64, 1, 1, 2, js) == b"composed"
    knobs.set("count_form", 1)
    assert lib.csgn_count_kernel(1247, 256, 64, 1, 1, 2, js) == b"k_count"
    assert lib.csgn_count_kernel(1247, 0, 64, 1, 1, 2, js) == b""
    assert lib.csgn_count_kernel(1247, 256, 3, 1, 1, 2, js) == b""
