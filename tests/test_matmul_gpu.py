"""Products of encrypted bit matrices on the device (csgn_matmul), word for word against the definition of
include/csgn_hip.h (pinned against the reference and the oracle in tests/test_matmul_cpu.py), in every form the knob
matmul_form selects, through caller outputs of exactly the documented size between guard words; partial tiles, the split
of the inner dimension over workgroups, the 8-byte path of misaligned operands, decryptions.  Run with `pytest -m gpu` on
an MI355X."""
import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import GuardedOutputs, decrypt_bits, hip, rand_terms  # noqa: F401
from tests.model_matmul import np_matmul

pytestmark = pytest.mark.gpu

FORMS = (-1, 0, 1)
LAYOUTS = (False, True)


def transpose_b(b, inner, cols):
    """The same matrix in the layout Bt: element k * inner + e."""
    return np.ascontiguousarray(b.reshape(inner, cols, b.shape[1], b.shape[2]).transpose(1, 0, 2, 3)
                                .reshape(cols * inner, b.shape[1], b.shape[2]))


def offset_upload(hip, words, shift):
    """`words` on the device, `shift` words past a fresh tensor's start."""
    whole = hip.upload(np.concatenate([np.zeros(shift, dtype=np.uint64), words.ravel()]))
    return whole[shift:]


def run(hip, n, a, b, rows, inner, cols, transposed, want, shift=0):
    """One csgn_matmul into an output of exactly the documented size between guard words (tests/model.py,
    GuardedOutputs), checked word for word and for writes outside it."""
    da, db = offset_upload(hip, a, shift), offset_upload(hip, b, shift)
    guarded = GuardedOutputs(hip, [want.size], shift=shift)
    hip.matmul(n, rows, inner, cols, da, a.shape[1], db, b.shape[1], transposed, out=guarded.outs[0])
    torch.cuda.synchronize()
    guarded.check([want], (n, rows, inner, cols, a.shape[1], b.shape[1], transposed, shift))


def check_forms(hip, knobs, n, a, b, rows, inner, cols, forms=FORMS, layouts=LAYOUTS, shift=0):
    want = np_matmul(a, b, rows, inner, cols)              # the same words in both layouts (test_layouts_agree)
    bt = transpose_b(b, inner, cols) if True in layouts else None
    for transposed in layouts:
        for form in forms:
            knobs.set("matmul_form", form)
            run(hip, n, a, bt if transposed else b, rows, inner, cols, transposed, want, shift)


# 63: dL = 1; 65 and 1247: even dL, 16-byte units; 129: odd dL, the 8-byte kernel; 4096: 32 units a term
@pytest.mark.parametrize("n", [63, 65, 129, 1247, 4096])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 7, 1), (3, 1, 2), (2, 33, 3), (9, 5, 8), (1, 257, 1)],
                         ids=lambda s: "x".join(map(str, s)))
def test_matmul_words(hip, knobs, n, shape):
    rows, inner, cols = shape
    for ta, tb in [(1, 1), (2, 1), (1, 3), (3, 2)]:
        a = rand_terms(n, rows * inner, ta, 100 + n + ta)
        b = rand_terms(n, inner * cols, tb, 200 + n + tb)
        check_forms(hip, knobs, n, a, b, rows, inner, cols)


@pytest.mark.parametrize("rows,cols", [(1, 1), (257, 1), (1, 257), (4099, 1), (1, 4099), (65539, 1), (13, 11), (37, 111)])
def test_matmul_tiles_and_groups(hip, knobs, rows, cols):
    """Partial last tiles in rows, in columns and in both, and many tiles a launch, in every form.  Every shape here is
    ONE launch of the fused kernel; the launches the host cuts rows and column tiles into run in
    tests/test_launch_split_gpu.py."""
    n, inner = 65, 3
    a = rand_terms(n, rows * inner, 1, 300 + rows)
    b = rand_terms(n, inner * cols, 1, 310 + cols)
    check_forms(hip, knobs, n, a, b, rows, inner, cols)


@pytest.mark.parametrize("n", [63, 1247])
@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("terms", [(1, 1), (2, 2)], ids=["fresh", "t2_2"])
def test_matmul_inner_split(hip, knobs, n, rows, terms):
    """The range of e is split over workgroups, with a last part that is not full: by the shape's own rule, and at three
    part lengths of knob matmul_epart.  One row reads its operands straight from memory, two rows stage them in LDS."""
    inner = 5000
    a = rand_terms(n, rows * inner, terms[0], 400 + n + rows)
    b = rand_terms(n, inner, terms[1], 410 + n)
    check_forms(hip, knobs, n, a, b, rows, inner, 1)
    for epart in (1, 7, 64):
        knobs.set("matmul_epart", epart)
        check_forms(hip, knobs, n, a, b, rows, inner, 1, forms=(1,), layouts=(True,))
    knobs.unset("matmul_epart")


@pytest.mark.parametrize("n", [65, 1247])
def test_matmul_misaligned_operands_take_the_8_byte_path(hip, knobs, n):
    """Operands and output one word off a 16-byte boundary at even dL: the same words, by 8-byte units."""
    for rows, inner, cols, ta, tb in [(3, 5, 2, 1, 1), (9, 4, 9, 2, 3), (1, 300, 1, 1, 2)]:
        a = rand_terms(n, rows * inner, ta, 500 + n + rows)
        b = rand_terms(n, inner * cols, tb, 510 + n + cols)
        check_forms(hip, knobs, n, a, b, rows, inner, cols, shift=1)


# What matmul_fused (csgn_matmul.hip) plans for each case, by its own arithmetic.  ub = bytes a unit, U = units a term.
# Terms are sliced when 2 (ta + tb) U ub > 32768: fit = 32768 / (2 (ta + tb) ub) units; fit >= 16: chunks = ceil(U / fit)
# slices of KC = ceil(U / chunks) units, the last of U - (chunks - 1) KC; fit < 16: whole terms.  Then the tile doubles
# rows and columns in turn while (RT ta + CT tb) KC ub <= 32768.
#   (n, shift, ta, tb)       U  ub   fit  slices       tile (3,2,3) / (2,3,9)
#   (4096, 0, 17, 16)        32 16   31   16 + 16      2 x 2 / 2 x 4
#   (4096, 0, 40, 24)        32 16   16   16 + 16      2 x 2 / 2 x 2   (fit is the smallest slice allowed; the 2 x 2 tile
#                                                                       is 32768 bytes, the whole budget)
#   (4096, 1, 17, 16)        64  8   62   32 + 32      2 x 2 / 2 x 4
#   (5000, 0, 16, 14)        79  8   68   40 + 39      2 x 2 / 2 x 4   (a short last slice: kc < KC, the holes of stage())
#   (5000, 0, 31, 29)        79  8   34   27 + 27 + 25 2 x 2 / 2 x 2
#   (4096, 0, 40, 30)        32 16   14   whole terms  1 x 1: two rows of whole terms are 56320 bytes, so the unstaged
#                                                      kernel runs on a shape with rows, cols > 1
SLICED = [(4096, 0, 17, 16), (4096, 0, 40, 24), (4096, 1, 17, 16), (5000, 0, 16, 14), (5000, 0, 31, 29), (4096, 0, 40, 30)]


@pytest.mark.parametrize("shape", [(3, 2, 3), (2, 3, 9)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("case", SLICED, ids=lambda c: "n%d_s%d_%dx%d" % c)
def test_matmul_unit_slices_and_lds_fallback(hip, knobs, case, shape):
    """Terms too long for the LDS budget: slices of units (chunk, k0, and kc < KC on a short last slice), and the
    unstaged 1 x 1 tile once a slice would be under 16 units.  Every part of e is one element (EP = 1: the tile of one e
    nearly fills the budget)."""
    n, shift, ta, tb = case
    rows, inner, cols = shape
    a = rand_terms(n, rows * inner, ta, 800 + ta)
    b = rand_terms(n, inner * cols, tb, 810 + tb)
    check_forms(hip, knobs, n, a, b, rows, inner, cols, forms=(-1, 1), shift=shift)


def test_matmul_budget_stops_an_asymmetric_tile(hip, knobs):
    """ta = 1, tb = 20 at n = 4096 (U = 32, whole terms: 2 * 21 * 512 bytes fit): the tile grows 2 x 1, 2 x 2, 4 x 2
    (22528 bytes) and stops there, 4 x 4 being 43008; one e a part (EP = 1).  9 rows and columns: partial last tiles both
    ways."""
    n, rows, inner, cols = 4096, 9, 2, 9
    a = rand_terms(n, rows * inner, 1, 820)
    b = rand_terms(n, inner * cols, 20, 821)
    check_forms(hip, knobs, n, a, b, rows, inner, cols, forms=(-1, 1))


def test_matmul_unit_slices_over_several_launches(hip, knobs):
    """Slices and the host's launch split together: (31, 29) terms at n = 5000 are 3 slices, (2, 3, 9) is 3 parts of e
    and 5 column tiles of 2 x 2, so a tile is per_tile = eparts * chunks = 9 workgroups; at launch_blocks = 15 (knob:
    the workgroups of one launch) a launch takes one tile: 5 launches, col0 = 0, 2, 4, 6, 8, the last of one column."""
    n, rows, inner, cols = 5000, 2, 3, 9
    a = rand_terms(n, rows * inner, 31, 830)
    b = rand_terms(n, inner * cols, 29, 831)
    knobs.set("launch_blocks", 15)
    check_forms(hip, knobs, n, a, b, rows, inner, cols, forms=(1,))


def test_matmul_decrypts(hip, knobs, oracle):
    n, d, rows, inner, cols = 127, 8, 5, 9, 4
    dl = (n + 63) // 64
    key, _ = oracle.keygen(n, d, glibc_draws(701, 64 * d + 64))
    rng = np.random.default_rng(702)
    A = rng.integers(0, 2, (rows, inner)).astype(np.uint8)
    B = rng.integers(0, 2, (inner, cols)).astype(np.uint8)
    want = (A.astype(np.int64) @ B.astype(np.int64)) % 2

    def enc(bits, seed):
        flat = np.ascontiguousarray(bits).ravel()
        return oracle.encrypt_seq(n, key, flat, glibc_draws(seed, flat.size * (n + 2)))[0].reshape(flat.size, 1, dl)

    ea, eb, ebt = enc(A, 703), enc(B, 704), enc(B.T, 705)
    for form in FORMS:
        knobs.set("matmul_form", form)
        for operand, transposed in [(eb, False), (ebt, True)]:
            out = hip.matmul(n, rows, inner, cols, hip.upload(ea.ravel()), 1, hip.upload(operand.ravel()), 1, transposed)
            torch.cuda.synchronize()
            words = hip.download(out).reshape(rows * cols, inner, dl)
            assert np.array_equal(decrypt_bits(oracle, n, key, words).reshape(rows, cols).astype(np.int64), want), form


def test_matmul_dispatch_names(hip, knobs):
    lib = hip.lib
    knobs.unset("matmul_form")
    assert lib.csgn_matmul_kernel(1247, 256, 256, 256, 1, 1, 0) == b"k_matmul"
    knobs.set("matmul_form", 0)
    assert lib.csgn_matmul_kernel(1247, 256, 256, 256, 1, 1, 0) == b"composed"
    assert lib.csgn_matmul_kernel(1247, 0, 256, 256, 1, 1, 0) == b""
