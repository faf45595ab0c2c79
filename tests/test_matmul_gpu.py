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
    """Partial last tiles in rows, in columns and in both, many tiles a launch, and the row groups launch_groups deals
    out, in every form."""
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
