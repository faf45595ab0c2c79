"""GPU parity tests: every result comes from libcsgn_hip.so through the C ABI
(include/csgn_hip.h) on cuda:0 and is compared bit-for-bit with the CPU oracle and with
the committed golden vectors (tests/golden/, generated from the genuine reference).

Run with `pytest -m gpu` on an MI355X.  Nothing here reads /root/reference.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle.binding import canonical_bitlen, glibc_draws
from tests.model import config5, csr, explicit_randomness, hip, make_key, planted, random_circuit

pytestmark = pytest.mark.gpu

KAT_PATH = os.path.join(os.path.dirname(__file__), "golden", "csgn_kat.json")
# extra entropy for the *_fuzz tests (0 = the committed cases): CSGN_FUZZ_SEED=k python -m pytest -k fuzz
FUZZ_SEED = int(os.environ.get("CSGN_FUZZ_SEED", "0"))

CONTEXTS = [(1247, 16), (4096, 32), (65, 4), (64, 4), (63, 4), (130, 5), (129, 3)]


def words(hex_list):
    return np.array([int(h, 16) for h in hex_list], dtype=np.uint64)


@pytest.fixture(scope="module")
def kat():
    with open(KAT_PATH) as f:
        return json.load(f)


# ------------------------------------------------------------------------------ harness

def test_library_is_the_hip_one(hip):
    import csgn_amd
    assert os.path.exists(csgn_amd.lib_path())
    assert hip.lib.csgn_abi_version() == 1


@pytest.mark.parametrize("n", [1247, 4096, 65, 63])
def test_synth_and_digest_match_oracle(hip, oracle, n):
    nw = 12345 * oracle.default_len(n)
    dev = hip.synth_fill(0xABCDEF, n, 0, nw)
    host = oracle.synth(0xABCDEF, n, 0, nw)
    assert np.array_equal(hip.download(dev), host)
    assert hip.digest(dev) == oracle.digest(host)
    assert hip.digest(dev, first_index=77) == oracle.digest(host, 77)
    # offset window
    dev2 = hip.synth_fill(0xABCDEF, n, 1000 * oracle.default_len(n), 500)
    assert np.array_equal(hip.download(dev2), host[1000 * oracle.default_len(n):][:500])


# ----------------------------------------------------------------------------- multiply

@pytest.mark.parametrize("n,d", CONTEXTS)
@pytest.mark.parametrize("t1,t2", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (7, 1), (1, 7), (32, 32),
                                   (33, 65), (5, 300), (300, 5), (129, 130)])
@pytest.mark.parametrize("batch", [1, 3])
def test_mul_uniform_matches_oracle(hip, oracle, n, d, t1, t2, batch):
    dl = oracle.default_len(n)
    L = oracle.synth(1000 + t1, n, 0, batch * t1 * dl)
    R = oracle.synth(2000 + t2, n, 0, batch * t2 * dl)
    out = hip.download(hip.mul_uniform(n, batch, t1, t2, hip.upload(L), hip.upload(R)))
    per = t1 * t2 * dl
    assert out.size == batch * per
    for b in range(batch):
        want, _ = oracle.mul(n, L[b * t1 * dl:(b + 1) * t1 * dl], R[b * t2 * dl:(b + 1) * t2 * dl])
        assert want.size == per
        assert np.array_equal(out[b * per:(b + 1) * per], want), (n, t1, t2, b)


@pytest.mark.parametrize("flat,xcd", [(0, 1), (0, 0), (2, 1), (4, 0), (8, 1)])
def test_mul_flat_variants_do_not_change_results(hip, oracle, knobs, flat, xcd):
    knobs.set("CSGN_MUL_FLAT", str(flat))
    knobs.set("CSGN_MUL_XCD", str(xcd))
    n, dl = 1247, 20
    for (t1, t2, batch) in [(100, 77, 2), (64, 128, 3), (257, 33, 1), (3, 5, 7), (1, 9, 5)]:
        L = oracle.synth(5, n, 0, batch * t1 * dl)
        R = oracle.synth(6, n, 0, batch * t2 * dl)
        out = hip.download(hip.mul_uniform(n, batch, t1, t2, hip.upload(L), hip.upload(R)))
        per = t1 * t2 * dl
        for b in range(batch):
            want, _ = oracle.mul(n, L[b * t1 * dl:(b + 1) * t1 * dl], R[b * t2 * dl:(b + 1) * t2 * dl])
            assert np.array_equal(out[b * per:(b + 1) * per], want)


@pytest.mark.parametrize("n,t1,t2,batch,kernel", [
    (1247, 16, 16, 20000, "k_touch+k_mul_flat"),   # rows of 160 units: two units per lane behind the touch; 102 MB of operands: two cuts
    (1247, 32, 32, 9000, "k_touch+k_mul_flat"),    # 92 MB of operands, 1 Ki-term products: 32 MB cuts (three launches)
    (1247, 16, 4, 40000, "k_mul_tiled"),           # thin, rows of 40 units: 64-thread workgroups, 8 rows per tile
    (1247, 4, 16, 40000, "k_mul_tiled"),           # rows of 160 units: the tiled kernel's default block
    (4096, 4, 4, 30000, "k_mul_tiled"),            # 128-unit rows, 4 rows: default block
    (4096, 64, 4, 6000, "k_mul_tiled"),            # 128-unit rows, tall: 128-thread workgroups, 8 rows per tile
    (4096, 64, 2, 6000, "k_mul_flat"),             # two-term rows stay with the flat kernel (two units per lane)
    (1247, 8, 8, 40000, "k_mul_tiled"),            # a whole small pair per 128-thread workgroup
    (1247, 4, 4, 100000, "k_mul_tiled"),           # 40-unit rows, 4 rows per pair
    (1247, 64, 2, 20000, "k_mul_flat"),            # rows of 20 units stay with the flat kernel (tall: two units per lane)
    (1247, 16, 8, 20000, "k_touch+k_mul_flat"),    # taller than 8 rows: touch + flat, two units per lane
])
def test_mul_default_dispatch_of_streaming_small_shapes(hip, oracle, knobs, n, t1, t2, batch, kernel):
    """The dispatch rules round 3 re-tuned (mul_plan: units per lane by row length, tiled kernel from 128-unit rows,
    touch cuts of 32 / 64 MB) on batches large enough to be STREAMS (>= 4 MB of operands, several cuts): the default
    dispatch gives the words the other kernel gives, and sampled pairs -- first, last, and the pairs either side of
    every cut -- equal the oracle."""
    import torch
    dl = oracle.default_len(n)
    assert hip.lib.csgn_mul_uniform_kernel(n, batch, t1, t2).decode() == kernel
    L = hip.synth_fill(81, n, 0, batch * t1 * dl)
    R = hip.synth_fill(82, n, 0, batch * t2 * dl)
    out = hip.mul_uniform(n, batch, t1, t2, L, R).clone()
    knobs.set("mul_flat", 1 if kernel == "k_mul_tiled" else -1)          # the other kernel family, no touch
    knobs.set("mul_touch", 0)
    other = hip.mul_uniform(n, batch, t1, t2, L, R)
    assert torch.equal(out, other)
    op_bytes = (t1 + t2) * dl * 8
    picks = {0, 1, batch // 2, batch - 2, batch - 1}
    for cut_mb in (32, 64):
        step = (cut_mb << 20) // op_bytes
        for k in range(1, 4):
            picks |= {min(batch - 1, max(0, k * step + dpair)) for dpair in (-1, 0, 1)}
    hl, hr = hip.download(L), hip.download(R)
    per = t1 * t2 * dl
    for b in sorted(picks):
        want, _ = oracle.mul(n, hl[b * t1 * dl:(b + 1) * t1 * dl], hr[b * t2 * dl:(b + 1) * t2 * dl])
        assert np.array_equal(hip.download(out[b * per:(b + 1) * per]), want), (n, t1, t2, b)


@pytest.mark.parametrize("n,d", CONTEXTS)
@pytest.mark.parametrize("t1,t2", [(1, 2), (3, 5), (33, 65), (5, 300), (129, 130)])
def test_mul_tiled_kernel_matches_oracle(hip, oracle, knobs, n, d, t1, t2):
    """The LDS-tiled kernel (CSGN_MUL_FLAT=-1; also the ragged path) on every context."""
    knobs.set("CSGN_MUL_FLAT", "-1")
    dl = oracle.default_len(n)
    batch = 2
    L = oracle.synth(1000 + t1, n, 0, batch * t1 * dl)
    R = oracle.synth(2000 + t2, n, 0, batch * t2 * dl)
    out = hip.download(hip.mul_uniform(n, batch, t1, t2, hip.upload(L), hip.upload(R)))
    per = t1 * t2 * dl
    for b in range(batch):
        want, _ = oracle.mul(n, L[b * t1 * dl:(b + 1) * t1 * dl], R[b * t2 * dl:(b + 1) * t2 * dl])
        assert np.array_equal(out[b * per:(b + 1) * per], want), (n, t1, t2, b)


@pytest.mark.parametrize("n,d", CONTEXTS)
@pytest.mark.parametrize("touch", [0, 1, 3])
def test_mul_flat_kernel_with_touch_matches_oracle(hip, oracle, knobs, n, d, touch):
    """The flat kernel forced on every context, with and without the operand touch pass (which
    only reads: results cannot depend on it)."""
    knobs.set("CSGN_MUL_FLAT", "1")
    knobs.set("CSGN_MUL_TOUCH", str(touch))
    dl = oracle.default_len(n)
    batch = 2
    for (t1, t2) in [(1, 2), (3, 5), (33, 65), (5, 300), (129, 130)]:
        L = oracle.synth(1000 + t1, n, 0, batch * t1 * dl)
        R = oracle.synth(2000 + t2, n, 0, batch * t2 * dl)
        out = hip.download(hip.mul_uniform(n, batch, t1, t2, hip.upload(L), hip.upload(R)))
        per = t1 * t2 * dl
        for b in range(batch):
            want, _ = oracle.mul(n, L[b * t1 * dl:(b + 1) * t1 * dl], R[b * t2 * dl:(b + 1) * t2 * dl])
            assert np.array_equal(out[b * per:(b + 1) * per], want), (n, t1, t2, b)


def test_mul_touch_chunking_across_64mb_of_operands(hip, oracle):
    """Default dispatch on a batch whose operands exceed one touch chunk (64 MB): 30 000 pairs of
    16x8 terms at N=1247 are cut after pair 17 476; pairs on both sides of the cut, the ends and a
    random sample are compared with the oracle."""
    n, dl, t1, t2, batch = 1247, 20, 16, 8, 30000
    assert hip.lib.csgn_mul_uniform_kernel(n, batch, t1, t2).decode() == "k_touch+k_mul_flat"
    L = hip.synth_fill(11, n, 0, batch * t1 * dl)
    R = hip.synth_fill(12, n, 0, batch * t2 * dl)
    out = hip.mul_uniform(n, batch, t1, t2, L, R)
    hl, hr, ho = hip.download(L), hip.download(R), hip.download(out)
    per = t1 * t2 * dl
    cut = (64 << 20) // ((t1 + t2) * dl * 8)
    picks = {0, 1, batch - 1, cut - 1, cut, cut + 1, 2 * cut - 1} | set(
        np.random.default_rng(5).integers(0, batch, 200).tolist())
    for b in sorted(p for p in picks if 0 <= p < batch):
        want, _ = oracle.mul(n, hl[b * t1 * dl:(b + 1) * t1 * dl], hr[b * t2 * dl:(b + 1) * t2 * dl])
        assert np.array_equal(ho[b * per:(b + 1) * per], want), b


@pytest.mark.parametrize("n,t1,t2,batch", [(1247, 100, 77, 200), (4096, 40, 40, 104), (1247, 33, 65, 300),
                                           (128, 64, 64, 2100)])
def test_mul_streaming_launches_default_dispatch(hip, oracle, n, t1, t2, batch):
    """Launches with >= 4 MB of operands take the touch + flat pair by default; every product of
    the batch is compared with the oracle."""
    assert hip.lib.csgn_mul_uniform_kernel(n, batch, t1, t2).decode() == "k_touch+k_mul_flat"
    dl = oracle.default_len(n)
    L = hip.synth_fill(21, n, 0, batch * t1 * dl)
    R = hip.synth_fill(22, n, 0, batch * t2 * dl)
    ho = hip.download(hip.mul_uniform(n, batch, t1, t2, L, R))
    hl, hr = hip.download(L), hip.download(R)
    per = t1 * t2 * dl
    for b in range(batch):
        want, _ = oracle.mul(n, hl[b * t1 * dl:(b + 1) * t1 * dl], hr[b * t2 * dl:(b + 1) * t2 * dl])
        assert np.array_equal(ho[b * per:(b + 1) * per], want), (n, t1, t2, b)


def test_mul_kernel_forms_fuzz(hip, oracle, knobs):
    """80 random (N, t1, t2, batch, arena slots) cases: the default dispatch, the LDS-tiled kernel
    and the flat kernel with and without the touch pass must produce identical words; every eighth
    case is also compared with the oracle."""
    import torch
    rng = np.random.default_rng(77 + FUZZ_SEED)
    for it in range(80):
        n = int(rng.choice([63, 64, 65, 130, 1247, 1300, 2048, 4096]))
        dl = oracle.default_len(n)
        t1, t2 = (int(x) for x in rng.integers(1, 200, size=2))
        if it % 7 == 0:
            t1, t2 = int(rng.integers(1, 4)), int(rng.integers(1, 1500))
        batch = int(rng.integers(1, 24))
        slots = int(rng.choice([0, 0, 1, 3])) if batch > 3 else 0
        L = hip.synth_fill(2 * it, n, 0, batch * t1 * dl)
        R = hip.synth_fill(2 * it + 1, n, 0, batch * t2 * dl)
        outs = []
        for env in ({}, {"CSGN_MUL_FLAT": "-1"}, {"CSGN_MUL_FLAT": "1", "CSGN_MUL_TOUCH": "3"},
                    {"CSGN_MUL_FLAT": "2", "CSGN_MUL_TOUCH": "0", "CSGN_MUL_XCD": "0"}):
            for k in ("CSGN_MUL_FLAT", "CSGN_MUL_TOUCH", "CSGN_MUL_XCD"):
                knobs.unset(k)
            for k, v in env.items():
                knobs.set(k, v)
            outs.append(hip.mul_uniform(n, batch, t1, t2, L, R, out_slots=slots).clone())
        for o in outs[1:]:
            assert torch.equal(outs[0], o), (n, t1, t2, batch, slots)
        if it % 8 == 0 and slots == 0:
            hl, hr, ho = hip.download(L), hip.download(R), hip.download(outs[0])
            per = t1 * t2 * dl
            for b in {0, batch - 1}:
                want, _ = oracle.mul(n, hl[b * t1 * dl:(b + 1) * t1 * dl], hr[b * t2 * dl:(b + 1) * t2 * dl])
                assert np.array_equal(ho[b * per:(b + 1) * per], want), (n, t1, t2, b)


@pytest.mark.parametrize("m,ti,nt", [(1, 64, 0), (2, 16, 1), (4, 7, 0), (8, 64, 1), (4, 1000, 1)])
def test_mul_tiled_tuning_knobs_do_not_change_results(hip, oracle, knobs, m, ti, nt):
    knobs.set("CSGN_MUL_FLAT", "-1")
    knobs.set("CSGN_MUL_M", str(m))
    knobs.set("CSGN_MUL_TI", str(ti))
    knobs.set("CSGN_MUL_NT", str(nt))
    n = 1247
    dl = 20
    for (t1, t2) in [(100, 77), (64, 128), (257, 33)]:
        L = oracle.synth(5, n, 0, 2 * t1 * dl)
        R = oracle.synth(6, n, 0, 2 * t2 * dl)
        out = hip.download(hip.mul_uniform(n, 2, t1, t2, hip.upload(L), hip.upload(R)))
        per = t1 * t2 * dl
        for b in range(2):
            want, _ = oracle.mul(n, L[b * t1 * dl:(b + 1) * t1 * dl], R[b * t2 * dl:(b + 1) * t2 * dl])
            assert np.array_equal(out[b * per:(b + 1) * per], want)


def test_mul_fresh_batch_65536(hip, oracle):
    """BASELINE config 2: batch=65536 independent 1x1 products at N=1247."""
    n, batch, dl = 1247, 65536, 20
    L = oracle.synth(11, n, 0, batch * dl)
    R = oracle.synth(12, n, 0, batch * dl)
    out = hip.download(hip.mul_uniform(n, batch, 1, 1, hip.upload(L), hip.upload(R)))
    assert np.array_equal(out, L & R)
    # spot-check against the oracle's 1x1 path
    for b in (0, 1, 4097, 65535):
        want, _ = oracle.mul(n, L[b * dl:(b + 1) * dl], R[b * dl:(b + 1) * dl])
        assert np.array_equal(out[b * dl:(b + 1) * dl], want)


def test_mul_arena_slots(hip, oracle):
    """Streaming a batch through a fixed arena: pair p lands in slot p % slots, later pairs
    overwrite earlier ones (SURVEY 8d streaming rule)."""
    n, dl, t1, t2, batch, slots = 1247, 20, 40, 50, 10, 4
    L = oracle.synth(21, n, 0, batch * t1 * dl)
    R = oracle.synth(22, n, 0, batch * t2 * dl)
    out = hip.download(hip.mul_uniform(n, batch, t1, t2, hip.upload(L), hip.upload(R), out_slots=slots))
    per = t1 * t2 * dl
    assert out.size == slots * per
    survivors = {p % slots: p for p in range(batch)}          # last writer per slot
    for slot, p in survivors.items():
        want, _ = oracle.mul(n, L[p * t1 * dl:(p + 1) * t1 * dl], R[p * t2 * dl:(p + 1) * t2 * dl])
        assert np.array_equal(out[slot * per:(slot + 1) * per], want)


@pytest.mark.parametrize("n,d", [(1247, 16), (4096, 32), (63, 4), (130, 5)])
def test_mul_ragged_matches_oracle(hip, oracle, n, d):
    dl = oracle.default_len(n)
    t1s = [1, 0, 3, 17, 1, 64, 2, 0, 5]
    t2s = [1, 4, 0, 9, 33, 65, 2, 0, 1]
    offL, offR = csr(t1s), csr(t2s)
    L = oracle.synth(31, n, 0, int(offL[-1]) * dl)
    R = oracle.synth(32, n, 0, int(offR[-1]) * dl)
    out, off_out = hip.mul_ragged(n, hip.upload(L), hip.upload(offL), hip.upload(R), hip.upload(offR))
    out, off_out = hip.download(out), hip.download(off_out)
    assert np.array_equal(off_out, csr([a * b for a, b in zip(t1s, t2s)]))   # the gathered term counts
    for b, (t1, t2) in enumerate(zip(t1s, t2s)):
        got = out[int(off_out[b]) * dl:int(off_out[b + 1]) * dl]
        if t1 == 0 or t2 == 0:
            assert got.size == 0
            continue
        want, _ = oracle.mul(n, L[int(offL[b]) * dl:int(offL[b + 1]) * dl],
                             R[int(offR[b]) * dl:int(offR[b + 1]) * dl])
        assert np.array_equal(got, want), b


def test_mul_rejects_bad_arguments(hip):
    from csgn_amd.capi import CsgnError, check
    x = hip.empty_words(64)
    with pytest.raises(CsgnError):      # N == 0
        check(hip.lib.csgn_mul_uniform(0, 1, 1, 1, x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, 0))
    with pytest.raises(CsgnError):      # null operand
        check(hip.lib.csgn_mul_uniform(1247, 1, 1, 1, 0, x.data_ptr(), x.data_ptr(), 0, 0))
    with pytest.raises(CsgnError):      # term larger than the kernels stage
        check(hip.lib.csgn_mul_uniform(1 << 20, 1, 1, 1, x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, 0))


def test_c_abi_refuses_bad_arguments_before_any_launch(hip):
    """Every compute entry point of include/csgn_hip.h turns a null pointer, N = 0, an oversized N, a bad generator
    or a bad circuit id into a non-zero status with a message -- checked on the host before anything is
    launched, so a caller's mistake can never become a device fault."""
    import ctypes as C
    import torch
    from csgn_amd import capi
    L = hip.lib
    x = hip.empty_words(4096)
    b = torch.zeros(4096, dtype=torch.uint8, device=hip.device)
    X, B, S, n = x.data_ptr(), b.data_ptr(), hip.stream, 1247
    rng = hip.rng_from_seed(1, 8)
    bad_rng = hip.rng_from_seed(1, 8)
    bad_rng.rounds = 7
    plan = (C.c_uint64 * 4)()
    cases = {
        "mul N=0": lambda: L.csgn_mul_uniform(0, 1, 1, 1, X, X, X, 0, S),
        "mul N too large": lambda: L.csgn_mul_uniform(1 << 40, 1, 1, 1, X, X, X, 0, S),
        "mul null out": lambda: L.csgn_mul_uniform(n, 1, 1, 1, X, X, 0, 0, S),
        "plan null": lambda: L.csgn_mul_ragged_plan(1, X, 0, X, C.byref(plan), S),
        "mul_ragged null offsets": lambda: L.csgn_mul_ragged(n, 1, X, 0, X, X, X, X, 1, 1, 1, S),
        "mul_ragged N=0": lambda: L.csgn_mul_ragged(0, 1, X, X, X, X, X, X, 1, 1, 1, S),
        "add null out": lambda: L.csgn_add_uniform(n, 1, 1, 1, X, X, 0, S),
        "add null left with terms": lambda: L.csgn_add_uniform(n, 1, 1, 1, 0, X, X, S),
        "add N=0": lambda: L.csgn_add_uniform(0, 1, 1, 1, X, X, X, S),
        "add_ragged null offsets": lambda: L.csgn_add_ragged(n, 1, X, 0, X, X, X, X, 2, S),
        "add_ragged null data": lambda: L.csgn_add_ragged(n, 1, 0, X, X, X, X, X, 2, S),
        "decrypt null mask": lambda: L.csgn_decrypt_uniform(n, 1, 1, X, 0, B, X, S),
        "decrypt null scratch": lambda: L.csgn_decrypt_uniform(n, 1, 1, X, X, B, 0, S),
        "decrypt N=0": lambda: L.csgn_decrypt_uniform(0, 1, 1, X, X, B, X, S),
        "decrypt_ragged null offsets": lambda: L.csgn_decrypt_ragged(n, 1, 1, X, 0, X, B, X, S),
        "decrypt_product null bits": lambda: L.csgn_decrypt_product_uniform(n, 1, 1, 1, X, X, X, 0, X, S),
        "compact null scratch": lambda: L.csgn_compact_ragged(n, 1, 1, 0, X, X, X, X, 0, S),
        "encrypt_explicit d=0": lambda: L.csgn_encrypt_explicit(n, 0, 1, B, X, X, X, X, X, S),
        "encrypt_explicit null": lambda: L.csgn_encrypt_explicit(n, 16, 1, B, 0, X, X, X, X, S),
        "encrypt_keyed null rng": lambda: L.csgn_encrypt_keyed(n, 16, 1, 0, B, X, X, 0, X, S),
        "encrypt_keyed bad rounds": lambda: L.csgn_encrypt_keyed(n, 16, 1, 0, B, X, X, C.byref(bad_rng), X, S),
        "encrypt_keyed d=0": lambda: L.csgn_encrypt_keyed(n, 0, 1, 0, B, X, X, C.byref(rng), X, S),
        "encrypt_keyed null key": lambda: L.csgn_encrypt_keyed(n, 16, 1, 0, B, 0, X, C.byref(rng), X, S),
        "encrypt_keyed position overflow": lambda: L.csgn_encrypt_keyed(n, 16, 2, (1 << 56) - 1, B, X, X, C.byref(rng), X, S),
        "encrypt_mul same generator": lambda: L.csgn_encrypt_mul_keyed(n, 16, 1, 0, B, B, X, X, C.byref(rng), C.byref(rng), X, 0, S),
        "encrypt_mul null plain": lambda: L.csgn_encrypt_mul_keyed(n, 16, 1, 0, B, 0, X, X, C.byref(rng), C.byref(bad_rng), X, 0, S),
        "permute null perm": lambda: L.csgn_permute_uniform(n, 1, 1, 0, X, 0, X, S),
        "permute null terms": lambda: L.csgn_permute_uniform(n, 1, 1, 0, 0, X, X, S),
        "synth N=0": lambda: L.csgn_synth_fill(1, 0, 0, 16, X, S),
        "synth null": lambda: L.csgn_synth_fill(1, n, 0, 16, 0, S),
        "digest null": lambda: L.csgn_digest(0, 16, 0, X, S),
        "key_mask index out of range": lambda: L.csgn_key_mask(n, (C.c_uint64 * 2)(5, n), 2, (C.c_uint64 * 20)()),
        "key_mask d=0": lambda: L.csgn_key_mask(n, (C.c_uint64 * 2)(5, 6), 0, (C.c_uint64 * 20)()),
        "rng bad rounds": lambda: L.csgn_rng_from_seed(C.byref(capi.CsgnRng()), 1, 9),
        "tuning unknown knob": lambda: L.csgn_set_tuning(b"no_such_knob", 1),
    }
    for name, call in cases.items():
        rc = call()
        assert rc != 0, name
        assert L.csgn_last_error(), name
    # circuits: ids that do not exist, building twice, running before building
    c = C.c_void_p()
    assert L.csgn_circuit_create(n, 0, C.byref(c)) != 0                     # batch 0
    capi.check(L.csgn_circuit_create(n, 4, C.byref(c)))
    try:
        v, w = C.c_uint32(), C.c_uint32()
        assert L.csgn_circuit_run(c, S) != 0                                # not built
        assert L.csgn_circuit_build(c) != 0                                 # no operations
        assert L.csgn_circuit_input(c, 0, C.byref(v)) != 0                  # zero terms
        capi.check(L.csgn_circuit_input(c, 1, C.byref(v)))
        assert L.csgn_circuit_mul(c, v.value, 99, C.byref(w)) != 0          # no such value
        assert L.csgn_circuit_decrypt(c, 99, X, C.byref(w)) != 0
        assert L.csgn_circuit_permute(c, v.value, 0, C.byref(w)) != 0       # null permutation
        capi.check(L.csgn_circuit_mul(c, v.value, v.value, C.byref(w)))
        capi.check(L.csgn_circuit_build(c))
        assert L.csgn_circuit_build(c) != 0                                 # already built
        assert L.csgn_circuit_input(c, 1, C.byref(v)) != 0                  # no inputs after build
    finally:
        L.csgn_circuit_destroy(c)
    torch.cuda.synchronize()                                                # and the device is still alive
    assert int(torch.arange(10, device=hip.device).sum().item()) == 45


# ---------------------------------------------------------------------------------- add

@pytest.mark.parametrize("n,d", CONTEXTS)
@pytest.mark.parametrize("t1,t2", [(1, 1), (1, 3), (4, 2), (17, 9), (0, 3), (5, 0), (300, 211)])
def test_add_uniform_matches_oracle(hip, oracle, n, d, t1, t2):
    dl = oracle.default_len(n)
    batch = 5
    L = oracle.synth(41, n, 0, max(batch * t1 * dl, 1))
    R = oracle.synth(42, n, 0, max(batch * t2 * dl, 1))
    out = hip.download(hip.add_uniform(n, batch, t1, t2, hip.upload(L), hip.upload(R)))
    per = (t1 + t2) * dl
    for b in range(batch):
        want, _ = oracle.add(L[b * t1 * dl:(b + 1) * t1 * dl], R[b * t2 * dl:(b + 1) * t2 * dl])
        assert np.array_equal(out[b * per:(b + 1) * per], want)


@pytest.mark.parametrize("n,d", [(1247, 16), (63, 4), (4096, 32)])
def test_add_ragged_matches_oracle(hip, oracle, n, d):
    dl = oracle.default_len(n)
    t1s = [1, 0, 3, 170, 1, 0]
    t2s = [1, 4, 0, 9, 333, 0]
    offL, offR = csr(t1s), csr(t2s)
    L = oracle.synth(51, n, 0, int(offL[-1]) * dl)
    R = oracle.synth(52, n, 0, int(offR[-1]) * dl)
    out, off_out = hip.add_ragged(n, hip.upload(L), hip.upload(offL), hip.upload(R), hip.upload(offR))
    out, off_out = hip.download(out), hip.download(off_out)
    assert np.array_equal(off_out, offL + offR)
    for b in range(len(t1s)):
        want, _ = oracle.add(L[int(offL[b]) * dl:int(offL[b + 1]) * dl],
                             R[int(offR[b]) * dl:int(offR[b + 1]) * dl])
        assert np.array_equal(out[int(off_out[b]) * dl:int(off_out[b + 1]) * dl], want)


# ------------------------------------------------------------------------------ decrypt

@pytest.mark.parametrize("n,d", CONTEXTS)
def test_decrypt_uniform_matches_oracle(hip, oracle, n, d):
    key = make_key(n, d, 3)
    mask = hip.key_mask(n, key)
    assert np.array_equal(mask, oracle.key_mask(n, key))
    dmask = hip.upload(mask)
    for terms in (1, 2, 5, 64, 255, 256, 257, 1000):
        batch = 7
        parts = [planted(oracle, n, key, terms, (b * 3) % (terms + 1), 100 + b) for b in range(batch)]
        flat = np.concatenate(parts)
        bits = hip.download(hip.decrypt_uniform(n, batch, terms, hip.upload(flat), dmask))
        for b in range(batch):
            want = oracle.decrypt(n, key, parts[b]) if terms <= 64 else oracle.decrypt_canonical(n, key, parts[b])
            assert want == ((b * 3) % (terms + 1)) % 2
            assert bits[b] == want, (n, terms, b)


@pytest.mark.parametrize("n,d", [(1247, 16), (4096, 32), (63, 4)])
def test_decrypt_ragged_matches_oracle(hip, oracle, n, d):
    key = make_key(n, d, 4)
    dmask = hip.upload(hip.key_mask(n, key))
    counts = [1, 0, 3, 300, 64, 0, 65, 1]
    parts = [planted(oracle, n, key, t, t // 2 + (t % 3 == 0), 200 + i) if t else np.zeros(0, np.uint64)
             for i, t in enumerate(counts)]
    flat = np.concatenate(parts)
    off = csr(counts)
    bits = hip.download(hip.decrypt_ragged(n, hip.upload(flat), hip.upload(off), dmask))
    for i, t in enumerate(counts):
        want = oracle.decrypt(n, key, parts[i]) if t else 0     # empty ciphertext -> 0
        assert bits[i] == want, i


def test_decrypt_one_million_terms(hip, oracle):
    """The stress shape of SURVEY 6 (1,048,576 terms): wave-per-ciphertext parity fold."""
    n, d, terms = 1247, 16, 1 << 20
    key = make_key(n, d, 5)
    dmask = hip.upload(hip.key_mask(n, key))
    for hits in (0, 1, 12345, 54321):
        flat = planted(oracle, n, key, terms, hits, 300 + hits)
        bits = hip.download(hip.decrypt_uniform(n, 1, terms, hip.upload(flat), dmask))
        assert bits[0] == hits % 2 == oracle.decrypt_canonical(n, key, flat)


# ------------------------------------------------------------------------------ encrypt

def test_encrypt_explicit_reproduces_reference_ciphertexts(hip, oracle, kat):
    """Golden fresh ciphertexts (from the genuine reference under srand(seed)) rebuilt on the GPU."""
    for case in kat["encrypt"]:
        n, d, seed, bits = case["n"], case["d"], case["seed"], case["bits"]
        key = np.array(case["key"], dtype=np.uint64)
        draws = glibc_draws(seed, (n + 2) * len(bits))
        dl = oracle.default_len(n)
        rnd = np.zeros(len(bits) * dl, dtype=np.uint64)
        chosen = np.zeros(len(bits), dtype=np.uint32)
        last = np.zeros(len(bits), dtype=np.uint8)
        pos = 0
        for i, b in enumerate(bits):
            r, c, l, used = explicit_randomness(n, key, b, draws[pos:])
            rnd[i * dl:(i + 1) * dl] = r
            chosen[i], last[i] = c, l
            pos += used
        out = hip.encrypt_explicit(n, d, hip.upload(np.array(bits, dtype=np.uint8)), hip.upload(rnd),
                                   hip.upload(chosen), hip.upload(last), hip.upload(hip.key_mask(n, key)))
        assert np.array_equal(hip.download(out), words(case["ct"])), (n, d, seed)


@pytest.mark.parametrize("n,d", [(1247, 16), (4096, 32), (65, 4), (63, 4), (100, 1), (128, 8)])
def test_encrypt_device_rng_properties(hip, oracle, n, d):
    key = make_key(n, d, 6)
    mask = hip.key_mask(n, key)
    rng = np.random.default_rng(7)
    batch = 4099
    plain = rng.integers(0, 2, size=batch).astype(np.uint8)
    dmask = hip.upload(mask)
    out = hip.encrypt_device_rng(n, d, hip.upload(plain), hip.upload(key), dmask, seed=99)
    dl = oracle.default_len(n)
    host = hip.download(out).reshape(batch, dl)
    rem = n % 64
    if rem:
        assert not np.any(host[:, -1] & np.uint64((1 << (64 - rem)) - 1))      # padding stays zero
    bits = hip.download(hip.decrypt_uniform(n, batch, 1, out, dmask))
    if d > 1:
        assert np.array_equal(bits, plain)
    for b in range(0, batch, 257):
        assert bits[b] == oracle.decrypt(n, key, host[b])
    # non-secret positions look random: overall density near 1/2
    dens = np.unpackbits(host.view(np.uint8)).mean() * (dl * 64) / n
    assert 0.45 < dens < 0.56
    # different seed -> different ciphertexts, same seed -> identical
    again = hip.download(hip.encrypt_device_rng(n, d, hip.upload(plain), hip.upload(key), dmask, seed=99))
    other = hip.download(hip.encrypt_device_rng(n, d, hip.upload(plain), hip.upload(key), dmask, seed=100))
    assert np.array_equal(again.reshape(batch, dl), host) and not np.array_equal(other.reshape(batch, dl), host)


KEYED_CONTEXTS = [(1247, 16), (4096, 32), (65, 4), (64, 4), (63, 4), (130, 5), (129, 3), (1247, 2), (4096, 3),
                  (300, 3), (1300, 4), (128, 1), (8192, 2), (2048, 5)]


@pytest.mark.parametrize("n,d", KEYED_CONTEXTS)
@pytest.mark.parametrize("wave", [1, 0, 2])
def test_encrypt_keyed_matches_the_restated_definition(hip, oracle, knobs, n, d, wave):
    """csgn_encrypt_keyed (ChaCha keystream, wave kernel and one-lane-per-ciphertext kernel) word for
    word against oracle.encrypt_keyed, on windows of the stream that start and end inside a group
    of ciphertexts.  Small D makes the all-secret-positions-came-out-1 clear frequent."""
    knobs.set("enc_wave", 1 if wave == 2 else wave)           # 0: one lane per ciphertext; 2: wave kernel with
    knobs.set("enc_compact", 0 if wave == 2 else 1)            # the full LDS tables, 1: with the compact ones
    key = make_key(n, d, 16)
    dmask, dkey = hip.upload(hip.key_mask(n, key)), hip.upload(key)
    units, passes, group = oracle.keyed_layout(n)
    rng = hip.rng_from_seed(77 + n, 8)
    rk, nonce = oracle.rng_from_seed(77 + n)
    assert list(rng.key) == [int(x) for x in rk] and rng.nonce == nonce
    dl = oracle.default_len(n)
    prng = np.random.default_rng(d)
    for first, batch in [(0, 3 * group + 5), (1, 1), (group - 1, 2), (5 * group + 7, 2 * group), (group, group),
                         (2**33 + 3, group + 9)]:
        plain = prng.integers(0, 2, batch).astype(np.uint8)
        got = hip.download(hip.encrypt_keyed(n, d, hip.upload(plain), dkey, dmask, rng, first_ciphertext=first))
        want = oracle.encrypt_keyed(n, key, plain, rk, nonce, 8, first_ciphertext=first)
        assert np.array_equal(got, want), (n, d, wave, first, batch)
        if d > 1:
            bits = hip.download(hip.decrypt_uniform(n, batch, 1, hip.upload(got), dmask))
            assert np.array_equal(bits, plain)


@pytest.mark.parametrize("rounds", [8, 12, 20])
def test_encrypt_keyed_rounds_and_a_million_ciphertexts(hip, oracle, rounds):
    """1 M fresh ciphertexts at N=1247 (BASELINE config 4's inputs): digest equal to the restated
    definition's, every ciphertext decrypts to its plaintext (a missed clear -- probability 2^-16 per
    plaintext-0 ciphertext, so about 8 in this batch -- would decrypt to 1)."""
    n, d, dl = 1247, 16, 20
    batch = (1 << 20) if rounds == 8 else (1 << 16)
    key = make_key(n, d, 3)
    dmask, dkey = hip.upload(hip.key_mask(n, key)), hip.upload(key)
    plain = np.random.default_rng(rounds).integers(0, 2, batch).astype(np.uint8)
    rng = hip.rng_from_seed(5, rounds)
    rk, nonce = oracle.rng_from_seed(5)
    out = hip.encrypt_keyed(n, d, hip.upload(plain), dkey, dmask, rng, first_ciphertext=12345)
    want = oracle.encrypt_keyed(n, key, plain, rk, nonce, rounds, first_ciphertext=12345)
    assert hip.digest(out) == oracle.digest(want)
    assert np.array_equal(hip.download(hip.decrypt_uniform(n, batch, 1, out, dmask)), plain)


def test_encrypt_keyed_fuzz(hip, oracle, knobs):
    """60 random (N, D, batch, first ciphertext, rounds) cases, keys with repeated indices among them:
    the wave kernel with compact and with full LDS tables and the one-lane-per-ciphertext kernel
    against the restated definition, word for word."""
    rng = np.random.default_rng(909 + FUZZ_SEED)
    for it in range(60):
        n = int(rng.choice([int(rng.integers(16, 4300)), 1247, 4096, 128, 640, 2560, 8192, 384]))
        d = int(rng.integers(1, min(n, 40) + 1))
        key = rng.permutation(n)[:d].astype(np.uint64)
        if it % 6 == 0 and d > 2:
            key[1] = key[0]                                   # setKey allows repeated indices
        if it % 11 == 0:
            key[:] = key[0]                                   # a single distinct position: never cleared
        batch = int(rng.choice([1, 2, 63, 64, 65, 127, 129, 500, 1500]))
        first = int(rng.choice([0, 1, int(rng.integers(0, 1 << 20)), int(rng.integers(0, 1 << 40))]))
        rounds = int(rng.choice([8, 8, 12, 20]))
        plain = rng.integers(0, 2, batch).astype(np.uint8)
        if d <= 3:
            plain[:] = 0                                      # make the clear frequent
        seed = int(rng.integers(0, 1 << 62))
        grng = hip.rng_from_seed(seed, rounds)
        rk, nonce = oracle.rng_from_seed(seed)
        want = oracle.encrypt_keyed(n, key, plain, rk, nonce, rounds, first_ciphertext=first)
        dmask, dkey, dplain = hip.upload(hip.key_mask(n, key)), hip.upload(key), hip.upload(plain)
        for wave, compact in ((1, 1), (1, 0), (0, -1)):
            knobs.set("enc_wave", wave)
            knobs.set("enc_compact", compact)
            got = hip.download(hip.encrypt_keyed(n, d, dplain, dkey, dmask, grng, first_ciphertext=first))
            assert np.array_equal(got, want), (it, n, d, batch, first, rounds, wave, compact)


@pytest.mark.parametrize("n,d", KEYED_CONTEXTS)
@pytest.mark.parametrize("wave", [1, 0])
def test_fused_fresh_chain_matches_encrypt_encrypt_multiply(hip, oracle, knobs, n, d, wave):
    """csgn_encrypt_mul_keyed (the reference's flow tests/basic_operations.cpp:26-40 as ONE
    kernel): the product words equal the restated definition's Enc_A & Enc_B (oracle.encrypt_keyed x2,
    src/Ciphertext.cpp:124-131), equal csgn_encrypt_keyed x2 + csgn_mul_uniform on the device, and the
    optional bits equal csgn_decrypt_uniform of the product and b1 & b0.  Windows of the stream that
    start and end inside a group; small D makes the clear-the-drawn-position rule frequent, in either
    factor and in both at once."""
    import torch
    knobs.set("enc_wave", wave)                              # 1: wave kernel, 0: one lane per pair
    key = make_key(n, d, 16)
    dmask, dkey = hip.upload(hip.key_mask(n, key)), hip.upload(key)
    units, passes, group = oracle.keyed_layout(n)
    ra, rb = hip.rng_from_seed(300 + n, 8), hip.rng_from_seed(301 + n, 8)
    (ka, na), (kb, nb) = oracle.rng_from_seed(300 + n), oracle.rng_from_seed(301 + n)
    prng = np.random.default_rng(d + 1)
    for first, batch in [(0, 3 * group + 5), (1, 1), (group - 1, 2), (5 * group + 7, 2 * group), (2**33 + 3, group + 9)]:
        pa = prng.integers(0, 2, batch).astype(np.uint8)
        pb = prng.integers(0, 2, batch).astype(np.uint8)
        if d <= 3:
            pa[: batch // 2] = 0                              # many plaintext-0 operands: the rule fires often
            pb[batch // 4:] = 0
        da, db = hip.upload(pa), hip.upload(pb)
        got, bits = hip.encrypt_mul_keyed(n, d, da, db, dkey, dmask, ra, rb, first_ciphertext=first)
        wa = oracle.encrypt_keyed(n, key, pa, ka, na, 8, first_ciphertext=first)
        wb = oracle.encrypt_keyed(n, key, pb, kb, nb, 8, first_ciphertext=first)
        assert np.array_equal(hip.download(got), wa & wb), (n, d, wave, first, batch)
        ea = hip.encrypt_keyed(n, d, da, dkey, dmask, ra, first_ciphertext=first)
        eb = hip.encrypt_keyed(n, d, db, dkey, dmask, rb, first_ciphertext=first)
        unfused = hip.mul_uniform(n, batch, 1, 1, ea, eb)
        assert torch.equal(got, unfused)
        want_bits = hip.download(hip.decrypt_uniform(n, batch, 1, unfused, dmask))
        assert np.array_equal(hip.download(bits), want_bits), (n, d, wave, first, batch)
        if len(set(int(k) for k in key)) > 1:
            assert np.array_equal(want_bits, pa & pb)
        # bits are optional
        got2, none = hip.encrypt_mul_keyed(n, d, da, db, dkey, dmask, ra, rb, first_ciphertext=first, with_bits=False)
        assert none is None and torch.equal(got2, got)


@pytest.mark.parametrize("rounds", [8, 20])
def test_fused_fresh_chain_a_million_pairs(hip, oracle, rounds):
    """BASELINE config 4's shape on one GPU: 1 M fresh pairs at N=1247 in one kernel; digest of the products
    equal to the restated definition's, bits equal b1 & b0 (about 16 of the 2 M operands hit the
    clear-the-drawn-position rule)."""
    n, d = 1247, 16
    batch = (1 << 20) if rounds == 8 else (1 << 16)
    key = make_key(n, d, 3)
    dmask, dkey = hip.upload(hip.key_mask(n, key)), hip.upload(key)
    prng = np.random.default_rng(rounds)
    pa, pb = prng.integers(0, 2, batch).astype(np.uint8), prng.integers(0, 2, batch).astype(np.uint8)
    ra, rb = hip.rng_from_seed(5, rounds), hip.rng_from_seed(6, rounds)
    (ka, na), (kb, nb) = oracle.rng_from_seed(5), oracle.rng_from_seed(6)
    got, bits = hip.encrypt_mul_keyed(n, d, hip.upload(pa), hip.upload(pb), dkey, dmask, ra, rb, first_ciphertext=999)
    wa = oracle.encrypt_keyed(n, key, pa, ka, na, rounds, first_ciphertext=999)
    wb = oracle.encrypt_keyed(n, key, pb, kb, nb, rounds, first_ciphertext=999)
    assert hip.digest(got) == oracle.digest(wa & wb)
    assert np.array_equal(hip.download(bits), pa & pb)


def test_fused_fresh_chain_argument_checks(hip):
    from csgn_amd import capi
    n, d = 1247, 16
    key = make_key(n, d, 1)
    dmask, dkey = hip.upload(hip.key_mask(n, key)), hip.upload(key)
    plain = hip.upload(np.ones(8, dtype=np.uint8))
    ra = hip.rng_from_seed(1, 8)
    with pytest.raises(capi.CsgnError, match="different streams"):
        hip.encrypt_mul_keyed(n, d, plain, plain, dkey, dmask, ra, ra)          # the same stream twice
    with pytest.raises(capi.CsgnError, match="same number of rounds"):
        hip.encrypt_mul_keyed(n, d, plain, plain, dkey, dmask, ra, hip.rng_from_seed(2, 12))
    out, bits = hip.encrypt_mul_keyed(n, d, plain[:0], plain[:0], dkey, dmask, ra, hip.rng_from_seed(2, 8))
    assert out.numel() == 0


def test_encrypt_keyed_os_entropy_and_argument_checks(hip, oracle):
    import ctypes as C
    from csgn_amd import capi
    a, b = hip.rng_from_os(), hip.rng_from_os(20)
    assert list(a.key) != list(b.key) and a.nonce != b.nonce and (a.rounds, b.rounds) == (8, 20)
    n, d = 1247, 16
    key = make_key(n, d, 1)
    dmask, dkey = hip.upload(hip.key_mask(n, key)), hip.upload(key)
    plain = hip.upload(np.array([1, 0, 1, 1, 0], dtype=np.uint8))
    out = hip.encrypt_keyed(n, d, plain, dkey, dmask, a)
    assert list(hip.download(hip.decrypt_uniform(n, 5, 1, out, dmask))) == [1, 0, 1, 1, 0]
    bad = capi.CsgnRng()
    bad.rounds = 7
    assert hip.lib.csgn_encrypt_keyed(n, d, 5, 0, plain.data_ptr(), dkey.data_ptr(), dmask.data_ptr(), C.byref(bad),
                                      out.data_ptr(), None) == -1
    assert hip.lib.csgn_rng_from_seed(C.byref(bad), 1, 9) == -1


# ------------------------------------- non-canonical bitlen: (v, bitlen) as a bit stream

def test_bitlen_stream_golden(hip, oracle):
    """csgn_decrypt_bitlen / csgn_permute_bitlen on the genuine reference's answers for ciphertexts
    whose Bitlen is not the canonical pattern (tests/golden/csgn_kat_bitlen.json)."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "csgn_kat_bitlen.json")) as f:
        cases = json.load(f)["bitlen_stream"]
    for c in cases:
        n = c["n"]
        key = np.array(c["key"], dtype=np.uint64)
        v, bl = words(c["v"]), np.array(c["bitlen"], dtype=np.uint64)
        dv, dbl = hip.upload(v), hip.upload(bl)
        assert hip.decrypt_bitlen(n, hip.upload(key), dv, dbl) == c["dec"], (n, c["pattern"])
        perm = hip.upload(np.array(c["perm"], dtype=np.uint32))
        assert np.array_equal(hip.download(hip.permute_bitlen(n, dv, dbl, perm)), words(c["permuted"]))


@pytest.mark.parametrize("n,d", [(1247, 16), (4096, 32), (65, 4), (64, 3), (63, 2), (130, 5), (2100, 7)])
def test_bitlen_stream_matches_oracle_on_arbitrary_patterns(hip, oracle, n, d):
    """Any bitlen the class API can be handed: zeros, short streams (positions past the end read 0,
    as the oracle defines the reference's out-of-bounds read), ragged lengths, long term lists; and
    the canonical pattern, where the stream calls must agree with the fast paths."""
    rng = np.random.default_rng(n + d)
    dl = oracle.default_len(n)
    for terms, kind in [(1, "canon"), (5, "canon"), (1, "rand"), (3, "rand"), (40, "rand"), (7, "zeros"), (9, "short"),
                        (2000, "near"), (1, "tiny")]:
        length = terms * dl + (3 if kind == "short" else 0)
        key = rng.permutation(n)[:d].astype(np.uint64)
        v = oracle.synth(int(rng.integers(1, 1 << 30)), n, 0, length)
        if kind == "canon":
            bl = canonical_bitlen(n, terms)
        elif kind == "rand":
            bl = rng.integers(0, 65, size=length).astype(np.uint64)
        elif kind == "zeros":
            bl = rng.choice([0, 0, 64, 17], size=length).astype(np.uint64)
        elif kind == "near":
            bl = (64 - rng.integers(0, 2, size=length)).astype(np.uint64)
        elif kind == "tiny":
            bl = np.ones(length, dtype=np.uint64)
        else:
            bl = rng.integers(50, 65, size=length).astype(np.uint64)
        # make the answer depend on the data: plant the key in every other term where the stream reaches
        pos = np.concatenate([[0], np.cumsum(bl)]).astype(np.int64)
        for k in range(0, terms, 2):
            for s_i in key:
                q = n * k + int(s_i)
                if q < pos[-1]:
                    w = int(np.searchsorted(pos, q, side="right") - 1)
                    v[w] |= np.uint64(1) << np.uint64(63 - (q - pos[w]))
        dv, dbl, dkey = hip.upload(v), hip.upload(bl), hip.upload(key)
        assert hip.decrypt_bitlen(n, dkey, dv, dbl) == oracle.decrypt(n, key, v, bl), (n, terms, kind)
        perm = rng.permutation(n).astype(np.uint64)
        got = hip.download(hip.permute_bitlen(n, dv, dbl, hip.upload(perm.astype(np.uint32))))
        assert np.array_equal(got, oracle.permute_ciphertext(n, perm, v, bl)), (n, terms, kind)
        if kind == "canon":
            dmask = hip.upload(hip.key_mask(n, key))
            assert hip.decrypt_bitlen(n, dkey, dv, dbl) == int(hip.download(hip.decrypt_uniform(n, 1, terms, dv, dmask))[0])
            assert np.array_equal(got, hip.download(hip.permute_uniform(n, 1, terms, dv, hip.upload(perm.astype(np.uint32)))))


# -------------------------------------------------------------------------- permutation

def test_permutation_golden(hip, oracle, kat):
    for case in kat["permutation"]:
        n, d = case["n"], case["d"]
        dl = oracle.default_len(n)
        perm = np.array(case["perm"], dtype=np.uint32)
        cts = words(case["ct"])
        dperm = hip.upload(perm)
        # three single-term ciphertexts as a batch
        out = hip.download(hip.permute_uniform(n, 3, 1, hip.upload(cts), dperm))
        for i in range(3):
            assert np.array_equal(out[i * dl:(i + 1) * dl],
                                  oracle.permute_ciphertext(n, perm.astype(np.uint64), cts[i * dl:(i + 1) * dl]))
        assert np.array_equal(out[:dl], words(case["permuted_first"]))
        # one 3-term ciphertext: the reference's truncation to the permuted first term
        multi = hip.download(hip.permute_uniform(n, 1, 3, hip.upload(cts), dperm))
        assert np.array_equal(multi, words(case["permuted_multi"]))
        # per-term extension permutes every term
        allp = hip.download(hip.permute_uniform(n, 1, 3, hip.upload(cts), dperm, per_term=True))
        assert np.array_equal(allp, out)
        # decrypt with the permuted key
        pkey = np.array(case["permuted_key"], dtype=np.uint64)
        bit = hip.download(hip.decrypt_uniform(n, 1, 1, hip.upload(multi), hip.upload(hip.key_mask(n, pkey))))
        assert bit[0] == case["dec_permuted"] == 1


# ------------------------------------------------------------------------ golden vectors

def test_golden_mul_add_decrypt(hip, oracle, kat):
    for case in kat["mul"]:
        n, t1, t2 = case["n"], case["t1"], case["t2"]
        out = hip.download(hip.mul_uniform(n, 1, t1, t2, hip.upload(words(case["a"])), hip.upload(words(case["b"]))))
        assert np.array_equal(out, words(case["out"])), (n, t1, t2)
    for case in kat["add"]:
        n, t1, t2 = case["n"], case["t1"], case["t2"]
        out = hip.download(hip.add_uniform(n, 1, t1, t2, hip.upload(words(case["a"])), hip.upload(words(case["b"]))))
        assert np.array_equal(out, words(case["out"]))
    for case in kat["decrypt"]:
        n, terms, hits = case["n"], case["terms"], case["hits"]
        key = np.array(case["key"], dtype=np.uint64)
        dl = oracle.default_len(n)
        v = oracle.synth(case["seed"], n, 0, terms * dl).reshape(terms, dl)
        v[:hits] |= oracle.key_mask(n, key)
        w, b = int(key[0]) // 64, 63 - int(key[0]) % 64
        v[hits:, w] &= ~np.uint64(1 << b)
        flat = np.ascontiguousarray(v.reshape(-1))
        dev = hip.upload(flat)
        assert "%016x" % hip.digest(dev) == case["digest"]
        bit = hip.download(hip.decrypt_uniform(n, 1, terms, dev, hip.upload(hip.key_mask(n, key))))
        assert bit[0] == case["bit"]


def test_golden_basic_operations(hip, oracle, kat):
    """tests/basic_operations.cpp on the GPU: Dec(Enc(1)+Enc(0)) = 1, Dec(Enc(1)*Enc(0)) = 0."""
    c = kat["basic_operations"]
    n = c["n"]
    key = np.array(c["key"], dtype=np.uint64)
    c1, c0 = hip.upload(words(c["c1"])), hip.upload(words(c["c0"]))
    added = hip.add_uniform(n, 1, 1, 1, c1, c0)
    mult = hip.mul_uniform(n, 1, 1, 1, c1, c0)
    assert np.array_equal(hip.download(added), words(c["added"]))
    assert np.array_equal(hip.download(mult), words(c["multiplied"]))
    dmask = hip.upload(hip.key_mask(n, key))
    assert hip.download(hip.decrypt_uniform(n, 1, 2, added, dmask))[0] == c["dec_added"] == 1
    assert hip.download(hip.decrypt_uniform(n, 1, 1, mult, dmask))[0] == c["dec_multiplied"] == 0


def test_golden_large_product_digests(hip, oracle, kat):
    """32x32, 256x256 and the 1024x1024 metric shape: digest of the GPU product equals the
    digest of the genuine reference's product (SURVEY 8c vi)."""
    for case in kat["digest"]:
        n, t1, t2 = case["n"], case["t1"], case["t2"]
        dl = oracle.default_len(n)
        a = hip.synth_fill(case["seed_a"], n, 0, t1 * dl)
        b = hip.synth_fill(case["seed_b"], n, 0, t2 * dl)
        out = hip.mul_uniform(n, 1, t1, t2, a, b)
        assert out.numel() == case["out_len"]
        assert "%016x" % hip.digest(out) == case["digest"], (t1, t2)
        host = hip.download(out[:4]), hip.download(out[-4:])
        assert np.array_equal(host[0], words(case["first_words"]))
        assert np.array_equal(host[1], words(case["last_words"]))


def test_timed_kernel_pair_at_the_timed_shape(hip, oracle, kat):
    """The kernels bench.py times (k_touch + k_mul_flat), at the timed shape (1024x1024 terms,
    N=1247), streamed through an arena smaller than the batch as bench.py does: 16 pairs (5.2 MB of
    operands, so the default dispatch IS the touch + flat pair), 6 slots, so the call is cut into
    launches of 6, 6 and 4 pairs and slots wrap.  EVERY surviving product is compared with the
    oracle's digest, and one of them is the golden 1024x1024 product of the genuine reference
    (tests/golden/csgn_kat.json digest[2]).  Reference: src/Ciphertext.cpp:146-163."""
    n, t, dl, B, slots = 1247, 1024, 20, 16, 6
    assert hip.lib.csgn_mul_uniform_kernel(n, B, t, t).decode() == "k_touch+k_mul_flat"
    case = [c for c in kat["digest"] if c["t1"] == 1024 and c["t2"] == 1024 and c["n"] == n][0]
    opw, per = t * dl, t * t * dl
    L = hip.synth_fill(31, n, 0, B * opw)
    R = hip.synth_fill(32, n, 0, B * opw)
    gq = 13                                                   # this pair is the golden one
    L[gq * opw:(gq + 1) * opw] = hip.synth_fill(case["seed_a"], n, 0, opw)
    R[gq * opw:(gq + 1) * opw] = hip.synth_fill(case["seed_b"], n, 0, opw)
    arena = hip.empty_words(slots * per)
    arena.fill_(-1)
    hip.mul_uniform(n, B, t, t, L, R, out=arena, out_slots=slots)
    hl, hr = hip.download(L), hip.download(R)
    # launches: pairs 0-5, 6-11, 12-15 -> slots 0..3 hold pairs 12..15, slots 4, 5 still hold 10, 11
    survivors = {0: 12, 1: 13, 2: 14, 3: 15, 4: 10, 5: 11}
    for slot, q in survivors.items():
        want, _ = oracle.mul(n, hl[q * opw:(q + 1) * opw], hr[q * opw:(q + 1) * opw])
        got = arena[slot * per:(slot + 1) * per]
        assert hip.digest(got) == oracle.digest(want), (slot, q)
        if q == gq:
            assert "%016x" % hip.digest(got) == case["digest"]
            assert np.array_equal(hip.download(got[:4]), words(case["first_words"]))
            assert np.array_equal(hip.download(got[-4:]), words(case["last_words"]))
    # and word for word for two of them (first and wrapped slot)
    for slot in (0, 5):
        q = survivors[slot]
        want, _ = oracle.mul(n, hl[q * opw:(q + 1) * opw], hr[q * opw:(q + 1) * opw])
        assert np.array_equal(hip.download(arena[slot * per:(slot + 1) * per]), want)


# ------------------------------------------------------- full-size, size-independent checks

def test_full_size_product_row_structure_and_decrypt_homomorphism(hip, oracle):
    """1024x1024 at N=1247: (i) every sampled output row i equals R masked by left term i;
    (ii) dec(a*b) = dec(a) & dec(b) with the 1M-term product decrypted on the GPU."""
    n, d, t, dl = 1247, 16, 1024, 20
    key = make_key(n, d, 8)
    mask = hip.key_mask(n, key)
    dmask = hip.upload(mask)
    for ha, hb in [(3, 5), (4, 7), (0, 9)]:
        A = planted(oracle, n, key, t, ha, 900 + ha)
        B = planted(oracle, n, key, t, hb, 950 + hb)
        dA, dB = hip.upload(A), hip.upload(B)
        prod = hip.mul_uniform(n, 1, t, t, dA, dB)
        P = hip.download(prod).reshape(t, t, dl)
        Ar, Br = A.reshape(t, dl), B.reshape(t, dl)
        for i in (0, 1, 63, 64, 511, 1023):
            assert np.array_equal(P[i], Br & Ar[i][None, :])
        bit = hip.download(hip.decrypt_uniform(n, 1, t * t, prod, dmask))[0]
        da = hip.download(hip.decrypt_uniform(n, 1, t, dA, dmask))[0]
        db = hip.download(hip.decrypt_uniform(n, 1, t, dB, dmask))[0]
        assert da == ha % 2 and db == hb % 2
        assert bit == (da & db) == (ha * hb) % 2


def test_circuit_config5_style(hip, oracle):
    """Context(4096,32): depth-8 mixed add/mul circuit on device-resident ciphertexts,
    permutation applied to the fresh inputs and to the key; plaintext tracked in the clear."""
    n, d = 4096, 32
    dl = 64
    key = make_key(n, d, 10)
    rng = np.random.default_rng(11)
    perm = rng.permutation(n).astype(np.uint64)
    pkey = oracle.permute_key(n, perm, key)
    dperm = hip.upload(perm.astype(np.uint32))
    dmask = hip.upload(hip.key_mask(n, key))
    dpmask = hip.upload(hip.key_mask(n, pkey))
    nb = 40
    plain = rng.integers(0, 2, size=nb).astype(np.uint8)
    fresh = hip.encrypt_device_rng(n, d, hip.upload(plain), hip.upload(key), dmask, seed=5)
    fresh = hip.permute_uniform(n, nb, 1, fresh, dperm)           # permuted fresh inputs
    assert np.array_equal(hip.download(hip.decrypt_uniform(n, nb, 1, fresh, dpmask)), plain)
    ct = lambda i: fresh[i * dl:(i + 1) * dl]
    x, xb, xt = ct(0), int(plain[0]), 1
    host_x = hip.download(x)
    k = 1
    for level in range(1, 9):
        if level % 2:
            x = hip.add_uniform(n, 1, xt, 1, x, ct(k)); xb ^= int(plain[k]); xt += 1
            host_x, _ = oracle.add(host_x, hip.download(ct(k)))
            k += 1
        else:
            rhs = hip.add_uniform(n, 1, 1, 1, ct(k), ct(k + 1)); rb = int(plain[k]) ^ int(plain[k + 1])
            host_rhs, _ = oracle.add(hip.download(ct(k)), hip.download(ct(k + 1)))
            x = hip.mul_uniform(n, 1, xt, 2, x, rhs); xb &= rb; xt *= 2
            host_x, _ = oracle.mul(n, host_x, host_rhs)
            k += 2
        assert np.array_equal(hip.download(x), host_x)
        assert hip.download(hip.decrypt_uniform(n, 1, xt, x, dpmask))[0] == xb == oracle.decrypt_canonical(n, pkey, host_x)


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 200, 1247, 2048, 2100, 4032, 4096, 8192, 10000])
def test_permute_all_word_counts(hip, oracle, n):
    """Small batches (9 terms: the ballot bit-gather, 4..64 words per pass, multi-pass above 64),
    first-term truncation and the per-term extension, for every word count."""
    dl = oracle.default_len(n)
    rng = np.random.default_rng(n)
    perm = rng.permutation(n).astype(np.uint64)
    nb = 9
    w = oracle.synth(5, n, 0, nb * dl)
    dperm = hip.upload(perm.astype(np.uint32))
    out = hip.download(hip.permute_uniform(n, nb, 1, hip.upload(w), dperm))
    for i in range(nb):
        assert np.array_equal(out[i * dl:(i + 1) * dl], oracle.permute_ciphertext(n, perm, w[i * dl:(i + 1) * dl])), (n, i)
    # 3-term inputs: first-term truncation vs per-term extension
    first = hip.download(hip.permute_uniform(n, 3, 3, hip.upload(w), dperm))
    for i in range(3):
        assert np.array_equal(first[i * dl:(i + 1) * dl], out[3 * i * dl:(3 * i + 1) * dl])
    assert np.array_equal(hip.download(hip.permute_uniform(n, 3, 3, hip.upload(w), dperm, per_term=True)), out)


@pytest.mark.parametrize("n", [1, 31, 63, 64, 65, 130, 1247, 1280, 1300, 4096, 4100, 8192, 10000, 16384])
@pytest.mark.parametrize("form", ["planes", "planes-narrow", "ballot", "planes-w1", "planes-w3", "planes-w16", "planes-p0"])
def test_permute_kernel_forms(hip, oracle, knobs, n, form):
    """Bit-plane form (64 terms per wave, 64x64 bit transposes; 16- and 8-byte staging) against
    the ballot form and the oracle, on batches that leave ragged last waves; strided first-term
    input and per-term mode."""
    knobs.set("CSGN_PERM_BALLOT", "1" if form == "ballot" else "0")
    knobs.set("CSGN_PERM_NARROW", "1" if form.endswith("narrow") else "0")
    if form.startswith("planes-w"):
        knobs.set("perm_waves", int(form[len("planes-w"):]))
    if form == "planes-p0":
        knobs.set("perm_persist", 0)                        # one 64-term group per workgroup
    dl = oracle.default_len(n)
    rng = np.random.default_rng(1000 + n)
    perm = rng.permutation(n).astype(np.uint64)
    dperm = hip.upload(perm.astype(np.uint32))
    for nb in (16, 64, 65, 200, 64 * 40 + 3):
        w = oracle.synth(nb, n, 0, nb * dl)
        dw = hip.upload(w)
        out = hip.download(hip.permute_uniform(n, nb, 1, dw, dperm))
        for i in range(nb):
            assert np.array_equal(out[i * dl:(i + 1) * dl],
                                  oracle.permute_ciphertext(n, perm, w[i * dl:(i + 1) * dl])), (n, nb, i)
        if nb % 4 == 0:
            first = hip.download(hip.permute_uniform(n, nb // 4, 4, dw, dperm))
            assert np.array_equal(first.reshape(-1, dl), out.reshape(-1, dl)[::4])
            assert np.array_equal(hip.download(hip.permute_uniform(n, nb // 4, 4, dw, dperm, per_term=True)), out)
    # inverse permutation restores the input
    inv = hip.upload(oracle.perm_inverse(perm).astype(np.uint32))
    w = oracle.synth(77, n, 0, 128 * dl)
    once = hip.permute_uniform(n, 128, 1, hip.upload(w), dperm)
    assert np.array_equal(hip.download(hip.permute_uniform(n, 128, 1, once, inv)), w)


def test_permute_forms_fuzz(hip, oracle, knobs):
    """120 random (N, batch, terms per input, per-term mode) cases, some with out-of-range
    permutation entries ("no source"): the bit-plane kernel with 16- and 8-byte staging and the
    ballot kernel must agree word for word; every tenth case is also checked against the oracle."""
    import torch
    rng = np.random.default_rng(2026 + FUZZ_SEED)
    for it in range(120):
        n = int(rng.integers(1, 4097))
        batch = int(rng.choice([16, 17, 63, 64, 65, 127, 128, 129, 1000, 4097, 20000]))
        dl = oracle.default_len(n)
        perm = rng.permutation(n).astype(np.uint32)
        if it % 5 == 0:
            perm[rng.integers(0, n, size=max(1, n // 7))] = n + int(rng.integers(0, 1000))
        dperm = hip.upload(perm)
        terms_in = int(rng.choice([1, 1, 3]))
        per_term = bool(rng.integers(0, 2)) if terms_in > 1 else False
        W = hip.synth_fill(it, n, 0, batch * terms_in * dl)
        outs = []
        for form in ("planes", "narrow", "ballot", "waves", "waves-narrow"):
            knobs.set("CSGN_PERM_BALLOT", "1" if form == "ballot" else "0")
            knobs.set("CSGN_PERM_NARROW", "1" if form.endswith("narrow") else "0")
            knobs.set("perm_waves", int(rng.integers(1, 17)) if form.startswith("waves") else 0)
            outs.append(hip.permute_uniform(n, batch, terms_in, W, dperm, per_term=per_term).clone())
        for o in outs[:2] + outs[3:]:
            assert torch.equal(o, outs[2]), (n, batch, terms_in, per_term)
        if it % 10 == 3:                              # a true permutation (it % 5 != 0): oracle too
            hw, ho = hip.download(W), hip.download(outs[0])
            stride = dl if per_term else terms_in * dl
            for b in (0, batch // 2, batch - 1):
                src = hw[b * stride:b * stride + dl]
                assert np.array_equal(ho[b * dl:(b + 1) * dl],
                                      oracle.permute_ciphertext(n, perm.astype(np.uint64), src)), (n, b)


@pytest.mark.parametrize("n,d", [(8320, 8), (8250, 5), (1247, 16), (193, 6), (704, 9), (1088, 7)])
@pytest.mark.parametrize("loop", [0, 1])
def test_decrypt_kernel_forms(hip, oracle, knobs, n, d, loop):
    """Both pass-1 forms (one-unit-per-lane workgroups of whole terms; looping 256-term
    workgroups for term sizes that do not pack into <=1024 lanes) on awkward term sizes."""
    knobs.set("CSGN_DEC_LOOP", str(loop))
    key = make_key(n, d, 13)
    dmask = hip.upload(hip.key_mask(n, key))
    for terms in (1, 7, 8, 9, 63, 64, 65, 300, 1031):
        batch = 3
        parts = [planted(oracle, n, key, terms, (5 * b + terms) % (terms + 1), 700 + b) for b in range(batch)]
        bits = hip.download(hip.decrypt_uniform(n, batch, terms, hip.upload(np.concatenate(parts)), dmask))
        for b in range(batch):
            assert bits[b] == oracle.decrypt_canonical(n, key, parts[b]) == ((5 * b + terms) % (terms + 1)) % 2


def test_config5_depth16_circuit_batched(hip, oracle):
    """BASELINE config 5 / SURVEY 8d: Context(4096,32), x0=Enc(b0); odd level: x += Enc(b);
    even level: x *= (Enc(b)+Enc(b')) -> 766 terms after 16 levels; a random Permutation is
    applied to every FRESH input and to the key first.  Run as a BATCH of independent circuits
    through the uniform batch calls; every circuit's ciphertext is compared with the oracle at
    the end and every level's decryption with the plaintext circuit evaluated in the clear."""
    n, d, dl, B = 4096, 32, 64, 24
    key = make_key(n, d, 21)
    rng = np.random.default_rng(22)
    perm = rng.permutation(n).astype(np.uint64)
    pkey = oracle.permute_key(n, perm, key)
    dmask = hip.upload(hip.key_mask(n, key))
    dpmask = hip.upload(hip.key_mask(n, pkey))
    per_circuit = 1 + 8 + 16                      # fresh inputs used by one circuit
    plain = rng.integers(0, 2, size=(per_circuit, B)).astype(np.uint8)   # input-major layout
    fresh = hip.encrypt_device_rng(n, d, hip.upload(plain.reshape(-1)), hip.upload(key), dmask, seed=77)
    fresh = hip.permute_uniform(n, per_circuit * B, 1, fresh, hip.upload(perm.astype(np.uint32)))
    inp = lambda i: fresh[i * B * dl:(i + 1) * B * dl]          # input i of every circuit: B ciphertexts
    x, xt = inp(0), 1
    xb = plain[0].copy()
    k = 1
    for level in range(1, 17):
        if level % 2:
            x = hip.add_uniform(n, B, xt, 1, x, inp(k)); xb ^= plain[k]; xt += 1; k += 1
        else:
            rhs = hip.add_uniform(n, B, 1, 1, inp(k), inp(k + 1))
            x = hip.mul_uniform(n, B, xt, 2, x, rhs); xb &= plain[k] ^ plain[k + 1]; xt *= 2; k += 2
        got = hip.download(hip.decrypt_uniform(n, B, xt, x, dpmask))
        assert np.array_equal(got, xb), level
    assert xt == 766 and k == per_circuit
    # full ciphertext parity for three of the circuits
    host_fresh = hip.download(fresh).reshape(per_circuit, B, dl)
    host_x = hip.download(x).reshape(B, xt * dl)
    for c in (0, 7, B - 1):
        hx, kk = host_fresh[0, c], 1
        for level in range(1, 17):
            if level % 2:
                hx, _ = oracle.add(hx, host_fresh[kk, c]); kk += 1
            else:
                r, _ = oracle.add(host_fresh[kk, c], host_fresh[kk + 1, c])
                hx, _ = oracle.mul(n, hx, r); kk += 2
        assert np.array_equal(host_x[c], hx)
        assert oracle.decrypt_canonical(n, pkey, hx) == xb[c]


def test_largest_supported_term_and_rejection(hip, oracle):
    """Terms of 16 KiB (N=131072) are the documented limit; one bit more is refused."""
    from csgn_amd.capi import CsgnError
    n = 131072
    dl = oracle.default_len(n)
    a = oracle.synth(1, n, 0, 3 * dl)
    b = oracle.synth(2, n, 0, 5 * dl)
    out = hip.download(hip.mul_uniform(n, 1, 3, 5, hip.upload(a), hip.upload(b)))
    want, _ = oracle.mul(n, a, b)
    assert np.array_equal(out, want)
    key = make_key(n, 8, 3)
    planted_ct = planted(oracle, n, key, 9, 4, 55)
    bit = hip.download(hip.decrypt_uniform(n, 1, 9, hip.upload(planted_ct), hip.upload(hip.key_mask(n, key))))
    assert bit[0] == 0 == oracle.decrypt_canonical(n, key, planted_ct)
    perm = np.random.default_rng(4).permutation(n).astype(np.uint64)
    got = hip.download(hip.permute_uniform(n, 1, 1, hip.upload(a[:dl]), hip.upload(perm.astype(np.uint32))))
    assert np.array_equal(got, oracle.permute_ciphertext(n, perm, a[:dl]))
    with pytest.raises(CsgnError):
        hip.mul_uniform(n + 1, 1, 1, 1, hip.upload(a), hip.upload(b))


@pytest.mark.parametrize("flat", ["-1", "1"])
def test_largest_single_product_index_edges(hip, knobs, flat):
    """One 16384 x 13107-term product at N=1247: 4 294 901 760 output words (34 GB), just under the
    documented 2^32-word limit and 2 147 450 880 sixteen-byte units, just under 2^31 -- the
    index arithmetic of both all-pairs kernels at its edge.  Sixty-odd whole rows (ends, rows at the
    2^32..2^35 byte marks, random ones) and 50 000 scattered terms are compared with torch's own
    bitwise_and (independent of the kernels); one more left term is refused."""
    import torch
    from csgn_amd.capi import CsgnError
    knobs.set("CSGN_MUL_FLAT", flat)
    n, dl, t1, t2 = 1247, 20, 16384, 13107
    assert t1 * t2 * dl < 2**32 <= (t1 + 1) * t2 * dl
    L = hip.synth_fill(31, n, 0, t1 * dl)
    R = hip.synth_fill(32, n, 0, t2 * dl)
    out = hip.mul_uniform(n, 1, t1, t2, L, R)
    Lw, Rw, Ow = (x.view(-1, dl) for x in (L, R, out[:t1 * t2 * dl]))
    g = torch.Generator(device="cpu").manual_seed(7)
    # whole rows: the ends, the rows around unit 2^31/... and byte 2^32/2^33/2^34/2^35, 48 random ones
    rows = {0, 1, t1 - 2, t1 - 1} | {(b // 160) // t2 + k for b in (2**32, 2**33, 2**34, 2**35) for k in (-1, 0, 1)}
    rows |= set(torch.randint(0, t1, (48,), generator=g).tolist())
    for i in sorted(r for r in rows if 0 <= r < t1):
        assert torch.equal(Ow[i * t2:(i + 1) * t2], torch.bitwise_and(Lw[i:i + 1], Rw)), i
    # scattered terms, 2000 at a time (one 200 000-index gather from the 34 GB tensor hung inside
    # torch on this image; the kernels under test are not involved in the gather)
    for _ in range(25):
        idx = torch.randint(0, t1 * t2, (2000,), generator=g, dtype=torch.int64).to(Ow.device)
        assert torch.equal(Ow[idx], torch.bitwise_and(Lw[idx // t2], Rw[idx % t2]))
    del out, Ow
    torch.cuda.empty_cache()
    from csgn_amd.capi import check
    big = hip.synth_fill(33, n, 0, (t1 + 1) * dl)
    with pytest.raises(CsgnError):                              # refused before any launch
        check(hip.lib.csgn_mul_uniform(n, 1, t1 + 1, t2, big.data_ptr(), R.data_ptr(), L.data_ptr(), 0,
                                       hip.stream))


@pytest.mark.parametrize("n,d", [(1247, 16), (4096, 32), (63, 4)])
def test_fused_product_and_sum_decrypt(hip, oracle, n, d):
    """Dec(L*R) and Dec(L+R) computed without materialising the result equal the decryption of
    the materialised result (GPU) and of the oracle's result."""
    key = make_key(n, d, 31)
    dmask = hip.upload(hip.key_mask(n, key))
    dl = oracle.default_len(n)
    for (t1, t2) in [(1, 1), (3, 5), (64, 33), (300, 7)]:
        batch = 12
        Ls = [planted(oracle, n, key, t1, (b * 7 + 1) % (t1 + 1), 800 + b) for b in range(batch)]
        Rs = [planted(oracle, n, key, t2, (b * 5 + 2) % (t2 + 1), 900 + b) for b in range(batch)]
        dL_, dR_ = hip.upload(np.concatenate(Ls)), hip.upload(np.concatenate(Rs))
        fused_mul = hip.download(hip.decrypt_combined_uniform(n, batch, t1, t2, dL_, dR_, dmask, True))
        fused_add = hip.download(hip.decrypt_combined_uniform(n, batch, t1, t2, dL_, dR_, dmask, False))
        prod = hip.mul_uniform(n, batch, t1, t2, dL_, dR_)
        summ = hip.add_uniform(n, batch, t1, t2, dL_, dR_)
        assert np.array_equal(fused_mul, hip.download(hip.decrypt_uniform(n, batch, t1 * t2, prod, dmask)))
        assert np.array_equal(fused_add, hip.download(hip.decrypt_uniform(n, batch, t1 + t2, summ, dmask)))
        for b in (0, 5, batch - 1):
            pm, _ = oracle.mul(n, Ls[b], Rs[b])
            pa, _ = oracle.add(Ls[b], Rs[b])
            assert fused_mul[b] == oracle.decrypt_canonical(n, key, pm)
            assert fused_add[b] == oracle.decrypt_canonical(n, key, pa)


def test_fused_product_decrypt_full_size(hip, oracle):
    """1024x1024 at N=1247: the fused form answers from 2x160 KB what the materialised
    168 MB product decrypts to."""
    n, d, t = 1247, 16, 1024
    key = make_key(n, d, 33)
    dmask = hip.upload(hip.key_mask(n, key))
    batch = 6
    Ls = [planted(oracle, n, key, t, 3 + b, 1000 + b) for b in range(batch)]
    Rs = [planted(oracle, n, key, t, 5 + 2 * b + (b % 2), 1100 + b) for b in range(batch)]
    dL_, dR_ = hip.upload(np.concatenate(Ls)), hip.upload(np.concatenate(Rs))
    fused = hip.download(hip.decrypt_combined_uniform(n, batch, t, t, dL_, dR_, dmask, True))
    prod = hip.mul_uniform(n, batch, t, t, dL_, dR_)
    mat = hip.download(hip.decrypt_uniform(n, batch, t * t, prod, dmask))
    assert np.array_equal(fused, mat)
    assert list(fused) == [((3 + b) * (5 + 2 * b + (b % 2))) % 2 for b in range(batch)]


def test_concurrent_host_threads_on_separate_streams(hip, oracle):
    """SURVEY 8b threading row: the shim is callable from several host threads at once, each on
    its own stream (ctypes drops the GIL during the calls); results stay bit-exact."""
    import threading
    import torch
    n, dl = 1247, 20
    key = make_key(n, 16, 41)
    dmask = hip.upload(hip.key_mask(n, key))
    errors = []

    def worker(idx):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for it in range(25):
                    t1, t2 = 3 + (it + idx) % 5, 2 + (it * 7 + idx) % 9
                    a = oracle.synth(1000 * idx + it, n, 0, t1 * dl)
                    b = oracle.synth(2000 * idx + it, n, 0, t2 * dl)
                    da, db = hip.upload(a), hip.upload(b)
                    prod = hip.mul_uniform(n, 1, t1, t2, da, db)
                    summ = hip.add_uniform(n, 1, t1, t2, da, db)
                    bit = hip.decrypt_uniform(n, 1, t1 * t2, prod, dmask)
                    want_p, _ = oracle.mul(n, a, b)
                    want_s, _ = oracle.add(a, b)
                    stream.synchronize()
                    assert np.array_equal(hip.download(prod), want_p)
                    assert np.array_equal(hip.download(summ), want_s)
                    assert hip.download(bit)[0] == oracle.decrypt_canonical(n, key, want_p)
        except Exception as e:          # noqa: BLE001
            errors.append((idx, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_concurrent_host_threads_ragged_plans_encrypt_and_permute(hip, oracle):
    """Per-host-thread state of the library under concurrency: every thread plans its OWN skewed CSR batch (one
    pair of >= 24 MB of output, multiplied by the thread's own csgn_mul_plan object), draws keyed
    ciphertexts and permutes them, each on its own stream, four threads at once.  A plan remembered by one
    thread must never steer another thread's multiply; all results equal the oracle's."""
    import threading
    import torch
    n, d, dl = 1247, 16, 20
    key = make_key(n, d, 43)
    dmask_host = hip.key_mask(n, key)
    errors = []

    def worker(idx):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                dmask, dkey = hip.upload(dmask_host), hip.upload(key)
                rng_np = np.random.default_rng(900 + idx)
                for it in range(3):
                    batch = 40 + 7 * idx + it
                    t1s, t2s = rng_np.integers(0, 5, size=batch), rng_np.integers(0, 5, size=batch)
                    big = int(rng_np.integers(0, batch))
                    t1s[big], t2s[big] = 400 + idx, 400 + 3 * it          # >= 160 000 product terms: 25.6 MB
                    offL, offR = csr(t1s.tolist()), csr(t2s.tolist())
                    hl = oracle.synth(3000 + 10 * idx + it, n, 0, int(offL[-1]) * dl)
                    hr = oracle.synth(4000 + 10 * idx + it, n, 0, int(offR[-1]) * dl)
                    out, off = hip.mul_ragged(n, hip.upload(hl), hip.upload(offL), hip.upload(hr), hip.upload(offR))
                    mo = hip.download(off)
                    assert np.array_equal(mo, csr((t1s * t2s).tolist()))
                    for b in {big, 0, batch - 1, max(0, big - 1), min(batch - 1, big + 1)}:
                        if t1s[b] and t2s[b]:
                            want, _ = oracle.mul(n, hl[int(offL[b]) * dl:int(offL[b + 1]) * dl],
                                                 hr[int(offR[b]) * dl:int(offR[b + 1]) * dl])
                            assert np.array_equal(hip.download(out[int(mo[b]) * dl:int(mo[b + 1]) * dl]), want), (idx, it, b)
                    # keyed encrypt at a thread-specific stream position, then a permutation of the fresh batch
                    rng = hip.rng_from_seed(500 + idx, 8)
                    rk, nonce = oracle.rng_from_seed(500 + idx)
                    plain = rng_np.integers(0, 2, 300 + idx).astype(np.uint8)
                    first = 1000 * idx + 17 * it
                    ct = hip.encrypt_keyed(n, d, hip.upload(plain), dkey, dmask, rng, first_ciphertext=first)
                    got = hip.download(ct)
                    assert np.array_equal(got, oracle.encrypt_keyed(n, key, plain, rk, nonce, 8, first_ciphertext=first))
                    perm = np.random.default_rng(idx * 31 + it).permutation(n).astype(np.uint32)
                    pc = hip.download(hip.permute_uniform(n, plain.size, 1, ct, hip.upload(perm)))
                    for c in (0, plain.size - 1):
                        assert np.array_equal(pc[c * dl:(c + 1) * dl], oracle.permute_ciphertext(n, perm, got[c * dl:(c + 1) * dl]))
                stream.synchronize()
        except Exception as e:          # noqa: BLE001
            import traceback
            errors.append((idx, repr(e), traceback.format_exc()[-600:]))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_mul_fresh_batch_one_million(hip, oracle):
    """BASELINE config 4 per-GPU shape and beyond: 1,048,576 independent 1x1 products."""
    n, batch, dl = 1247, 1 << 20, 20
    L = hip.synth_fill(71, n, 0, batch * dl)
    R = hip.synth_fill(72, n, 0, batch * dl)
    out = hip.mul_uniform(n, batch, 1, 1, L, R)
    hl, hr = oracle.synth(71, n, 0, batch * dl), oracle.synth(72, n, 0, batch * dl)
    assert hip.digest(out) == oracle.digest(hl & hr)
    got = hip.download(out[-20:])
    want, _ = oracle.mul(n, hl[-20:], hr[-20:])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n,d", [(1247, 16), (4096, 32), (63, 4)])
def test_compaction_extension(hip, oracle, n, d):
    """EXTENSION, not reference behaviour: mod-2 compaction.  Checked against the
    extension's own CPU checker (exact term list) and, more importantly, for the property that
    makes it legal: Dec is unchanged under ANY key."""
    dl = oracle.default_len(n)
    rng = np.random.default_rng(n)
    # ragged batch with planted duplicates: pools of distinct terms drawn with repetition
    cts = []
    for b, (pool, draws) in enumerate([(1, 2), (1, 3), (5, 40), (300, 1000), (0, 0), (64, 64), (7, 1)]):
        if draws == 0:
            cts.append(np.zeros(0, dtype=np.uint64))
            continue
        base = oracle.synth(500 + b, n, 0, pool * dl).reshape(pool, dl)
        idx = rng.integers(0, pool, size=draws)
        cts.append(np.ascontiguousarray(base[idx].reshape(-1)))
    off = csr([c.size // dl for c in cts])
    flat = np.concatenate(cts)
    out, off_out = hip.compact_ragged(n, hip.upload(flat), hip.upload(off))
    out, off_out = hip.download(out), hip.download(off_out)
    keys = [make_key(n, d, 90 + i) for i in range(3)]
    for b, ct in enumerate(cts):
        got = out[int(off_out[b]) * dl:int(off_out[b + 1]) * dl]
        want = oracle.compact(n, ct)
        assert np.array_equal(got, want), b
        rows = got.reshape(-1, dl)
        assert len({r.tobytes() for r in rows}) == rows.shape[0]          # all distinct
        for key in keys:
            assert oracle.decrypt_canonical(n, key, got) == oracle.decrypt_canonical(n, key, ct)
    assert int(off_out[1]) - int(off_out[0]) == 0      # x + x cancels completely
    assert int(off_out[2]) - int(off_out[1]) == 1      # x + x + x leaves x


def test_compaction_of_squared_sum(hip, oracle):
    """(a+b)*(a+b) = a*a + a*b + b*a + b*b: the two cross terms are bit-identical (AND commutes)
    and cancel; the GPU decryption of the compacted ciphertext still equals Dec(a+b)."""
    n, d, dl = 1247, 16, 20
    key = make_key(n, d, 7)
    dmask = hip.upload(hip.key_mask(n, key))
    plain = np.array([1, 0], dtype=np.uint8)
    fresh = hip.encrypt_device_rng(n, d, hip.upload(plain), hip.upload(key), dmask, seed=3)
    s = hip.add_uniform(n, 1, 1, 1, fresh[:dl], fresh[dl:])
    sq = hip.mul_uniform(n, 1, 2, 2, s, s)
    out, off_out = hip.compact_ragged(n, sq, hip.upload(csr([4])))
    assert hip.download(off_out).tolist() == [0, 2]
    bit = hip.download(hip.decrypt_uniform(n, 1, 2, out, dmask))[0]
    assert bit == hip.download(hip.decrypt_uniform(n, 1, 4, sq, dmask))[0] == 1


def _dup_ciphertext(oracle, rng, n, seed, pool, draws):
    """`draws` terms drawn with repetition from `pool` distinct synthetic terms (pool 0 = no terms)."""
    dl = oracle.default_len(n)
    if draws == 0:
        return np.zeros(0, dtype=np.uint64)
    base = oracle.synth(seed, n, 0, pool * dl).reshape(pool, dl)
    return np.ascontiguousarray(base[rng.integers(0, pool, size=draws)].reshape(-1))


def _check_compaction(hip, oracle, n, cts, max_terms=0, expect_compacted=True):
    dl = oracle.default_len(n)
    off = csr([c.size // dl for c in cts])
    flat = np.concatenate(cts) if off[-1] else np.zeros(0, dtype=np.uint64)
    out, off_out = hip.compact_ragged(n, hip.upload(flat) if flat.size else hip.empty_words(1), hip.upload(off),
                                      total_terms=int(off[-1]), max_terms=max_terms)
    out, off_out = hip.download(out), hip.download(off_out)
    assert off_out[0] == 0 and np.all(np.diff(off_out.astype(np.int64)) >= 0)
    for b, ct in enumerate(cts):
        got = out[int(off_out[b]) * dl:int(off_out[b + 1]) * dl]
        want = oracle.compact(n, ct) if expect_compacted else ct
        assert np.array_equal(got, want), (n, b, ct.size // dl, got.size // dl, want.size // dl)
    assert out.size == int(off_out[-1]) * dl
    return off_out


@pytest.mark.parametrize("n", [1247, 4096, 130, 129, 63])
def test_compaction_many_groups_and_sizes(hip, oracle, n):
    """Several hundred ciphertexts of every size class in one call: runs of small ones that share a
    workgroup, ciphertexts that fill one alone, empty ones in every position, and (at the wider contexts)
    ciphertexts beyond a workgroup's group that are deduplicated by hash partitions -- all behind one look-back
    chain of output offsets.  Term lists identical to the checker's."""
    rng = np.random.default_rng(n + 11)
    cts = []
    for b in range(260):
        kind = rng.integers(0, 10)
        if kind == 0:
            draws = 0
        elif kind < 6:
            draws = int(rng.integers(1, 40))
        elif kind < 9:
            draws = int(rng.integers(40, 700))
        else:
            draws = int(rng.integers(700, 1400))
        pool = max(1, int(draws * rng.choice([0.05, 0.5, 1.0, 3.0])))
        cts.append(_dup_ciphertext(oracle, rng, n, 3000 + b, pool, draws))
    cts[0] = np.zeros(0, dtype=np.uint64)                      # leading, trailing and adjacent empties
    cts[-1] = np.zeros(0, dtype=np.uint64)
    cts[100] = cts[101] = cts[102] = np.zeros(0, dtype=np.uint64)
    _check_compaction(hip, oracle, n, cts)


def test_compaction_large_ciphertexts(hip, oracle):
    """Ciphertexts of many workgroup groups (3 000 to 40 000 terms at N=1247: the hash-partition path), between
    small ones, with 0 %, 50 % and 97 % duplicates."""
    n = 1247
    rng = np.random.default_rng(5)
    cts = [_dup_ciphertext(oracle, rng, n, 1, 5, 9),
           _dup_ciphertext(oracle, rng, n, 2, 40000, 3000),
           _dup_ciphertext(oracle, rng, n, 3, 20000, 40000),
           np.zeros(0, dtype=np.uint64),
           _dup_ciphertext(oracle, rng, n, 4, 300, 10000),
           _dup_ciphertext(oracle, rng, n, 5, 100, 1024),
           _dup_ciphertext(oracle, rng, n, 6, 2000, 1025),
           _dup_ciphertext(oracle, rng, n, 7, 3, 2)]
    off_out = _check_compaction(hip, oracle, n, cts)
    assert int(off_out[6]) - int(off_out[5]) <= 100


@pytest.mark.parametrize("n", [1247, 4096, 129, 64, 16500])
def test_compaction_large_ciphertexts_partition_overflow_and_shapes(hip, oracle, n):
    """The partitions of a large ciphertext (pairs dealt by the top bits of the term hash, 2048 to a partition at
    most): one term repeated thousands of times overflows its partition and the call takes the exact path; sizes
    on both sides of every partition count (one, two, many partitions); several large ciphertexts in one batch
    with small ones between them; N = 16 500 has terms of 129 sixteen-byte units -- more than a wave's lanes, which then
    loop over a term's units.  Term lists identical to the checker's."""
    rng = np.random.default_rng(n)
    dl = oracle.default_len(n)
    heavy = _dup_ciphertext(oracle, rng, n, 60, 3000, 9000).reshape(-1, dl)
    heavy[rng.permutation(9000)[:5001]] = heavy[0]                # one term 5001 times: its partition overflows
    cts = [_dup_ciphertext(oracle, rng, n, 61, 4, 6), np.ascontiguousarray(heavy.reshape(-1)),
           _dup_ciphertext(oracle, rng, n, 62, 5000, 5000)]
    _check_compaction(hip, oracle, n, cts)
    sizes = [1025, 2048, 2049, 4097, 0, 7, 12289, 1500]
    cts = [_dup_ciphertext(oracle, rng, n, 63 + i, max(1, int(t * f)), t) for i, (t, f) in
           enumerate(zip(sizes, [1.0, 0.5, 4.0, 0.25, 1.0, 1.0, 0.6, 0.01]))]
    _check_compaction(hip, oracle, n, cts)


def test_compaction_of_a_ciphertext_of_more_than_two_million_terms(hip):
    """One ciphertext of 2^21 + 5000 terms (4096 hash partitions: beyond what a stripe sorts in LDS, so every term takes
    its partition's cursor itself) between two small ones: 1500 planted pairs of equal terms cancel, everything else
    stays in order.  Checked on the device against the construction (the oracle would need minutes)."""
    import torch
    n, dl = 1247, 20
    T = (1 << 21) + 5000
    counts = [3, T, 2]
    total = sum(counts)
    w = hip.synth_fill(97, n, 0, total * dl).view(total, dl)
    g = torch.Generator(device="cpu")
    g.manual_seed(5)
    picks = (torch.randperm(T, generator=g)[:3000] + 3).to(hip.device)      # 1500 disjoint pairs inside the long ciphertext
    a, b = picks[:1500], picks[1500:]
    w[b] = w[a]
    keep = torch.ones(total, dtype=torch.bool, device=hip.device)
    keep[a] = False
    keep[b] = False
    out, off_out = hip.compact_ragged(n, w.reshape(-1), hip.upload(csr(counts)), total_terms=total)
    off_out = hip.download(off_out)
    assert list(np.diff(off_out.astype(np.int64))) == [3, T - 3000, 2]
    assert torch.equal(out.view(-1, dl), w[keep])


@pytest.mark.parametrize("batch", [50_000, 300_000])
def test_compaction_small_bound_fills_the_groups_and_survives_being_broken(hip, oracle, batch):
    """With a small bound on a ciphertext's terms the runs of tiny ciphertexts are cut into FULL groups (window = group
    size - bound) instead of half-full ones.  A caller who breaks such a bound everywhere (ciphertexts of up to 6 terms
    promised to have at most 2) would make every ciphertext a group of its own and overrun the group arrays of a scratch
    block sized without the bound: the plan notices and the whole call takes the unbounded geometry.  Both the honest
    and the broken promise give the checker's term lists (300 000 ciphertexts: the plan's scan kernel)."""
    n, dl = 1247, 20
    rng = np.random.default_rng(batch)
    for top, bound in ((3, 3), (6, 2), (3, 40)):
        counts = rng.integers(0, top + 1, size=batch)
        total = int(counts.sum())
        words_ = oracle.synth(91, n, 0, total * dl).reshape(total, dl)
        off = csr(counts)
        starts = off[:-1].astype(np.int64)
        twin = np.nonzero(counts >= 2)[0][::3]                        # every third such ciphertext: its second term = its first
        words_[starts[twin] + 1] = words_[starts[twin]]
        out, off_out = hip.compact_ragged(n, hip.upload(words_.reshape(-1)), hip.upload(off), total_terms=total, max_terms=bound)
        out, off_out = hip.download(out).reshape(-1, dl), hip.download(off_out)
        want_counts = counts.copy()
        want_counts[twin] -= 2
        assert np.array_equal(np.diff(off_out.astype(np.int64)), want_counts), (top, bound)
        keep = np.ones(total, dtype=bool)
        keep[starts[twin]] = keep[starts[twin] + 1] = False
        assert np.array_equal(out, words_[keep]), (top, bound)


@pytest.mark.parametrize("n,sizes", [(1247, [1100, 1792, 3, 1500, 0, 1025, 700]), (4096, [766, 321, 768, 5, 500])])
def test_compaction_wide_groups(hip, oracle, n, sizes):
    """Ciphertexts between one workgroup's usual group (1024 terms at N=1247, 320 at N=4096) and the wide build's
    (1792 / 768 -- BASELINE config 5 ends at 766 terms): with the caller's bound they are read once by the
    48-units-per-lane build of the main kernel; without it they take the hash-partition path.  Same term lists as the
    checker's either way, 0 % to 97 % duplicates."""
    rng = np.random.default_rng(n + 3)
    cts = [_dup_ciphertext(oracle, rng, n, 40 + i, max(1, int(t * f)), t) for i, (t, f) in
           enumerate(zip(sizes, [1.5, 0.5, 1.0, 0.03, 1.0, 2.0, 0.3]))]
    _check_compaction(hip, oracle, n, cts, max_terms=max(sizes))
    _check_compaction(hip, oracle, n, cts)


def test_compaction_one_million_single_terms_and_empties(hip, oracle):
    """A batch of 2^20 ciphertexts of 0, 1 or 2 terms: groups are runs of hundreds of ciphertexts whose
    offsets the workgroup stages in LDS; x + x vanishes."""
    n, dl = 1247, 20
    rng = np.random.default_rng(9)
    counts = rng.integers(0, 3, size=1 << 20)
    same = rng.integers(0, 2, size=counts.size).astype(bool)          # a 2-term ciphertext of two equal terms
    total = int(counts.sum())
    words_ = oracle.synth(77, n, 0, total * dl).reshape(total, dl)
    off = csr(counts)
    starts = off[:-1].astype(np.int64)
    twin = np.nonzero((counts == 2) & same)[0]
    words_[starts[twin] + 1] = words_[starts[twin]]
    out, off_out = hip.compact_ragged(n, hip.upload(words_.reshape(-1)), hip.upload(off), total_terms=total,
                                      max_terms=2)
    out, off_out = hip.download(out).reshape(-1, dl), hip.download(off_out)
    want_counts = counts.copy()
    want_counts[twin] = 0
    assert np.array_equal(np.diff(off_out.astype(np.int64)), want_counts)
    keep = np.ones(total, dtype=bool)
    keep[starts[twin]] = keep[starts[twin] + 1] = False
    assert np.array_equal(out, words_[keep])


@pytest.mark.parametrize("bits", [1, 3])
def test_compaction_survives_tag_collisions(hip, oracle, knobs, bits):
    """With the hash tags narrowed to a few bits, unequal terms collide all the time: the verify pass
    catches it and the group (or, for large ciphertexts, the call: the exact open-addressing table in HBM) is redone with full compares -- the words stay exact."""
    knobs.set("compact_tag_bits", bits)
    rng = np.random.default_rng(bits)
    for n in (1247, 129):
        cts = [_dup_ciphertext(oracle, rng, n, 10, 50, 200),
               _dup_ciphertext(oracle, rng, n, 11, 1000, 1000),
               _dup_ciphertext(oracle, rng, n, 12, 700, 2500),
               _dup_ciphertext(oracle, rng, n, 13, 2, 7),
               np.zeros(0, dtype=np.uint64),
               _dup_ciphertext(oracle, rng, n, 14, 30, 31)]
        _check_compaction(hip, oracle, n, cts)


def test_compaction_sparse_terms(hip, oracle):
    """Deep products are sparse (a bit survives ten ANDs with probability 2^-10): terms with one or two set
    bits, many of them equal or all zero, must hash apart and merge exactly."""
    n, dl = 1247, 20
    rng = np.random.default_rng(3)
    cts = []
    for t in (1000, 64, 1024, 2000):
        rows = np.zeros((t, dl), dtype=np.uint64)
        for r in range(t):
            for _ in range(int(rng.integers(0, 3))):
                bit = int(rng.integers(0, 200))                # few positions: plenty of equal terms
                rows[r, bit // 64] |= np.uint64(1) << np.uint64(63 - bit % 64)
        cts.append(rows.reshape(-1))
    _check_compaction(hip, oracle, n, cts)


def test_compaction_bound_that_is_exceeded_copies_the_ciphertext(hip, oracle):
    """max_terms is a launch hint: a ciphertext larger than one group that breaks a promised bound is
    copied through as it is (legal: Dec unchanged), everything else is compacted."""
    n = 1247
    rng = np.random.default_rng(8)
    big = _dup_ciphertext(oracle, rng, n, 21, 10, 3000)
    small = _dup_ciphertext(oracle, rng, n, 22, 10, 300)
    dl = oracle.default_len(n)
    off = csr([small.size // dl, big.size // dl, small.size // dl])
    out, off_out = hip.compact_ragged(n, hip.upload(np.concatenate([small, big, small])), hip.upload(off),
                                      max_terms=512)
    out, off_out = hip.download(out), hip.download(off_out)
    want_small = oracle.compact(n, small)
    k = want_small.size // dl
    assert off_out.tolist() == [0, k, k + 3000, 2 * k + 3000]
    assert np.array_equal(out[:k * dl], want_small)
    assert np.array_equal(out[k * dl:(k + 3000) * dl], big)
    assert np.array_equal(out[(k + 3000) * dl:], want_small)


ENC_FORMS = {"seg": {}, "lds": {"CSGN_ENC_LDS": "1"}}


@pytest.mark.parametrize("form", sorted(ENC_FORMS))
def test_encrypt_kernel_forms_reproduce_reference(hip, oracle, kat, knobs, form):
    """Both encrypt kernels (register/ballot segments; LDS-staged general form) against the genuine
    reference's fresh ciphertexts, plus agreement of their device-RNG streams on several contexts
    (even and odd dL, term sizes that do and do not pack into segments)."""
    def use(f):
        knobs.unset("CSGN_ENC_LDS")
        for k, v in ENC_FORMS[f].items():
            knobs.set(k, v)
    use(form)
    test_encrypt_explicit_reproduces_reference_ciphertexts(hip, oracle, kat)
    for n, d in [(1247, 16), (4096, 32), (65, 4), (63, 4), (130, 5), (8192, 8)]:
        key = make_key(n, d, 6)
        dmask = hip.upload(hip.key_mask(n, key))
        plain = np.random.default_rng(1).integers(0, 2, size=5000).astype(np.uint8)
        use(form)
        mine = hip.download(hip.encrypt_device_rng(n, d, hip.upload(plain), hip.upload(key), dmask, seed=5))
        use("lds")
        other = hip.download(hip.encrypt_device_rng(n, d, hip.upload(plain), hip.upload(key), dmask, seed=5))
        assert np.array_equal(mine, other), (n, d)
        bits = hip.download(hip.decrypt_uniform(n, 5000, 1, hip.upload(mine), dmask))
        assert np.array_equal(bits, plain)


def test_config3_depth10_chain_then_1024x1024(hip, oracle):
    """BASELINE config 3: a depth-10 multiply chain x <- x * (Enc(b) + Enc(b')) grows a fresh
    ciphertext to 2^10 = 1024 terms; two such chains are then multiplied (1024 x 1024 terms).
    Run as a batch on the GPU; every stage checked against the plaintext circuit, the final
    operands and the 1M-term product against the oracle."""
    n, d, dl, B = 1247, 16, 20, 3
    key = make_key(n, d, 51)
    dmask = hip.upload(hip.key_mask(n, key))
    rng = np.random.default_rng(52)

    def chain(seed):
        per = 1 + 20
        plain = rng.integers(0, 2, size=(per, B)).astype(np.uint8)
        fresh = hip.encrypt_device_rng(n, d, hip.upload(plain.reshape(-1)), hip.upload(key), dmask, seed=seed)
        inp = lambda i: fresh[i * B * dl:(i + 1) * B * dl]
        x, xt, xb = inp(0), 1, plain[0].copy()
        for level in range(10):
            rhs = hip.add_uniform(n, B, 1, 1, inp(1 + 2 * level), inp(2 + 2 * level))
            x = hip.mul_uniform(n, B, xt, 2, x, rhs)
            xt *= 2
            xb &= plain[1 + 2 * level] ^ plain[2 + 2 * level]
            assert np.array_equal(hip.download(hip.decrypt_uniform(n, B, xt, x, dmask)), xb), level
        # oracle replay of circuit 0
        hf = hip.download(fresh).reshape(per, B, dl)
        hx = hf[0, 0]
        for level in range(10):
            r, _ = oracle.add(hf[1 + 2 * level, 0], hf[2 + 2 * level, 0])
            hx, _ = oracle.mul(n, hx, r)
        assert xt == 1024 and np.array_equal(hip.download(x[:1024 * dl]), hx)
        return x, xb, hx

    xa, ba, ha = chain(101)
    xc, bc, hc = chain(202)
    prod = hip.mul_uniform(n, B, 1024, 1024, xa, xc)
    bits = hip.download(hip.decrypt_uniform(n, B, 1024 * 1024, prod, dmask))
    assert np.array_equal(bits, ba & bc)
    assert np.array_equal(bits, hip.download(hip.decrypt_combined_uniform(n, B, 1024, 1024, xa, xc, dmask, True)))
    want, _ = oracle.mul(n, ha, hc)
    assert hip.digest(prod[:1024 * 1024 * dl]) == oracle.digest(want)


@pytest.mark.parametrize("dispatch", ["default", "tiled"])
def test_config3_as_written_batch_4096_through_an_arena(hip, oracle, knobs, dispatch):
    """BASELINE config 3 as it is written: batch = 4096 pairs of 1024-term x 1024-term operands, the
    operands being depth-10 multiply chains (x <- x * (Enc(b) + Enc(b')), ten times, on fresh
    ciphertexts), streamed through a small output arena (6 slots, so launches wrap and the last one is
    partial).  Pair p's operands are the two chains of circuit p % 2 with their 1024 terms in a
    per-pair order, so no two pairs multiply the same buffers.  EVERY product still in the arena at
    the end is digested against the oracle (src/Ciphertext.cpp:146-163), once with the library's own
    dispatch for this shape (operand touch pass + flat kernel) and once with the LDS-tiled kernel the
    config names (knob mul_flat = -1)."""
    import torch
    n, d, dl, B, T, slots, B0 = 1247, 16, 20, 4096, 1024, 6, 2
    if dispatch == "tiled":
        knobs.set("mul_flat", -1)
    want_kernel = "k_mul_tiled" if dispatch == "tiled" else "k_touch+k_mul_flat"
    assert hip.lib.csgn_mul_uniform_kernel(n, B, T, T).decode() == want_kernel
    key = make_key(n, d, 71)
    dmask, dkey = hip.upload(hip.key_mask(n, key)), hip.upload(key)
    rng = np.random.default_rng(72)

    def chain(seed):
        per = 1 + 20
        plain = rng.integers(0, 2, size=(per, B0)).astype(np.uint8)
        fresh = hip.encrypt_device_rng(n, d, hip.upload(plain.reshape(-1)), dkey, dmask, seed=seed)
        inp = lambda i: fresh[i * B0 * dl:(i + 1) * B0 * dl]
        x, xt = inp(0), 1
        for level in range(10):
            rhs = hip.add_uniform(n, B0, 1, 1, inp(1 + 2 * level), inp(2 + 2 * level))
            x = hip.mul_uniform(n, B0, xt, 2, x, rhs)
            xt *= 2
        assert xt == T
        return x.view(B0, T, dl)

    ca, cb = chain(303), chain(404)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(73)
    orders = torch.stack([torch.randperm(T, generator=gen) for _ in range(2 * B)]).to(hip.device)   # per pair and side
    L = hip.empty_words(B * T * dl).view(B, T, dl)
    R = hip.empty_words(B * T * dl).view(B, T, dl)
    for c in range(B0):
        sel = torch.arange(c, B, B0, device=hip.device)
        L[sel] = ca[c][orders[sel]]
        R[sel] = cb[c][orders[B + sel]]
    per = T * T * dl
    arena = hip.empty_words(slots * per)
    arena.fill_(-1)
    hip.mul_uniform(n, B, T, T, L.view(-1), R.view(-1), out=arena, out_slots=slots)
    torch.cuda.synchronize()
    # pair q lands in slot q % slots; launches of 6 pairs, the last one holds 4096 - 682*6 = 4 pairs
    last_full = (B // slots) * slots
    survivors = {q % slots: q for q in range(last_full - slots, B)}       # later pairs overwrite earlier ones
    assert sorted(survivors) == list(range(slots)) and survivors[0] == last_full and survivors[slots - 1] == last_full - 1
    for slot, q in survivors.items():
        want, _ = oracle.mul(n, hip.download(L[q].reshape(-1)), hip.download(R[q].reshape(-1)))
        assert hip.digest(arena[slot * per:(slot + 1) * per]) == oracle.digest(want), (dispatch, slot, q)
    # the plaintext of every surviving product, from the materialised words and from the fused form
    bits = hip.download(hip.decrypt_uniform(n, slots, T * T, arena, dmask))
    qs = torch.tensor([survivors[s] for s in range(slots)], device=hip.device)
    fused = hip.download(hip.decrypt_combined_uniform(n, slots, T, T, L[qs].reshape(-1), R[qs].reshape(-1), dmask, True))
    assert np.array_equal(bits, fused)


@pytest.mark.parametrize("n,d,seed", [(1247, 16, 1), (4096, 32, 2), (65, 4, 3), (63, 4, 4)])
def test_fuzz_random_operation_sequences(hip, oracle, n, d, seed):
    """Seeded random walk over the whole C ABI: a pool of device-resident ciphertexts and its
    host twin (oracle) are driven through 150 random mul / add / permute / compact / decrypt
    steps; words and plaintext bits must agree after every step."""
    rng = np.random.default_rng(seed)
    dl = oracle.default_len(n)
    key = make_key(n, d, 60 + seed)
    dmask = hip.upload(hip.key_mask(n, key))
    perm = rng.permutation(n).astype(np.uint64)
    dperm = hip.upload(perm.astype(np.uint32))
    pkey = oracle.permute_key(n, perm, key)
    dpmask = hip.upload(hip.key_mask(n, pkey))
    plain = rng.integers(0, 2, size=8).astype(np.uint8)
    fresh = hip.encrypt_device_rng(n, d, hip.upload(plain), hip.upload(key), dmask, seed=seed)
    pool = [(fresh[i * dl:(i + 1) * dl], hip.download(fresh[i * dl:(i + 1) * dl]).copy(), int(plain[i])) for i in range(8)]
    for step in range(150):
        op = rng.choice(["mul", "add", "add", "permute", "compact", "decrypt"])
        i, j = rng.integers(0, len(pool), size=2)
        (da, ha, ba), (db, hb, bb) = pool[i], pool[j]
        ta, tb = ha.size // dl, hb.size // dl
        if op == "mul" and ta * tb <= 4096 and ta and tb:
            dev = hip.mul_uniform(n, 1, ta, tb, da, db)
            host, _ = oracle.mul(n, ha, hb)
            pool.append((dev, host, ba & bb))
        elif op == "add" and ta + tb <= 4096:
            dev = hip.add_uniform(n, 1, ta, tb, da, db)
            host, _ = oracle.add(ha, hb)
            pool.append((dev, host, ba ^ bb))
        elif op == "permute" and ta >= 1:
            dev = hip.permute_uniform(n, 1, ta, da, dperm)            # reference semantics: first term only
            host = oracle.permute_ciphertext(n, perm, ha)
            assert np.array_equal(hip.download(dev), host)
            got = hip.download(hip.decrypt_uniform(n, 1, 1, dev, dpmask))[0]
            assert got == oracle.decrypt_canonical(n, pkey, host)
            continue
        elif op == "compact" and ta >= 1:
            dev, off_out = hip.compact_ragged(n, da, hip.upload(csr([ta])))
            host = oracle.compact(n, ha)
            assert np.array_equal(hip.download(dev), host)
            if host.size:
                pool.append((dev, host, ba))
        else:
            if ta:
                assert hip.download(hip.decrypt_uniform(n, 1, ta, da, dmask))[0] == oracle.decrypt_canonical(n, key, ha)
            continue
        dev, host, bit = pool[-1]
        assert np.array_equal(hip.download(dev), host), (step, op)
        t = host.size // dl
        if t:
            got = hip.download(hip.decrypt_uniform(n, 1, t, dev, dmask))[0]
            assert got == oracle.decrypt_canonical(n, key, host)
            if d > 1:
                assert got == bit, (step, op)
        if len(pool) > 40:
            pool = pool[:8] + pool[-16:]


@pytest.mark.parametrize("n,d", [(1247, 16), (63, 4), (4096, 32)])
@pytest.mark.parametrize("force_flat", [0, 1])
def test_ragged_skewed_batches(hip, oracle, knobs, n, d, force_flat):
    """Skewed CSR batches (one large pair among many tiny and empty ones, runs of empty pairs
    longer than a workgroup) through both ragged multiply kernels and the ragged add."""
    knobs.set("CSGN_RAGGED_FLAT", str(force_flat))
    dl = oracle.default_len(n)
    rng = np.random.default_rng(n + force_flat)
    t1s = [1, 0, 0, 90, 1] + [0] * 300 + [2, 3] + [1] * 40 + [0, 7]
    t2s = [1, 5, 0, 70, 1] + [0] * 300 + [3, 2] + [1] * 40 + [9, 0]
    offL, offR = csr(t1s), csr(t2s)
    L = oracle.synth(61, n, 0, int(offL[-1]) * dl)
    R = oracle.synth(62, n, 0, int(offR[-1]) * dl)
    dLw, dRw, dOL, dOR = hip.upload(L), hip.upload(R), hip.upload(offL), hip.upload(offR)
    out, off_out = hip.mul_ragged(n, dLw, dOL, dRw, dOR)
    out, off_out = hip.download(out), hip.download(off_out)
    assert np.array_equal(off_out, csr([a * b for a, b in zip(t1s, t2s)]))
    sout, soff = hip.add_ragged(n, dLw, dOL, dRw, dOR)
    sout, soff = hip.download(sout), hip.download(soff)
    assert np.array_equal(soff, offL + offR)
    for b, (t1, t2) in enumerate(zip(t1s, t2s)):
        lh = L[int(offL[b]) * dl:int(offL[b + 1]) * dl]
        rh = R[int(offR[b]) * dl:int(offR[b + 1]) * dl]
        got = out[int(off_out[b]) * dl:int(off_out[b + 1]) * dl]
        if t1 and t2:
            want, _ = oracle.mul(n, lh, rh)
            assert np.array_equal(got, want), b
        else:
            assert got.size == 0
        want_s, _ = oracle.add(lh, rh)
        assert np.array_equal(sout[int(soff[b]) * dl:int(soff[b + 1]) * dl], want_s), b


@pytest.mark.parametrize("n,d,batch", [(1247, 16, 1), (4096, 32, 5), (65, 4, 300)])
def test_circuit_graph_matches_one_by_one_calls_and_oracle(hip, oracle, n, d, batch):
    """csgn_circuit_*: a depth-9 add/multiply circuit with two decrypts, captured into a hipGraph and
    run twice on different inputs, against the one-by-one C-ABI calls (every word, every bit) and
    the oracle (element 0); plus the argument checks."""
    import ctypes as C
    import torch
    from csgn_amd.capi import CsgnError, check
    lib = hip.lib
    dl = oracle.default_len(n)
    key = make_key(n, d, 77)
    dmask = hip.upload(hip.key_mask(n, key))
    c = C.c_void_p()
    check(lib.csgn_circuit_create(n, batch, C.byref(c)))
    def new(fn, *a):
        v = C.c_uint32()
        check(fn(c, *a, C.byref(v)))
        return v.value
    ins = [new(lib.csgn_circuit_input, 1) for _ in range(14)]
    x, k, mid = ins[0], 1, None
    for level in range(1, 10):
        if level % 2:
            x = new(lib.csgn_circuit_add, x, ins[k]); k += 1
        else:
            x = new(lib.csgn_circuit_mul, x, new(lib.csgn_circuit_add, ins[k], ins[k + 1])); k += 2
        if level == 4:
            mid = x
    b_mid = new(lib.csgn_circuit_decrypt, mid, dmask.data_ptr())
    b_end = new(lib.csgn_circuit_decrypt, x, dmask.data_ptr())
    with pytest.raises(CsgnError):
        new(lib.csgn_circuit_add, x, 999)                       # no such value
    assert lib.csgn_circuit_value(c, x) is None                 # nothing allocated before build
    with pytest.raises(CsgnError):
        check(lib.csgn_circuit_run(c, hip.stream))              # not built
    check(lib.csgn_circuit_build(c))
    with pytest.raises(CsgnError):
        new(lib.csgn_circuit_input, 1)                          # frozen after build
    for rnd in range(2):
        plain = np.random.default_rng(10 * rnd + batch).integers(0, 2, size=(14, batch)).astype(np.uint8)
        fresh = hip.encrypt_device_rng(n, d, hip.upload(plain.reshape(-1)), hip.upload(key), dmask, seed=rnd + 5)
        inp = lambda i: fresh[i * batch * dl:(i + 1) * batch * dl]
        for i in range(14):
            check(lib.csgn_memcpy_d2d(lib.csgn_circuit_value(c, ins[i]), inp(i).data_ptr(), batch * dl * 8, hip.stream))
        check(lib.csgn_circuit_run(c, hip.stream))
        # the same circuit, one call at a time
        y, yt, yb, k, y_mid, h = inp(0), 1, plain[0].copy(), 1, None, hip.download(inp(0))[:dl]
        for level in range(1, 10):
            if level % 2:
                y = hip.add_uniform(n, batch, yt, 1, y, inp(k)); yt += 1; yb ^= plain[k]
                h, _ = oracle.add(h, hip.download(inp(k))[:dl]); k += 1
            else:
                r = hip.add_uniform(n, batch, 1, 1, inp(k), inp(k + 1))
                y = hip.mul_uniform(n, batch, yt, 2, y, r); yt *= 2; yb &= plain[k] ^ plain[k + 1]
                hr, _ = oracle.add(hip.download(inp(k))[:dl], hip.download(inp(k + 1))[:dl])
                h, _ = oracle.mul(n, h, hr); k += 2
            if level == 4:
                y_mid, yb_mid = y, yb.copy()
        terms = int(lib.csgn_circuit_value_terms(c, x))
        assert terms == yt == 47
        got = hip.empty_words(batch * terms * dl)
        check(lib.csgn_memcpy_d2d(got.data_ptr(), lib.csgn_circuit_value(c, x), batch * terms * dl * 8, hip.stream))
        assert torch.equal(got, y[:batch * terms * dl])
        assert np.array_equal(hip.download(got)[:terms * dl], h)
        for bid, want in ((b_mid, yb_mid), (b_end, yb)):
            gb = torch.empty(batch, dtype=torch.uint8, device=got.device)
            check(lib.csgn_memcpy_d2d(gb.data_ptr(), lib.csgn_circuit_bits(c, bid), batch, hip.stream))
            if d > 1:
                assert np.array_equal(hip.download(gb), want)
        assert np.array_equal(hip.download(hip.decrypt_uniform(n, batch, yt, y, dmask)),
                              hip.download(gb))
    lib.csgn_circuit_destroy(c)


@pytest.mark.parametrize("n,d,batch,flags", [(1247, 16, 300, 0), (4096, 32, 7, 0), (129, 3, 33, 0), (1247, 16, 300, 23),
                                             (129, 3, 33, 15)])
def test_circuit_with_compaction_bounds_growth(hip, oracle, n, d, batch, flags):
    """csgn_circuit_compact: x <- compact((x + a_k) * (x + a_k)) four times over, then + and Dec, as ONE
    hipGraph.  Uncompacted the chain would square its size every level (2 -> 9 -> 100 -> ... terms); compacted,
    (x + a)^2 = x^2 + a (the cross terms cancel, u & u = u) never grows past the distinct terms.  Every value
    behind the first compaction is DYNAMIC: the device writes its CSR offsets, multiplies run through the
    csgn_mul_ragged_async kernels with launches sized by static bounds.  Offsets, words and bits equal the same
    chain done on the host with the oracle (mul / add / compact / decrypt), on two input sets."""
    import torch
    from csgn_amd.capi import check
    lib = hip.lib
    dl = oracle.default_len(n)
    key = make_key(n, d, 5)
    dmask = hip.upload(hip.key_mask(n, key))
    c = C.c_void_p()
    check(lib.csgn_circuit_create(n, batch, C.byref(c)))
    def new(fn, *a):
        v = C.c_uint32()
        check(fn(c, *a, C.byref(v)))
        return v.value
    levels = 3
    ins = [new(lib.csgn_circuit_input, 1) for _ in range(levels + 2)]
    x = ins[0]
    stages = []
    for k in range(1, levels + 1):
        s_ = new(lib.csgn_circuit_add, x, ins[k])
        x = new(lib.csgn_circuit_compact, new(lib.csgn_circuit_mul, s_, s_))
        stages.append(x)
    y = new(lib.csgn_circuit_add, x, ins[levels + 1])
    bits_x = new(lib.csgn_circuit_decrypt, x, dmask.data_ptr())
    bits_y = new(lib.csgn_circuit_decrypt, y, dmask.data_ptr())
    with pytest.raises(Exception):
        new(lib.csgn_circuit_permute, x, dmask.data_ptr())        # no permutation of a ragged value
    if flags:
        # COMPILED (round 5): dynamic values under liveness, placement and decrypt fusion -- y = x + a is read by its
        # decrypt alone and dissolves into Dec(x) ^ Dec(a) unless it is kept; x and y are kept here because the test reads them
        check(lib.csgn_circuit_optimize(c, flags))
        check(lib.csgn_circuit_output(c, x))
        check(lib.csgn_circuit_output(c, y))
    check(lib.csgn_circuit_build(c))
    if flags:
        assert lib.csgn_circuit_value(c, stages[0]) is None       # an intermediate the compiler did not have to keep
    assert lib.csgn_circuit_value_terms(c, x) == 0                # ragged; the known sizes are bounds
    for rnd in range(2):
        plain = np.random.default_rng(rnd + batch).integers(0, 2, size=(levels + 2, batch)).astype(np.uint8)
        fresh = hip.encrypt_device_rng(n, d, hip.upload(plain.reshape(-1)), hip.upload(key), dmask, seed=rnd + 3)
        hf = hip.download(fresh).reshape(levels + 2, batch, dl)
        if rnd == 1:                                              # some equal inputs: a + a vanishes inside the chain
            hf[1, ::3] = hf[0, ::3]
            fresh = hip.upload(hf.reshape(-1))
        for i in range(levels + 2):
            check(lib.csgn_memcpy_d2d(lib.csgn_circuit_value(c, ins[i]), fresh[i * batch * dl:].data_ptr(), batch * dl * 8, hip.stream))
        check(lib.csgn_circuit_run(c, hip.stream))
        torch.cuda.synchronize()
        # the same chain on the host
        want = [hf[0, b].copy() for b in range(batch)]
        for k in range(1, levels + 1):
            for b in range(batch):
                s_h, _ = oracle.add(want[b], hf[k, b])
                p_h, _ = oracle.mul(n, s_h, s_h) if s_h.size else (s_h, None)
                want[b] = oracle.compact(n, p_h)
        def fetch(v):
            bound = int(lib.csgn_circuit_value_total_terms(c, v))
            off = hip.empty_words(batch + 1)
            check(lib.csgn_memcpy_d2d(off.data_ptr(), lib.csgn_circuit_value_offsets(c, v), (batch + 1) * 8, hip.stream))
            w = hip.empty_words(max(1, bound * dl))
            check(lib.csgn_memcpy_d2d(w.data_ptr(), lib.csgn_circuit_value(c, v), bound * dl * 8, hip.stream))
            return hip.download(off), hip.download(w), bound
        off, words_, bound = fetch(x)
        assert int(off[-1]) <= bound and int(off[-1]) == sum(w.size // dl for w in want)
        for b in range(batch):
            assert np.array_equal(words_[int(off[b]) * dl:int(off[b + 1]) * dl], want[b]), (rnd, b)
            assert want[b].size // dl <= levels + 1               # the chain does not grow: at most the distinct inputs
        offy, wy, _ = fetch(y)
        for b in range(0, batch, max(1, batch // 7)):
            wb, _ = oracle.add(want[b], hf[levels + 1, b])
            assert np.array_equal(wy[int(offy[b]) * dl:int(offy[b + 1]) * dl], wb)
        bx = hip.empty_words(1).new_empty(batch, dtype=torch.uint8)
        check(lib.csgn_memcpy_d2d(bx.data_ptr(), lib.csgn_circuit_bits(c, bits_x), batch, hip.stream))
        by = torch.empty_like(bx)
        check(lib.csgn_memcpy_d2d(by.data_ptr(), lib.csgn_circuit_bits(c, bits_y), batch, hip.stream))
        torch.cuda.synchronize()
        clear = plain[0].copy()
        hfb = plain.copy()
        if rnd == 1:
            hfb[1, ::3] = hfb[0, ::3]
        clear = hfb[0].copy()
        for k in range(1, levels + 1):
            clear ^= hfb[k]                                       # Dec((x + a)^2) = Dec(x + a)
        assert np.array_equal(bx.cpu().numpy(), clear)
        assert np.array_equal(by.cpu().numpy(), clear ^ hfb[levels + 1])
        for b in range(0, batch, max(1, batch // 5)):
            assert oracle.decrypt_canonical(n, key, want[b]) == clear[b]
    lib.csgn_circuit_destroy(c)


@pytest.mark.parametrize("n,d,batch", [(1247, 16, 65536), (1247, 16, 1000), (4096, 32, 77), (65, 3, 5000)])
def test_circuit_graph_fresh_enc_mul_add_dec_as_one_graph(hip, oracle, n, d, batch):
    """BASELINE configs 2 / 4 end to end as ONE hipGraph: two encrypt nodes (keyed generator writing
    straight into the circuit's block), c1*c0 and c1+c0, two decrypts.  Every replay must use a new
    keystream: a node encrypts under its own derived key (csgn_circuit_node_key, restated in the oracle)
    with nonce = run number, bumped on the device; ciphertext words equal the restated definition, bits
    equal the clear circuit."""
    import ctypes as C
    import torch
    from csgn_amd.capi import check
    lib = hip.lib
    dl = oracle.default_len(n)
    key = make_key(n, d, 31)
    dmask, dkey = hip.upload(hip.key_mask(n, key)), hip.upload(key)
    rng = hip.rng_from_seed(99, 8)
    rk, nonce = oracle.rng_from_seed(99)
    nk = oracle.node_key(rk, nonce)
    got_nk = (C.c_uint32 * 8)()
    check(lib.csgn_circuit_node_key(C.byref(rng), got_nk))
    assert list(got_nk) == [int(x) for x in nk] and list(got_nk) != [int(x) for x in rk]
    pa = torch.zeros(batch, dtype=torch.uint8, device=hip.device)
    pb = torch.zeros(batch, dtype=torch.uint8, device=hip.device)
    c = C.c_void_p()
    check(lib.csgn_circuit_create(n, batch, C.byref(c)))
    def new(fn, *a):
        v = C.c_uint32()
        check(fn(c, *a, C.byref(v)))
        return v.value
    first_b = 1 << 40                                           # second node: its own range of the stream
    va = new(lib.csgn_circuit_encrypt, d, pa.data_ptr(), dkey.data_ptr(), dmask.data_ptr(), C.byref(rng), 0)
    vb = new(lib.csgn_circuit_encrypt, d, pb.data_ptr(), dkey.data_ptr(), dmask.data_ptr(), C.byref(rng), first_b)
    vm = new(lib.csgn_circuit_mul, va, vb)
    vs = new(lib.csgn_circuit_add, va, vb)
    bm = new(lib.csgn_circuit_decrypt, vm, dmask.data_ptr())
    bs = new(lib.csgn_circuit_decrypt, vs, dmask.data_ptr())
    check(lib.csgn_circuit_build(c))
    assert lib.csgn_circuit_epoch(c) == 0
    seen = []
    for run in (1, 2, 3):
        ha = np.random.default_rng(run).integers(0, 2, batch).astype(np.uint8)
        hb = np.random.default_rng(100 + run).integers(0, 2, batch).astype(np.uint8)
        pa.copy_(torch.from_numpy(ha))
        pb.copy_(torch.from_numpy(hb))
        check(lib.csgn_circuit_run(c, hip.stream))
        assert lib.csgn_circuit_epoch(c) == run
        def grab(v, terms):
            t = hip.empty_words(batch * terms * dl)
            check(lib.csgn_memcpy_d2d(t.data_ptr(), lib.csgn_circuit_value(c, v), batch * terms * dl * 8, hip.stream))
            return t
        ca, cb = grab(va, 1), grab(vb, 1)
        sample = slice(0, min(batch, 3000) * dl)
        assert np.array_equal(hip.download(ca)[sample],
                              oracle.encrypt_keyed(n, key, ha[:min(batch, 3000)], nk, run, 8))
        assert np.array_equal(hip.download(cb)[sample],
                              oracle.encrypt_keyed(n, key, hb[:min(batch, 3000)], nk, run, 8, first_ciphertext=first_b))
        assert torch.equal(grab(vm, 1), ca & cb)                # src/Ciphertext.cpp:124-131
        both = grab(vs, 2).view(batch, 2 * dl)
        assert torch.equal(both[:, :dl].reshape(-1), ca) and torch.equal(both[:, dl:].reshape(-1), cb)
        for bid, want in ((bm, ha & hb), (bs, ha ^ hb)):
            gb = torch.empty(batch, dtype=torch.uint8, device=hip.device)
            check(lib.csgn_memcpy_d2d(gb.data_ptr(), lib.csgn_circuit_bits(c, bid), batch, hip.stream))
            assert np.array_equal(hip.download(gb), want)
        seen.append(hip.download(ca)[:dl].copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])   # no keystream re-use
    lib.csgn_circuit_destroy(c)


@pytest.mark.parametrize("n,d,batch", [(1247, 16, 65536), (4096, 32, 77), (65, 3, 5000)])
def test_circuit_graph_fused_fresh_chain_node(hip, oracle, n, d, batch):
    """csgn_circuit_encrypt_mul: Enc*Enc (+Dec) as ONE graph node.  Words equal the restated definition under
    the two derived node keys with nonce = run number, bits equal b1 & b0 (computed by the kernel from the
    generated words: checked against csgn_decrypt_uniform of the product), every replay differs."""
    import ctypes as C
    import torch
    from csgn_amd.capi import check
    lib = hip.lib
    dl = oracle.default_len(n)
    key = make_key(n, d, 41)
    dmask, dkey = hip.upload(hip.key_mask(n, key)), hip.upload(key)
    ra, rb = hip.rng_from_seed(199, 8), hip.rng_from_seed(299, 8)
    (ka, na), (kb, nb) = oracle.rng_from_seed(199), oracle.rng_from_seed(299)
    nka, nkb = oracle.node_key(ka, na), oracle.node_key(kb, nb)
    pa = torch.zeros(batch, dtype=torch.uint8, device=hip.device)
    pb = torch.zeros(batch, dtype=torch.uint8, device=hip.device)
    c = C.c_void_p()
    check(lib.csgn_circuit_create(n, batch, C.byref(c)))
    vf, bf = C.c_uint32(), C.c_uint32()
    first = 12345
    check(lib.csgn_circuit_encrypt_mul(c, d, pa.data_ptr(), pb.data_ptr(), dkey.data_ptr(), dmask.data_ptr(), C.byref(ra),
                                       C.byref(rb), first, C.byref(vf), C.byref(bf)))
    assert lib.csgn_circuit_encrypt_mul(c, d, pa.data_ptr(), pb.data_ptr(), dkey.data_ptr(), dmask.data_ptr(), C.byref(ra),
                                        C.byref(ra), first, C.byref(vf), None) == -1          # the same stream twice
    check(lib.csgn_circuit_build(c))
    prev = None
    for run in (1, 2, 3):
        ha = np.random.default_rng(run).integers(0, 2, batch).astype(np.uint8)
        hb = np.random.default_rng(200 + run).integers(0, 2, batch).astype(np.uint8)
        pa.copy_(torch.from_numpy(ha))
        pb.copy_(torch.from_numpy(hb))
        check(lib.csgn_circuit_run(c, hip.stream))
        prod = hip.empty_words(batch * dl)
        check(lib.csgn_memcpy_d2d(prod.data_ptr(), lib.csgn_circuit_value(c, vf.value), batch * dl * 8, hip.stream))
        k = min(batch, 3000)
        want = (oracle.encrypt_keyed(n, key, ha[:k], nka, run, 8, first_ciphertext=first)
                & oracle.encrypt_keyed(n, key, hb[:k], nkb, run, 8, first_ciphertext=first))
        assert np.array_equal(hip.download(prod)[:k * dl], want), run
        gb = torch.empty(batch, dtype=torch.uint8, device=hip.device)
        check(lib.csgn_memcpy_d2d(gb.data_ptr(), lib.csgn_circuit_bits(c, bf.value), batch, hip.stream))
        bits = hip.download(gb)
        assert np.array_equal(bits, hip.download(hip.decrypt_uniform(n, batch, 1, prod, dmask)))
        if len(set(int(x) for x in key)) > 1:
            assert np.array_equal(bits, ha & hb)
        if prev is not None:
            assert not torch.equal(prod, prev)
        prev = prod
    lib.csgn_circuit_destroy(c)


@pytest.mark.parametrize("flags", [0, 23, 31])
def test_circuit_compiled_with_encrypt_nodes(hip, oracle, flags):
    """Encrypt nodes under the compiler: e1 = Enc(a), e2 = Enc(b) generated inside the graph, Dec(e1 + e2), Dec(e1 * e2)
    and a fused Enc*Enc node that is kept for its bits only (its value has no reader: it must still have somewhere to be
    written).  Tape and compiled give a ^ b, a & b, a & b on three runs with new plaintexts; in the compiled graph the sum
    and the product are never computed (both decrypts fused) and the fused node's value is not addressable."""
    import ctypes as C
    import torch
    from csgn_amd.capi import check
    lib = hip.lib
    n, d, batch = 1247, 16, 500
    key = make_key(n, d, 43)
    dmask, dkey = hip.upload(hip.key_mask(n, key)), hip.upload(key)
    r1, r2, r3, r4 = (hip.rng_from_seed(500 + i, 8) for i in range(4))
    pa = torch.zeros(batch, dtype=torch.uint8, device=hip.device)
    pb = torch.zeros(batch, dtype=torch.uint8, device=hip.device)
    c = C.c_void_p()
    check(lib.csgn_circuit_create(n, batch, C.byref(c)))
    def new(fn, *a):
        v = C.c_uint32()
        check(fn(c, *a, C.byref(v)))
        return v.value
    e1 = new(lib.csgn_circuit_encrypt, d, pa.data_ptr(), dkey.data_ptr(), dmask.data_ptr(), C.byref(r1), 0)
    e2 = new(lib.csgn_circuit_encrypt, d, pb.data_ptr(), dkey.data_ptr(), dmask.data_ptr(), C.byref(r2), batch)
    vf, bf = C.c_uint32(), C.c_uint32()
    check(lib.csgn_circuit_encrypt_mul(c, d, pa.data_ptr(), pb.data_ptr(), dkey.data_ptr(), dmask.data_ptr(), C.byref(r3),
                                       C.byref(r4), 2 * batch, C.byref(vf), C.byref(bf)))
    vs = new(lib.csgn_circuit_add, e1, e2)
    vp = new(lib.csgn_circuit_mul, e1, e2)
    b_s = new(lib.csgn_circuit_decrypt, vs, dmask.data_ptr())
    b_p = new(lib.csgn_circuit_decrypt, vp, dmask.data_ptr())
    if flags:
        check(lib.csgn_circuit_optimize(c, flags))
    check(lib.csgn_circuit_build(c))
    try:
        if flags:
            st = (C.c_uint64 * 8)()
            check(lib.csgn_circuit_stats(c, st))
            assert st[5] == 2 and st[6] == 2                         # two decrypts fused, sum and product dropped
            assert lib.csgn_circuit_value(c, vf.value) is None and lib.csgn_circuit_value(c, vs) is None
        for run in range(3):
            ha = np.random.default_rng(run).integers(0, 2, batch).astype(np.uint8)
            hb = np.random.default_rng(50 + run).integers(0, 2, batch).astype(np.uint8)
            pa.copy_(torch.from_numpy(ha))
            pb.copy_(torch.from_numpy(hb))
            check(lib.csgn_circuit_run(c, hip.stream))
            got = {}
            for name, bid in (("sum", b_s), ("product", b_p), ("fused", bf.value)):
                gb = torch.empty(batch, dtype=torch.uint8, device=hip.device)
                check(lib.csgn_memcpy_d2d(gb.data_ptr(), lib.csgn_circuit_bits(c, bid), batch, hip.stream))
                got[name] = hip.download(gb)
            assert np.array_equal(got["sum"], ha ^ hb), run
            assert np.array_equal(got["product"], ha & hb), run
            assert np.array_equal(got["fused"], ha & hb), run
    finally:
        lib.csgn_circuit_destroy(c)


@pytest.mark.parametrize("flags", [0, 31])
def test_circuit_compaction_of_values_beyond_one_workgroup_inside_a_graph(hip, oracle, flags):
    """csgn_circuit_compact on a value whose static bound is beyond the wide build's group ((a + b)^2 with 46-term
    inputs: 8464 product terms): the hash-partition kernels (1024-thread scatter with 120 KB of LDS set by
    hipFuncSetAttribute, dedup, the no-op exact path) are captured into the circuit's graph.  92 terms survive of every
    element (the cross terms cancel), words equal the oracle's on two input sets, tape and compiled."""
    import torch
    from csgn_amd.capi import check
    lib = hip.lib
    n, batch, T = 1247, 3, 46
    dl = oracle.default_len(n)
    c = C.c_void_p()
    check(lib.csgn_circuit_create(n, batch, C.byref(c)))
    def new(fn, *a):
        v = C.c_uint32()
        check(fn(c, *a, C.byref(v)))
        return v.value
    ia, ib = new(lib.csgn_circuit_input, T), new(lib.csgn_circuit_input, T)
    s_ = new(lib.csgn_circuit_add, ia, ib)
    x = new(lib.csgn_circuit_compact, new(lib.csgn_circuit_mul, s_, s_))
    if flags:
        check(lib.csgn_circuit_optimize(c, flags))
        check(lib.csgn_circuit_output(c, x))
    check(lib.csgn_circuit_build(c))
    try:
        for rnd in range(2):
            ha = oracle.synth(300 + rnd, n, 0, batch * T * dl)
            hb = oracle.synth(310 + rnd, n, 0, batch * T * dl)
            for v, h in ((ia, ha), (ib, hb)):
                d = hip.upload(h)
                check(lib.csgn_memcpy_d2d(lib.csgn_circuit_value(c, v), d.data_ptr(), h.size * 8, hip.stream))
            check(lib.csgn_circuit_run(c, hip.stream))
            torch.cuda.synchronize()
            bound = int(lib.csgn_circuit_value_total_terms(c, x))
            off = hip.empty_words(batch + 1)
            check(lib.csgn_memcpy_d2d(off.data_ptr(), lib.csgn_circuit_value_offsets(c, x), (batch + 1) * 8, hip.stream))
            w = hip.empty_words(bound * dl)
            check(lib.csgn_memcpy_d2d(w.data_ptr(), lib.csgn_circuit_value(c, x), bound * dl * 8, hip.stream))
            off, w = hip.download(off), hip.download(w)
            for b in range(batch):
                sh, _ = oracle.add(ha[b * T * dl:(b + 1) * T * dl], hb[b * T * dl:(b + 1) * T * dl])
                ph, _ = oracle.mul(n, sh, sh)
                want = oracle.compact(n, ph)
                assert want.size // dl == 2 * T
                assert np.array_equal(w[int(off[b]) * dl:int(off[b + 1]) * dl], want), (rnd, b)
    finally:
        lib.csgn_circuit_destroy(c)


@pytest.mark.parametrize("n,d,batch", [(1247, 16, 300), (4096, 32, 40), (65, 4, 1000)])
def test_circuit_graph_ragged_values(hip, oracle, n, d, batch):
    _ragged_circuit(hip, oracle, n, d, batch, 0, True)


@pytest.mark.parametrize("flags,keep", [(23, True), (23, False), (31, False), (3, True)])
def test_circuit_graph_ragged_values_compiled(hip, oracle, flags, keep):
    """The same circuit COMPILED: with x and s kept their words and offsets are the tape's; with nothing kept only the
    bits exist -- Dec(x) = Dec(s) & Dec(a + u) from the materialised s (it has a second reader: its own decrypt) and the
    sum a + u, or with PUSHDOWN from the leaves."""
    _ragged_circuit(hip, oracle, 1247, 16, 200, flags, keep)


def _ragged_circuit(hip, oracle, n, d, batch, flags, keep):
    """Ragged values in a captured circuit (static per-element shapes): x = (a*b + c) * (a + u) with
    ragged a, b, c (0..5 terms per element, empty ones included) and a uniform u, two decrypts.  Words
    against the one-by-one CSR calls and, per sampled element, the oracle; bits against the oracle."""
    import ctypes as C
    import torch
    from csgn_amd.capi import CsgnError, check
    lib = hip.lib
    dl = oracle.default_len(n)
    rng = np.random.default_rng(n + batch)
    key = make_key(n, d, 5)
    dmask = hip.upload(hip.key_mask(n, key))
    ta, tb, tc = (rng.integers(0, 6, size=batch).astype(np.uint64) for _ in range(3))
    c = C.c_void_p()
    check(lib.csgn_circuit_create(n, batch, C.byref(c)))
    def new(fn, *a):
        v = C.c_uint32()
        check(fn(c, *a, C.byref(v)))
        return v.value
    va = new(lib.csgn_circuit_input_ragged, ta.ctypes.data)
    vb = new(lib.csgn_circuit_input_ragged, tb.ctypes.data)
    vc = new(lib.csgn_circuit_input_ragged, tc.ctypes.data)
    vu = new(lib.csgn_circuit_input, 2)
    vab = new(lib.csgn_circuit_mul, va, vb)
    vs = new(lib.csgn_circuit_add, vab, vc)
    vau = new(lib.csgn_circuit_add, va, vu)
    vx = new(lib.csgn_circuit_mul, vs, vau)
    b_s = new(lib.csgn_circuit_decrypt, vs, dmask.data_ptr())
    b_x = new(lib.csgn_circuit_decrypt, vx, dmask.data_ptr())
    with pytest.raises(CsgnError):
        new(lib.csgn_circuit_permute, va, dmask.data_ptr())     # ragged permute: refused
    if flags:
        check(lib.csgn_circuit_optimize(c, flags))
        if keep:
            check(lib.csgn_circuit_output(c, vx))
            check(lib.csgn_circuit_output(c, vs))
    check(lib.csgn_circuit_build(c))
    assert lib.csgn_circuit_value_terms(c, vx) == 0 and lib.csgn_circuit_value_terms(c, vu) == 2
    tx = (ta * tb + tc) * (ta + 2)
    assert lib.csgn_circuit_value_total_terms(c, vx) == int(tx.sum())
    # inputs: planted so that decryptions are not all zero
    def fill(v, terms, seed):
        total = int(terms.sum())
        w = oracle.synth(seed, n, 0, max(total, 1) * dl)[:total * dl].reshape(total, dl)
        hit = np.random.default_rng(seed).integers(0, 2, total).astype(bool)
        w[hit] |= oracle.key_mask(n, key)
        w = np.ascontiguousarray(w.reshape(-1))
        if total:
            check(lib.csgn_memcpy_h2d(lib.csgn_circuit_value(c, v), w.ctypes.data, w.size * 8, hip.stream))
        return w
    ha, hb, hc = fill(va, ta, 1), fill(vb, tb, 2), fill(vc, tc, 3)
    hu = fill(vu, np.full(batch, 2, dtype=np.uint64), 4)
    check(lib.csgn_circuit_run(c, hip.stream))
    torch.cuda.synchronize()
    def grab(v):
        total = int(lib.csgn_circuit_value_total_terms(c, v))
        t = hip.empty_words(max(total * dl, 1))
        check(lib.csgn_memcpy_d2d(t.data_ptr(), lib.csgn_circuit_value(c, v), total * dl * 8, hip.stream))
        return hip.download(t)[:total * dl]
    off = lambda t: np.concatenate([[0], np.cumsum(t)]).astype(np.int64)
    oa, ob, oc, ox, os_ = off(ta), off(tb), off(tc), off(tx), off(ta * tb + tc)
    if keep:
        gx, gs = grab(vx), grab(vs)
        got_off = torch.empty(batch + 1, dtype=torch.int64, device=hip.device)
        check(lib.csgn_memcpy_d2d(got_off.data_ptr(), lib.csgn_circuit_value_offsets(c, vx), (batch + 1) * 8, hip.stream))
        assert np.array_equal(hip.download(got_off).astype(np.int64), ox)
    else:
        assert lib.csgn_circuit_value(c, vx) is None and lib.csgn_circuit_value_offsets(c, vx) is None
    bits = {}
    for name, bid in (("s", b_s), ("x", b_x)):
        gb = torch.empty(batch, dtype=torch.uint8, device=hip.device)
        check(lib.csgn_memcpy_d2d(gb.data_ptr(), lib.csgn_circuit_bits(c, bid), batch, hip.stream))
        bits[name] = hip.download(gb)
    for i in range(0, batch, max(1, batch // 60)):
        a_i, b_i, c_i = ha[oa[i] * dl:oa[i + 1] * dl], hb[ob[i] * dl:ob[i + 1] * dl], hc[oc[i] * dl:oc[i + 1] * dl]
        u_i = hu[2 * i * dl:2 * (i + 1) * dl]
        ab = oracle.mul(n, a_i, b_i)[0] if a_i.size and b_i.size else np.zeros(0, dtype=np.uint64)
        s_i = np.concatenate([ab, c_i])
        au = np.concatenate([a_i, u_i])
        x_i = oracle.mul(n, s_i, au)[0] if s_i.size else np.zeros(0, dtype=np.uint64)
        if keep:
            assert np.array_equal(gs[os_[i] * dl:os_[i + 1] * dl], s_i), i
            assert np.array_equal(gx[ox[i] * dl:ox[i + 1] * dl], x_i), i
        assert bits["s"][i] == (oracle.decrypt_canonical(n, key, s_i) if s_i.size else 0)
        assert bits["x"][i] == (oracle.decrypt_canonical(n, key, x_i) if x_i.size else 0)
    assert bits["x"].any() or bits["s"].any()
    lib.csgn_circuit_destroy(c)


@pytest.mark.parametrize("batch", [1, 3, 200])
def test_circuit_graph_config5_with_permutation(hip, oracle, batch):
    """BASELINE config 5 as ONE hipGraph: Context(4096,32), a random Permutation applied to every
    fresh input inside the graph, the depth-16 add/multiply circuit (766 terms), decrypt under the
    permuted key.  Bits equal the circuit in the clear; words of element 0 equal the oracle's."""
    import ctypes as C
    import torch
    from csgn_amd.capi import check
    lib = hip.lib
    n, d, levels = 4096, 32, 16
    dl = oracle.default_len(n)
    key = make_key(n, d, 21)
    perm = np.random.default_rng(22).permutation(n).astype(np.uint64)
    pkey = oracle.permute_key(n, perm, key)
    dmask, dpmask = hip.upload(hip.key_mask(n, key)), hip.upload(hip.key_mask(n, pkey))
    dperm = hip.upload(perm.astype(np.uint32))
    nin = 1 + levels // 2 + 2 * (levels // 2)
    c = C.c_void_p()
    check(lib.csgn_circuit_create(n, batch, C.byref(c)))
    def new(fn, *a):
        v = C.c_uint32()
        check(fn(c, *a, C.byref(v)))
        return v.value
    raw = [new(lib.csgn_circuit_input, 1) for _ in range(nin)]
    ins = [new(lib.csgn_circuit_permute, r, dperm.data_ptr()) for r in raw]
    x, k = ins[0], 1
    for level in range(1, levels + 1):
        if level % 2:
            x = new(lib.csgn_circuit_add, x, ins[k]); k += 1
        else:
            x = new(lib.csgn_circuit_mul, x, new(lib.csgn_circuit_add, ins[k], ins[k + 1])); k += 2
    bid = new(lib.csgn_circuit_decrypt, x, dpmask.data_ptr())
    check(lib.csgn_circuit_build(c))
    plain = np.random.default_rng(batch).integers(0, 2, size=(nin, batch)).astype(np.uint8)
    fresh = hip.encrypt_device_rng(n, d, hip.upload(plain.reshape(-1)), hip.upload(key), dmask, seed=9)
    for i in range(nin):
        check(lib.csgn_memcpy_d2d(lib.csgn_circuit_value(c, raw[i]), fresh[i * batch * dl:].data_ptr(),
                                  batch * dl * 8, hip.stream))
    check(lib.csgn_circuit_run(c, hip.stream))
    xb, k = plain[0].copy(), 1
    hf = hip.download(fresh).reshape(nin, batch, dl)
    h = oracle.permute_ciphertext(n, perm, hf[0, 0])
    for level in range(1, levels + 1):
        if level % 2:
            xb ^= plain[k]
            h, _ = oracle.add(h, oracle.permute_ciphertext(n, perm, hf[k, 0])); k += 1
        else:
            xb &= plain[k] ^ plain[k + 1]
            r, _ = oracle.add(oracle.permute_ciphertext(n, perm, hf[k, 0]), oracle.permute_ciphertext(n, perm, hf[k + 1, 0]))
            h, _ = oracle.mul(n, h, r); k += 2
    assert int(lib.csgn_circuit_value_terms(c, x)) == 766
    gb = torch.empty(batch, dtype=torch.uint8, device=fresh.device)
    check(lib.csgn_memcpy_d2d(gb.data_ptr(), lib.csgn_circuit_bits(c, bid), batch, hip.stream))
    assert np.array_equal(hip.download(gb), xb)
    got = hip.empty_words(766 * dl)
    check(lib.csgn_memcpy_d2d(got.data_ptr(), lib.csgn_circuit_value(c, x), 766 * dl * 8, hip.stream))
    assert np.array_equal(hip.download(got), h)
    assert oracle.decrypt_canonical(n, pkey, h) == xb[0]
    lib.csgn_circuit_destroy(c)


@pytest.mark.parametrize("n,d,batch,flags", [(1247, 16, 5, 23), (4096, 32, 3, 23), (130, 3, 70, 7), (1247, 16, 9, 31),
                                             (1247, 16, 5, 2), (4096, 32, 4, 5), (130, 3, 11, 17)])
def test_circuit_compiled_matches_tape_on_random_dags(hip, oracle, n, d, batch, flags):
    """The compiler property on the real kernels: 60 random DAG circuits -- chains, shared
    sub-expressions, a*a and a+a, values nobody reads, several decrypts, random retained outputs -- built twice, as a
    TAPE and COMPILED (liveness + placement + decrypt fusion + the prologue copy launch; one parameter set with
    PUSHDOWN, three with some of the passes only).  Every bit vector of the compiled graph equals the tape's and the circuit evaluated in the clear on
    the plaintext bits; every retained value is word-identical to the tape's; values the compiler did not retain
    answer NULL; element 0 of every retained value equals the oracle's mul/add chain; the compiled block is
    never larger than the tape's."""
    import ctypes as C
    import torch
    from csgn_amd.capi import check
    lib = hip.lib
    dl = oracle.default_len(n)
    key = make_key(n, d, 31)
    dmask = hip.upload(hip.key_mask(n, key))
    dkey = hip.upload(key)
    placed = fused = hoisted = 0
    for seed in range(60):
        tape = random_circuit(lib, 3000 + seed, n, batch, dmask.data_ptr(), max_terms=300)
        comp = random_circuit(lib, 3000 + seed, n, batch, dmask.data_ptr(), max_terms=300)
        try:
            check(lib.csgn_circuit_optimize(comp.c, flags))             # (the generator marked the same outputs on both)
            check(lib.csgn_circuit_build(tape.c))
            check(lib.csgn_circuit_build(comp.c))
            assert lib.csgn_circuit_block_bytes(comp.c) <= lib.csgn_circuit_block_bytes(tape.c)
            stats = (C.c_uint64 * 8)()
            check(lib.csgn_circuit_stats(comp.c, stats))
            placed += stats[4]
            fused += stats[5]
            hoisted += stats[7]
            ins = [v for v, nd in enumerate(tape.nodes) if nd[0] == "in"]
            nterms = sum(tape.terms[v] for v in ins)
            plain = np.random.default_rng(seed).integers(0, 2, size=(nterms, batch)).astype(np.uint8)
            fresh = hip.encrypt_device_rng(n, d, hip.upload(plain.reshape(-1)), dkey, dmask, seed=seed + 1)
            # input v, element e = the terms' fresh ciphertexts side by side; clear value = XOR of their bits
            row, clear, host = 0, {}, {}
            hf = hip.download(fresh).reshape(nterms, batch, dl)
            for v in ins:
                t = tape.terms[v]
                words = np.ascontiguousarray(hf[row:row + t].transpose(1, 0, 2))      # [batch, t, dl]
                clear[v] = np.bitwise_xor.reduce(plain[row:row + t], axis=0)
                host[v] = words
                dw = hip.upload(words.reshape(-1))
                for c in (tape.c, comp.c):
                    check(lib.csgn_memcpy_d2d(lib.csgn_circuit_value(c, v), dw.data_ptr(), batch * t * dl * 8, hip.stream))
                row += t
            check(lib.csgn_circuit_run(tape.c, hip.stream))
            check(lib.csgn_circuit_run(comp.c, hip.stream))
            torch.cuda.synchronize()
            for v, nd in enumerate(tape.nodes):
                if nd[0] == "add":
                    clear[v] = clear[nd[1]] ^ clear[nd[2]]
                elif nd[0] == "mul":
                    clear[v] = clear[nd[1]] & clear[nd[2]]
            def fetch(c, ptr, nbytes, dtype):
                t = torch.empty(nbytes // np.dtype(dtype).itemsize, dtype=torch.int64 if dtype == np.uint64 else torch.uint8,
                                device=fresh.device)
                check(lib.csgn_memcpy_d2d(t.data_ptr(), ptr, nbytes, hip.stream))
                return hip.download(t)
            for bid, v in enumerate(tape.decrypts):
                bt = fetch(tape.c, lib.csgn_circuit_bits(tape.c, bid), batch, np.uint8)
                bc = fetch(comp.c, lib.csgn_circuit_bits(comp.c, bid), batch, np.uint8)
                assert np.array_equal(bt, bc), (seed, bid)
                if d >= 16:                                              # (a 3-index key hits by chance)
                    assert np.array_equal(bc, clear[v]), (seed, bid)
            for v in range(len(tape.terms)):
                ptr = lib.csgn_circuit_value(comp.c, v)
                if v in tape.outputs or tape.nodes[v][0] == "in":
                    assert ptr is not None, (seed, v)
                    nb = batch * tape.terms[v] * dl * 8
                    wc = fetch(comp.c, ptr, nb, np.uint64)
                    wt = fetch(tape.c, lib.csgn_circuit_value(tape.c, v), nb, np.uint64)
                    assert np.array_equal(wc, wt), (seed, v)
                else:
                    assert ptr is None, (seed, v)
            # element 0 of the retained outputs against the oracle's chain
            want0 = {}
            def oracle_value(v):
                if v in want0:
                    return want0[v]
                nd = tape.nodes[v]
                if nd[0] == "in":
                    r = np.ascontiguousarray(host[v][0].reshape(-1))
                elif nd[0] == "add":
                    r, _ = oracle.add(oracle_value(nd[1]), oracle_value(nd[2]))
                else:
                    r, _ = oracle.mul(n, oracle_value(nd[1]), oracle_value(nd[2]))
                want0[v] = r
                return r
            for v in tape.outputs:
                got = fetch(comp.c, lib.csgn_circuit_value(comp.c, v), tape.terms[v] * dl * 8, np.uint64)
                assert np.array_equal(got, oracle_value(v)), (seed, v)
        finally:
            tape.close()
            comp.close()
    if flags & 2:
        assert placed > 20
    if flags & 12:
        assert fused > 20
    if flags & 16:
        assert hoisted > 20


@pytest.mark.parametrize("n,d,batch", [(4096, 32, 64), (1247, 16, 300), (1247, 16, 1)])
def test_circuit_compiled_config5(hip, oracle, n, d, batch):
    """BASELINE config 5 compiled (tests/basic_operations.cpp:34-40 style flow, depth 16, 766 terms): bits equal the tape's
    and the clear circuit; with the final value marked as an output its words equal the tape's and (element 0) the
    oracle's; the stats say what the compiler did (7 products placed, 1 decrypt fused, the last product and the add
    in front of nothing dropped), and a second run on new inputs is right too (regions are reused ACROSS runs)."""
    import ctypes as C
    import torch
    from csgn_amd.capi import check
    lib = hip.lib
    dl = oracle.default_len(n)
    key = make_key(n, d, 5)
    dmask, dkey = hip.upload(hip.key_mask(n, key)), hip.upload(key)
    tape, x = config5(lib, n, batch, mask_ptr=dmask.data_ptr())
    comp, _ = config5(lib, n, batch, mask_ptr=dmask.data_ptr())
    kept, _ = config5(lib, n, batch, mask_ptr=dmask.data_ptr())
    ins = [v for v, nd in enumerate(tape.nodes) if nd[0] == "in"]
    try:
        check(lib.csgn_circuit_optimize(comp.c, 23))
        check(lib.csgn_circuit_optimize(kept.c, 23))
        kept.output(x)
        for c in (tape, comp, kept):
            check(lib.csgn_circuit_build(c.c))
        st = (C.c_uint64 * 8)()
        check(lib.csgn_circuit_stats(comp.c, st))
        assert st[4] == 7 and st[5] == 1 and st[6] == 1                   # placed, fused, dropped (the last product)
        assert st[7] == 25 and st[3] == 11     # all 25 input copies in the prologue: 7 products + 1 copy launch + 2 decrypts + 1 combine
        st_t = (C.c_uint64 * 8)()
        check(lib.csgn_circuit_stats(tape.c, st_t))
        assert st[1] * 2 < st_t[1] and st[0] * 2 < st_t[0]                # algorithmic bytes and block: less than half
        assert lib.csgn_circuit_value(comp.c, x) is None and lib.csgn_circuit_value(kept.c, x) is not None
        for rnd in range(2):
            plain = np.random.default_rng(rnd + batch).integers(0, 2, size=(25, batch)).astype(np.uint8)
            fresh = hip.encrypt_device_rng(n, d, hip.upload(plain.reshape(-1)), dkey, dmask, seed=rnd + 3)
            for c in (tape, comp, kept):
                for i in range(25):
                    check(lib.csgn_memcpy_d2d(lib.csgn_circuit_value(c.c, ins[i]), fresh[i * batch * dl:].data_ptr(),
                                              batch * dl * 8, hip.stream))
                check(lib.csgn_circuit_run(c.c, hip.stream))
            xb, k = plain[0].copy(), 1
            for level in range(1, 17):
                if level % 2:
                    xb ^= plain[k]; k += 1
                else:
                    xb &= plain[k] ^ plain[k + 1]; k += 2
            got = {}
            for name, c in (("tape", tape), ("comp", comp), ("kept", kept)):
                gb = torch.empty(batch, dtype=torch.uint8, device=fresh.device)
                check(lib.csgn_memcpy_d2d(gb.data_ptr(), lib.csgn_circuit_bits(c.c, 0), batch, hip.stream))
                got[name] = hip.download(gb)
                assert np.array_equal(got[name], xb), (name, rnd)
            wt, wk = hip.empty_words(batch * 766 * dl), hip.empty_words(batch * 766 * dl)
            check(lib.csgn_memcpy_d2d(wt.data_ptr(), lib.csgn_circuit_value(tape.c, x), batch * 766 * dl * 8, hip.stream))
            check(lib.csgn_memcpy_d2d(wk.data_ptr(), lib.csgn_circuit_value(kept.c, x), batch * 766 * dl * 8, hip.stream))
            assert torch.equal(wt, wk)
            hf = hip.download(fresh).reshape(25, batch, dl)
            h, k = hf[0, 0], 1
            for level in range(1, 17):
                if level % 2:
                    h, _ = oracle.add(h, hf[k, 0]); k += 1
                else:
                    r, _ = oracle.add(hf[k, 0], hf[k + 1, 0])
                    h, _ = oracle.mul(n, h, r); k += 2
            assert np.array_equal(hip.download(wk)[:766 * dl], h)
    finally:
        for c in (tape, comp, kept):
            c.close()


def test_circuit_decrypts_a_long_uniform_value_uploaded_just_before_the_run(hip, oracle):
    """a circuit whose decrypt takes the long-uniform path (> 4096 terms per element: per-ciphertext partial
    words are zero-filled inside the graph, by a KERNEL node like every zero fill a circuit may capture), inputs
    uploaded IMMEDIATELY before csgn_circuit_run on the same stream, five times over with new inputs: the bits equal the
    one-by-one decrypt, the oracle and the clear product.  (The hipMemsetAsync form of the fill -- dev knob
    zero_memset, tools/graph_memset_case.py -- returned ONE wrong bit in this test's second run inside the suite's
    process and none in 240 runs alone; DESIGN 4.9 has the record.)"""
    import ctypes as C
    import torch
    from csgn_amd.capi import check
    lib = hip.lib
    n, d, batch, t = 1247, 16, 3, 70
    dl = oracle.default_len(n)
    key = make_key(n, d, 3)
    dmask = hip.upload(hip.key_mask(n, key))
    c = C.c_void_p()
    check(lib.csgn_circuit_create(n, batch, C.byref(c)))
    def new(fn, *a):
        v = C.c_uint32()
        check(fn(c, *a, C.byref(v)))
        return v.value
    a, b = new(lib.csgn_circuit_input, t), new(lib.csgn_circuit_input, t)
    p = new(lib.csgn_circuit_mul, a, b)                                  # 4900 terms per element
    bid = new(lib.csgn_circuit_decrypt, p, dmask.data_ptr())
    check(lib.csgn_circuit_build(c))
    try:
        for rnd in range(5):
            plain = np.random.default_rng(rnd).integers(0, 2, size=2 * t * batch).astype(np.uint8)
            fresh = hip.encrypt_device_rng(n, d, hip.upload(plain), hip.upload(key), dmask, seed=rnd + 40)
            torch.cuda.synchronize()
            half = batch * t * dl
            check(lib.csgn_memcpy_d2d(lib.csgn_circuit_value(c, a), fresh.data_ptr(), half * 8, hip.stream))
            check(lib.csgn_memcpy_d2d(lib.csgn_circuit_value(c, b), fresh[half:].data_ptr(), half * 8, hip.stream))
            check(lib.csgn_circuit_run(c, hip.stream))
            gb = torch.empty(batch, dtype=torch.uint8, device=fresh.device)
            check(lib.csgn_memcpy_d2d(gb.data_ptr(), lib.csgn_circuit_bits(c, bid), batch, hip.stream))
            prod = hip.mul_uniform(n, batch, t, t, fresh[:half], fresh[half:])
            want = hip.download(hip.decrypt_uniform(n, batch, t * t, prod, dmask))
            got = hip.download(gb)
            assert np.array_equal(got, want), rnd
            h0 = hip.download(prod)[:t * t * dl]
            assert got[0] == oracle.decrypt_canonical(n, key, h0)
            pb = plain.reshape(2, batch, t)
            assert np.array_equal(got, np.bitwise_xor.reduce(pb[0], axis=1) & np.bitwise_xor.reduce(pb[1], axis=1))
    finally:
        lib.csgn_circuit_destroy(c)


@pytest.mark.parametrize("capacity_factor", [1, 40])
def test_mul_ragged_async_offsets_that_do_not_start_at_zero(hip, oracle, capacity_factor):
    """offset arrays that are a SUB-RANGE of a larger CSR (first entries 5 and 7, not 0) -- csgn_mul_ragged_async
    on 3 000 fresh 1 x 1 pairs takes the all-1x1 stream (inside the CSR kernel with a tight capacity bound, as the gated
    stream kernel in front of the wave-cooperative one with a loose bound) and must read the operands from where the
    offsets say; the same for a mixed batch through the CSR / wave-cooperative kernels.  Every pair against the oracle."""
    n, dl = 1247, 20
    rng = np.random.default_rng(12)
    for shapes in ([(1, 1)] * 3000, [(int(a), int(b)) for a, b in rng.integers(1, 6, size=(500, 2))]):
        t1s, t2s = [a for a, _ in shapes], [b for _, b in shapes]
        offL, offR = csr(t1s) + np.uint64(5), csr(t2s) + np.uint64(7)
        L, R = hip.synth_fill(61, n, 0, int(offL[-1]) * dl), hip.synth_fill(62, n, 0, int(offR[-1]) * dl)
        total = int(np.sum(np.asarray(t1s) * np.asarray(t2s)))
        out, off_out, plan = hip.mul_ragged_async(n, L, hip.upload(offL), R, hip.upload(offR), total * capacity_factor)
        res = hip.mul_ragged_async_result(plan)
        assert res[0] == total and res[4] == 0
        out, oo = hip.download(out), hip.download(off_out)
        hl, hr = hip.download(L), hip.download(R)
        for b in range(len(shapes)):
            want, _ = oracle.mul(n, hl[int(offL[b]) * dl:int(offL[b + 1]) * dl], hr[int(offR[b]) * dl:int(offR[b + 1]) * dl])
            assert np.array_equal(out[int(oo[b]) * dl:int(oo[b + 1]) * dl], want), b


@pytest.mark.parametrize("n,d", [(1247, 2), (4096, 3), (130, 2)])
def test_decrypt_batches_of_every_kind_on_scratch_that_holds_garbage(hip, oracle, n, d):
    """Ragged batches with empty, short and long (> 4096 terms: queued for the chunk kernel) ciphertexts and uniform
    batches of 1 to 700 terms, on a scratch block pre-filled with random bytes and used three times over: the same bits
    every time, the oracle's on sampled ciphertexts.  (Written for round 5's attempt to fold the parity pass into the
    hit-bit launch -- tail workgroups waiting on counters in the scratch block; DESIGN section 8 has why it was not kept.)"""
    import torch
    from csgn_amd.capi import check
    lib = hip.lib
    dl = oracle.default_len(n)
    key = make_key(n, d, 13)
    dmask = hip.upload(hip.key_mask(n, key))
    rng = np.random.default_rng(n)
    cases = [("ragged", rng.integers(0, 12, size=5000)),
             ("ragged", np.concatenate([rng.integers(0, 4, size=700), [5000, 0, 4097, 4096, 1], rng.integers(0, 40, size=300)])),
             ("uniform", np.full(3000, 1)), ("uniform", np.full(777, 5)), ("uniform", np.full(9, 700)), ("ragged", np.zeros(40, dtype=np.int64))]
    for kind, counts in cases:
        counts = np.asarray(counts, dtype=np.int64)
        batch, total = counts.size, int(counts.sum())
        off_h = csr(counts.tolist())
        W = hip.synth_fill(90 + batch, n, 0, max(total, 1) * dl)
        off = hip.upload(off_h)
        nbytes = int(lib.csgn_decrypt_scratch_bytes(batch, total))
        scratch = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device=hip.device)
        res = []
        for _ in range(3):
            bits = torch.full((batch,), 7, dtype=torch.uint8, device=hip.device)
            if kind == "uniform":
                check(lib.csgn_decrypt_uniform(n, batch, int(counts[0]), W.data_ptr(), dmask.data_ptr(), bits.data_ptr(), scratch.data_ptr(), hip.stream))
            else:
                check(lib.csgn_decrypt_ragged(n, batch, total, W.data_ptr(), off.data_ptr(), dmask.data_ptr(), bits.data_ptr(), scratch.data_ptr(), hip.stream))
            res.append(hip.download(bits))
        assert all(np.array_equal(r, res[0]) for r in res), (kind, batch)
        assert res[0].max() <= 1
        h = hip.download(W)
        for b in list(range(0, batch, max(1, batch // 25))) + [batch - 1]:
            v = h[int(off_h[b]) * dl:int(off_h[b + 1]) * dl]
            assert res[0][b] == (oracle.decrypt_canonical(n, key, v) if v.size else 0), (kind, b)


def test_add_ragged_with_bounds_on_the_term_counts(hip, oracle):
    """csgn_add_ragged_bounded: bounds met with equality send a CSR batch to the uniform kernel (50 000 sums of 1 + 1
    terms, 700 of 3 + 2) -- words and offsets equal csgn_add_ragged's and the oracle's; loose bounds change nothing; bounds
    too small for the total are refused."""
    from csgn_amd.capi import CsgnError
    n, dl = 1247, 20
    for batch, t1, t2 in ((50000, 1, 1), (700, 3, 2)):
        L, R = hip.synth_fill(90 + t1, n, 0, batch * t1 * dl), hip.synth_fill(91 + t2, n, 0, batch * t2 * dl)
        oL, oR = hip.upload(csr([t1] * batch)), hip.upload(csr([t2] * batch))
        ref, ref_off = hip.add_ragged(n, L, oL, R, oR, total_terms_out=batch * (t1 + t2))
        ref, ref_off = hip.download(ref), hip.download(ref_off)
        for b1, b2 in ((t1, t2), (t1 + 1, t2), (40, 50)):
            got, off = hip.add_ragged(n, L, oL, R, oR, total_terms_out=batch * (t1 + t2), max_t1=b1, max_t2=b2)
            assert np.array_equal(hip.download(got), ref) and np.array_equal(hip.download(off), ref_off), (batch, b1, b2)
        hl, hr = hip.download(L), hip.download(R)
        for b in (0, batch - 1):
            want, _ = oracle.add(hl[b * t1 * dl:(b + 1) * t1 * dl], hr[b * t2 * dl:(b + 1) * t2 * dl])
            assert np.array_equal(ref[b * (t1 + t2) * dl:(b + 1) * (t1 + t2) * dl], want)
        with pytest.raises(CsgnError):
            hip.add_ragged(n, L, oL, R, oR, total_terms_out=batch * (t1 + t2), max_t1=t1, max_t2=t2 - 1)


def test_decrypt_ragged_with_a_bound_on_the_term_counts(hip, oracle):
    """csgn_decrypt_ragged_bounded: a CSR batch whose bound is met with equality (batch * max_terms == total_terms)
    runs the uniform kernels -- 70 000 single-term ciphertexts and 900 three-term ones give the bits of
    csgn_decrypt_uniform, csgn_decrypt_ragged and the oracle; a bound that is not tight, and one above the
    long-ciphertext threshold, change nothing; a bound too small for total_terms is refused."""
    from csgn_amd.capi import CsgnError
    n, dl = 1247, 20
    key = make_key(n, 2, 9)                                             # short key: one synthetic term in four hits
    dmask = hip.upload(hip.key_mask(n, key))
    for batch, t in ((70000, 1), (900, 3)):
        W = hip.synth_fill(77 + t, n, 0, batch * t * dl)
        off = hip.upload(csr([t] * batch))
        want = hip.download(hip.decrypt_uniform(n, batch, t, W, dmask))
        assert 0 < want.sum() < batch
        for bound in (t, 0, t + 5, 5000):
            got = hip.download(hip.decrypt_ragged(n, W, off, dmask, total_terms=batch * t, max_terms=bound))
            assert np.array_equal(got, want), (batch, t, bound)
        h = hip.download(W)
        for b in (0, batch // 2, batch - 1):
            assert want[b] == oracle.decrypt_canonical(n, key, h[b * t * dl:(b + 1) * t * dl])
    # ragged for real: the bound only drops the long-ciphertext launch
    counts = np.random.default_rng(4).integers(0, 9, size=3000)
    off_h = csr(counts.tolist())
    W = hip.synth_fill(80, n, 0, int(off_h[-1]) * dl)
    off = hip.upload(off_h)
    a = hip.download(hip.decrypt_ragged(n, W, off, dmask, total_terms=int(off_h[-1])))
    b = hip.download(hip.decrypt_ragged(n, W, off, dmask, total_terms=int(off_h[-1]), max_terms=8))
    assert np.array_equal(a, b) and a.any()
    h = hip.download(W)
    for i in (0, 1, 1500, 2999):
        v = h[int(off_h[i]) * dl:int(off_h[i + 1]) * dl]
        assert a[i] == (oracle.decrypt_canonical(n, key, v) if v.size else 0)
    with pytest.raises(CsgnError):
        hip.decrypt_ragged(n, W, off, dmask, total_terms=int(off_h[-1]), max_terms=3)   # 3000 * 3 < total


def test_ragged_mul_sliced_with_operand_touch(hip, oracle, knobs):
    """A ragged product above 1 GiB (7 000 pairs of 20..44 x 20..44 terms, N=1247) goes in slices, each
    preceded by the device-side operand touch; identical to the unsliced run, sampled pairs equal
    the oracle, including pairs that straddle a slice boundary."""
    import torch
    n, dl = 1247, 20
    rng = np.random.default_rng(8)
    batch = 7000
    t1s, t2s = rng.integers(20, 45, size=batch), rng.integers(20, 45, size=batch)
    offL, offR = csr(t1s.tolist()), csr(t2s.tolist())
    total = int(np.sum(t1s * t2s))
    assert total * 10 > (1 << 26)                               # more units than one slice
    L = hip.synth_fill(51, n, 0, int(offL[-1]) * dl)
    R = hip.synth_fill(52, n, 0, int(offR[-1]) * dl)
    dOL, dOR = hip.upload(offL), hip.upload(offR)
    knobs.set("CSGN_RAGGED_FLAT", "1")
    knobs.set("CSGN_RAGGED_TOUCH", "0")
    ref, ref_off = hip.mul_ragged(n, L, dOL, R, dOR)
    ref = ref.clone()
    knobs.set("CSGN_RAGGED_TOUCH", "1")                         # ... sliced with the touch pass
    out, off = hip.mul_ragged(n, L, dOL, R, dOR)
    assert torch.equal(out, ref) and torch.equal(off, ref_off)
    # stream order: operands written on the caller's stream right before the call are what the product sees,
    # and overwriting them right after it does not reach back into it
    L2, R2 = torch.zeros_like(L), torch.zeros_like(R)
    for _ in range(3):
        L2.copy_(L); R2.copy_(R)
        out, off = hip.mul_ragged(n, L2, dOL, R2, dOR)
        L2.zero_(); R2.zero_()
        assert torch.equal(out, ref)
    del L2, R2
    for m, c in ((1, 8), (2, 2), (4, 4), (4, 8), (4, 16)):      # chunks per turn / per workgroup
        knobs.set("ragged_m", m)
        knobs.set("ragged_c", c)
        out, off = hip.mul_ragged(n, L, dOL, R, dOR)
        assert torch.equal(out, ref) and torch.equal(off, ref_off), (m, c)
    mo = hip.download(off)
    assert np.array_equal(mo, csr((t1s * t2s).tolist()))
    cut_term = (1 << 26) // 10                                  # first term of the second slice
    straddler = int(np.searchsorted(mo, cut_term, side="right") - 1)
    hl, hr = hip.download(L), hip.download(R)
    for b in sorted({0, 1, batch - 1, straddler - 1, straddler, straddler + 1} | set(rng.integers(0, batch, 40).tolist())):
        want, _ = oracle.mul(n, hl[int(offL[b]) * dl:int(offL[b + 1]) * dl], hr[int(offR[b]) * dl:int(offR[b + 1]) * dl])
        got = hip.download(out[int(mo[b]) * dl:int(mo[b + 1]) * dl])
        assert np.array_equal(got, want), b


def test_ragged_mul_slices_shrink_when_operands_are_heavy(hip, oracle, knobs):
    """A ragged product above 1 GiB whose operands are a large share of it (27 000 pairs of 10..22 x 10..22 terms:
    ~138 MB of operands for 1.1 GB of products): the plan's operand totals make csgn_mul_ragged cut the output in
    512 MiB slices (so that every slice's operands can be touched) instead of 1 GiB ones.  Same words as the
    unsliced run (touch off), sampled pairs equal the oracle, including pairs at the 512 MiB slice boundaries."""
    import torch
    n, dl = 1247, 20
    rng = np.random.default_rng(18)
    batch = 27000
    t1s, t2s = rng.integers(10, 23, size=batch), rng.integers(10, 23, size=batch)
    offL, offR = csr(t1s.tolist()), csr(t2s.tolist())
    total = int(np.sum(t1s * t2s))
    assert total * 10 > (1 << 26)                               # more than 1 GiB of 16-byte units
    assert int(offL[-1] + offR[-1]) * 10 * (1 << 26) > total * 10 * ((80 << 20) // 16)   # > 80 MB of operands per GiB
    L = hip.synth_fill(53, n, 0, int(offL[-1]) * dl)
    R = hip.synth_fill(54, n, 0, int(offR[-1]) * dl)
    dOL, dOR = hip.upload(offL), hip.upload(offR)
    knobs.set("CSGN_RAGGED_TOUCH", "0")                         # one launch, no slices
    ref, ref_off = hip.mul_ragged(n, L, dOL, R, dOR)
    ref = ref.clone()
    knobs.set("CSGN_RAGGED_TOUCH", "1")
    out, off = hip.mul_ragged(n, L, dOL, R, dOR)                # planned on this thread: slices follow the operand share
    assert torch.equal(out, ref) and torch.equal(off, ref_off)
    mo = hip.download(off)
    assert np.array_equal(mo, csr((t1s * t2s).tolist()))
    hl, hr = hip.download(L), hip.download(R)
    picks = {0, batch - 1}
    for cut_unit in (1 << 25, 1 << 26, 3 << 25):                # first terms of the 512 MiB slices
        if cut_unit // 10 >= total:
            continue
        b = min(batch - 1, int(np.searchsorted(mo, cut_unit // 10, side="right")) - 1)
        picks |= {max(0, b - 1), b, min(batch - 1, b + 1)}
    for b in sorted(picks):
        want, _ = oracle.mul(n, hl[int(offL[b]) * dl:int(offL[b + 1]) * dl], hr[int(offR[b]) * dl:int(offR[b + 1]) * dl])
        assert np.array_equal(hip.download(out[int(mo[b]) * dl:int(mo[b + 1]) * dl]), want), b


@pytest.mark.parametrize("n,mu,batch", [(1247, 1.6, 120000), (4096, 1.2, 50000)])
def test_ragged_long_tailed_small_pairs(hip, oracle, knobs, n, mu, batch):
    """A log-normal batch of small pairs with a long tail (mean ~8 x 8 terms, a few pairs of hundreds): unsliced,
    untouched, 16 chunks per workgroup by default.  Same words for other chunk / turn / touch settings; the largest
    pairs, the smallest and a sample equal the oracle."""
    import torch
    dl = oracle.default_len(n)
    rng = np.random.default_rng(int(mu * 10) + n)
    t1s = np.clip(rng.lognormal(mu, 1, batch), 1, 600).astype(int)
    t2s = np.clip(rng.lognormal(mu, 1, batch), 1, 600).astype(int)
    offL, offR = csr(t1s.tolist()), csr(t2s.tolist())
    total = int(np.sum(t1s * t2s))
    assert total >= 65536 and total // batch < 512 and int(t1s.max()) > 16
    L = hip.synth_fill(93, n, 0, int(offL[-1]) * dl)
    R = hip.synth_fill(94, n, 0, int(offR[-1]) * dl)
    dOL, dOR = hip.upload(offL), hip.upload(offR)
    out, off = hip.mul_ragged(n, L, dOL, R, dOR)
    out = out.clone()
    for c, m in ((8, 4), (2, 2), (1, 1)):
        knobs.set("ragged_c", c)
        knobs.set("ragged_m", m)
        ref, ref_off = hip.mul_ragged(n, L, dOL, R, dOR)
        assert torch.equal(out, ref) and torch.equal(off, ref_off), (c, m)
    mo = hip.download(off)
    hl, hr = hip.download(L), hip.download(R)
    order = np.argsort(t1s * t2s)
    picks = set(order[-6:].tolist()) | set(order[:3].tolist()) | {0, batch - 1} | set(rng.integers(0, batch, 40).tolist())
    for b in sorted(picks):
        want, _ = oracle.mul(n, hl[int(offL[b]) * dl:int(offL[b + 1]) * dl], hr[int(offR[b]) * dl:int(offR[b + 1]) * dl])
        assert np.array_equal(hip.download(out[int(mo[b]) * dl:int(mo[b + 1]) * dl]), want), b


@pytest.mark.parametrize("n", [63, 1247, 4096])
def test_ragged_cooperative_kernel_matches_the_csr_kernel(hip, oracle, knobs, n):
    """k_mul_ragged_coop (knob ragged_coop = 1): a wave walks the pairs of its stretch of the output together.  Same
    words as the CSR kernel for a batch with empty pairs and runs of them longer than the 63-pair window, 1 x 1 pairs,
    rows shorter and longer than a block, one pair far larger than a wave's stretch -- for stretches of 1, 3 and 64
    blocks per wave (every stretch boundary inside a pair, inside a row, between pairs) -- and through
    csgn_mul_ragged_async; a sample of pairs against the oracle."""
    import torch
    dl = oracle.default_len(n)
    rng = np.random.default_rng(n)
    t1s = np.concatenate([[1, 0, 0, 90, 1], np.zeros(200, int), [2, 3], np.ones(70, int), [0, 7, 300],
                          np.clip(rng.lognormal(1.4, 1, 3000), 1, 200).astype(int), [0, 0, 1]])
    t2s = np.concatenate([[1, 5, 0, 70, 1], np.zeros(200, int), [3, 2], np.ones(70, int), [9, 0, 250],
                          np.clip(rng.lognormal(1.4, 1, 3000), 1, 200).astype(int), [3, 0, 1]])
    batch = len(t1s)
    offL, offR = csr(t1s.tolist()), csr(t2s.tolist())
    total = int(np.sum(t1s * t2s))
    L = hip.synth_fill(95, n, 0, int(offL[-1]) * dl)
    R = hip.synth_fill(96, n, 0, int(offR[-1]) * dl)
    dOL, dOR = hip.upload(offL), hip.upload(offR)
    knobs.set("ragged_flat", 1)                     # everything through the ragged kernels (no per-pair uniform launches)
    knobs.set("ragged_coop", 0)
    ref, ref_off = hip.mul_ragged(n, L, dOL, R, dOR)
    ref = ref.clone()
    knobs.set("ragged_coop", 1)
    # the software-pipelined form (hand-counted waits) and the plain one, 2 and 4 blocks per group
    # ... with the in-kernel operand touch (the default, 128 KiB a side at most and window), capped at 1 KiB, and without
    for span, k, pipe, touch in [(1, 4, 1, 128), (3, 4, 1, 128), (0, 4, 1, 128), (1, 2, 1, 128), (3, 2, 1, 1), (0, 2, 1, 128),
                                 (2, 4, 1, 1), (5, 2, 1, 128), (7, 4, 1, 128), (1, 4, 0, 128), (3, 2, 0, 128), (0, 4, 0, 1),
                                 (0, 4, 1, 0), (3, 4, 1, 0), (1, 2, 0, 0)]:
        knobs.set("ragged_coop_span", span)
        knobs.set("ragged_coop_k", k)
        knobs.set("ragged_coop_pipe", pipe)
        knobs.set("ragged_coop_touch", touch)
        got, off = hip.mul_ragged(n, L, dOL, R, dOR)
        assert torch.equal(off, ref_off)
        assert torch.equal(got, ref), (span, k, pipe, touch)
        guard = hip.empty_words((total + 7) * dl)
        guard.fill_(0x5A5A5A5A)
        out, off, plan = hip.mul_ragged_async(n, L, dOL, R, dOR, total + 7, out=guard)
        assert hip.mul_ragged_async_result(plan)[0] == total
        assert torch.equal(out[:total * dl], ref[:total * dl]), (span, k, pipe)
        assert bool((out[total * dl:] == 0x5A5A5A5A).all())        # nothing past the real end
        if span == 3:                                              # a bound that is too small: the gate is 0, nothing is written
            guard.fill_(0x5A5A5A5A)
            out, off, plan = hip.mul_ragged_async(n, L, dOL, R, dOR, total - 1, out=guard)
            assert hip.mul_ragged_async_result(plan)[4] == 1
            assert bool((guard == 0x5A5A5A5A).all()), (span, k, pipe)
    mo = hip.download(ref_off)
    hl, hr = hip.download(L), hip.download(R)
    for b in [0, 3, 207, 208, 279, 280, 281, batch - 1] + rng.integers(282, batch - 3, 12).tolist():
        if t1s[b] and t2s[b]:
            want, _ = oracle.mul(n, hl[int(offL[b]) * dl:int(offL[b + 1]) * dl], hr[int(offR[b]) * dl:int(offR[b + 1]) * dl])
            assert np.array_equal(hip.download(got[int(mo[b]) * dl:int(mo[b + 1]) * dl]), want), b


@pytest.mark.parametrize("n", [1247, 4096])
def test_ragged_size_classes_match_the_csr_kernel(hip, oracle, knobs, n):
    """Size classes (round 4; measured slower than the CSR kernel and therefore off unless knob ragged_classes = 1):
    the plan lists the small pairs (t1 <= 64, t2 <= 128) by class, the multiply gives every class one LDS-tiled launch
    shaped for it and the CSR kernel skips what they wrote.  A batch that visits every
    class boundary (1, 8, 9, 16, 17, 32, 33, 64, 65 x 1, 2, 3, 4, 5, ... 128, 129 terms), empty pairs, runs of tiny
    pairs and pairs with one long side: on (knob 1) and off (the default) give the same words;
    samples of every kind equal the oracle.  A batch with small pairs ONLY never launches the CSR kernel."""
    import torch
    dl = oracle.default_len(n)
    rng = np.random.default_rng(n)
    edge1 = [0, 1, 7, 8, 9, 16, 17, 32, 33, 64, 65, 100]
    edge2 = [0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 200]
    pairs = [(a, b) for a in edge1 for b in edge2] * 2
    pairs += [(int(a), int(b)) for a, b in zip(np.clip(rng.lognormal(2, 1, 3000), 1, 300).astype(int),
                                                np.clip(rng.lognormal(2, 1, 3000), 1, 300).astype(int))]
    pairs += [(1, 1)] * 700 + [(300, 2), (2, 300), (0, 5), (70, 70)]
    order = rng.permutation(len(pairs))
    t1s = np.array([pairs[i][0] for i in order]); t2s = np.array([pairs[i][1] for i in order])
    offL, offR = csr(t1s.tolist()), csr(t2s.tolist())
    L = hip.synth_fill(95, n, 0, int(offL[-1]) * dl)
    R = hip.synth_fill(96, n, 0, int(offR[-1]) * dl)
    dOL, dOR = hip.upload(offL), hip.upload(offR)
    knobs.set("ragged_classes", 0)
    ref, ref_off = hip.mul_ragged(n, L, dOL, R, dOR)
    ref = ref.clone()
    knobs.set("ragged_classes", 1)                          # the plan builds the lists, the multiply uses them
    out, off = hip.mul_ragged(n, L, dOL, R, dOR)
    assert torch.equal(off, ref_off) and torch.equal(out, ref)
    mo = hip.download(ref_off)
    hl, hr = hip.download(L), hip.download(R)
    picks = set(rng.integers(0, len(pairs), 60).tolist()) | {0, len(pairs) - 1}
    for b in sorted(picks):
        if t1s[b] and t2s[b]:
            want, _ = oracle.mul(n, hl[int(offL[b]) * dl:int(offL[b + 1]) * dl], hr[int(offR[b]) * dl:int(offR[b + 1]) * dl])
            assert np.array_equal(hip.download(ref[int(mo[b]) * dl:int(mo[b + 1]) * dl]), want), b
    # small pairs only: class launches alone
    small = (t1s <= 64) & (t2s <= 128)
    t1b, t2b = t1s[small], t2s[small]
    oL, oR = csr(t1b.tolist()), csr(t2b.tolist())
    Lb = hip.synth_fill(97, n, 0, int(oL[-1]) * dl)
    Rb = hip.synth_fill(98, n, 0, int(oR[-1]) * dl)
    knobs.set("ragged_classes", 0)
    ref2, ref2_off = hip.mul_ragged(n, Lb, hip.upload(oL), Rb, hip.upload(oR))
    ref2 = ref2.clone()
    knobs.set("ragged_classes", 1)
    out2, off2 = hip.mul_ragged(n, Lb, hip.upload(oL), Rb, hip.upload(oR))
    assert torch.equal(out2, ref2) and torch.equal(off2, ref2_off)


@pytest.mark.parametrize("n,lo,hi,batch", [(1247, 0, 6, 300000), (1247, 4, 13, 60000), (4096, 1, 9, 40000), (128, 0, 6, 200000)])
def test_ragged_batches_of_small_pairs(hip, oracle, knobs, n, lo, hi, batch):
    """Batches of SMALL pairs (0..5, 4..12, 1..8 terms; also N=128 with its one-unit terms): by default the tiled kernel
    with one narrow workgroup per pair (no lookup); with knob ragged_flat = 1 the CSR kernel, whose every turn spans
    dozens of pairs there and takes the offset-window path.  Same words either way and for every chunk / turn
    setting, sampled pairs equal the oracle (incl. empty pairs, the first and the last pair)."""
    import torch
    dl = oracle.default_len(n)
    rng = np.random.default_rng(n + hi)
    t1s, t2s = rng.integers(lo, hi, size=batch), rng.integers(lo, hi, size=batch)
    offL, offR = csr(t1s.tolist()), csr(t2s.tolist())
    L = hip.synth_fill(91, n, 0, int(offL[-1]) * dl)
    R = hip.synth_fill(92, n, 0, int(offR[-1]) * dl)
    dOL, dOR = hip.upload(offL), hip.upload(offR)
    out, off = hip.mul_ragged(n, L, dOL, R, dOR)                 # default: one narrow workgroup per pair (tiled kernel)
    out = out.clone()
    knobs.set("ragged_flat", 1)                                 # the CSR kernel, every chunk / turn setting
    for m, c in ((4, 0), (1, 8), (2, 2), (4, 16), (1, 1)):
        knobs.set("ragged_m", m)
        knobs.set("ragged_c", c)
        other, other_off = hip.mul_ragged(n, L, dOL, R, dOR)
        assert torch.equal(out, other) and torch.equal(off, other_off), (m, c)
    mo = hip.download(off)
    assert np.array_equal(mo, csr((t1s * t2s).tolist()))
    hl, hr = hip.download(L), hip.download(R)
    picks = {0, 1, batch // 3, batch // 2, batch - 2, batch - 1} | set(rng.integers(0, batch, 60).tolist())
    for b in sorted(picks):
        if t1s[b] and t2s[b]:
            want, _ = oracle.mul(n, hl[int(offL[b]) * dl:int(offL[b + 1]) * dl], hr[int(offR[b]) * dl:int(offR[b + 1]) * dl])
            assert np.array_equal(hip.download(out[int(mo[b]) * dl:int(mo[b + 1]) * dl]), want), b


def test_ragged_huge_pairs_take_uniform_launches(hip, oracle, knobs):
    """csgn_mul_planned by a csgn_mul_plan object: pairs of 24 MB of output and more (written down by
    the plan) get uniform launches of their own, the CSR kernel runs on the stretches between them.  Two
    huge pairs (400x400 and 512x330 terms, N=1247), one at the very start, among 3000 small and empty
    ones, and a third at the very end; identical to the CSR kernel alone (knob ragged_flat = 1), huge and
    neighbouring pairs equal the oracle.  The plan-less csgn_mul_ragged (a pure function of its arguments)
    must give the same words through the CSR kernel."""
    import torch
    n, dl = 1247, 20
    rng = np.random.default_rng(77)
    batch = 3003
    t1s, t2s = rng.integers(0, 6, size=batch), rng.integers(0, 6, size=batch)
    huge = {0: (400, 400), 1500: (512, 330), batch - 1: (300, 600)}
    for b, (a, c) in huge.items():
        t1s[b], t2s[b] = a, c
    offL, offR = csr(t1s.tolist()), csr(t2s.tolist())
    L = hip.synth_fill(61, n, 0, int(offL[-1]) * dl)
    R = hip.synth_fill(62, n, 0, int(offR[-1]) * dl)
    dOL, dOR = hip.upload(offL), hip.upload(offR)
    out, off = hip.mul_ragged(n, L, dOL, R, dOR)                 # plan + multiply: the huge pairs go uniform
    out = out.clone()
    knobs.set("ragged_flat", 1)
    ref, ref_off = hip.mul_ragged(n, L, dOL, R, dOR)             # everything through the CSR kernel
    assert torch.equal(out, ref) and torch.equal(off, ref_off)
    knobs.unset("ragged_flat")
    # the plan-less entry: same words
    from csgn_amd.capi import check
    mo = hip.download(off)
    dOL2, dOR2, off2 = dOL.clone(), dOR.clone(), off.clone()
    out2 = hip.empty_words(out.numel())
    check(hip.lib.csgn_mul_ragged(n, batch, L.data_ptr(), dOL2.data_ptr(), R.data_ptr(), dOR2.data_ptr(), out2.data_ptr(),
                                  off2.data_ptr(), int(t1s.max()), int(t2s.max()), int(mo[-1]), hip.stream))
    assert torch.equal(out2, ref)
    hl, hr = hip.download(L), hip.download(R)
    for b in sorted(set(huge) | {1, 2, 1499, 1501, batch - 2}):
        if t1s[b] and t2s[b]:
            want, _ = oracle.mul(n, hl[int(offL[b]) * dl:int(offL[b + 1]) * dl], hr[int(offR[b]) * dl:int(offR[b + 1]) * dl])
            assert np.array_equal(hip.download(out[int(mo[b]) * dl:int(mo[b + 1]) * dl]), want), b


def test_stale_plan_is_detected_not_multiplied(hip, oracle):
    from csgn_amd.capi import check
    """ADVICE r3 / VERDICT r3 #9: a plan remembers host copies of its huge pairs' offsets.  A caller that rewrites
    the offset arrays IN PLACE with the same totals (pairs shuffled) and multiplies by the old plan used to get
    silently wrong words; csgn_mul_planned now checks the arrays against the plan's checksum whenever it is
    about to use such records and returns CSGN_ERR_INVALID.  Planning again gives the right products."""
    import torch
    from csgn_amd import capi
    n, dl = 1247, 20
    t1s = np.array([400, 3, 2, 512, 1, 4], dtype=np.int64)
    t2s = np.array([400, 2, 5, 330, 1, 3], dtype=np.int64)
    offL, offR = csr(t1s.tolist()), csr(t2s.tolist())
    L = hip.synth_fill(71, n, 0, int(offL[-1]) * dl)
    R = hip.synth_fill(72, n, 0, int(offR[-1]) * dl)
    dOL, dOR = hip.upload(offL), hip.upload(offR)
    off_out = hip.empty_words(len(t1s) + 1)
    plan = (C.c_uint64 * 4)()
    handle = hip.mul_plan()
    try:
        check(hip.lib.csgn_mul_plan_ragged(handle, len(t1s), dOL.data_ptr(), dOR.data_ptr(), off_out.data_ptr(),
                                           C.byref(plan), hip.stream))
        total = int(plan[0])
        out = hip.empty_words(total * dl)
        assert hip.lib.csgn_mul_plan_validate(handle, hip.stream) == 0
        check(hip.lib.csgn_mul_planned(handle, n, L.data_ptr(), R.data_ptr(), out.data_ptr(), hip.stream))
        first = hip.download(out)
        # shuffle the pairs in place: same multiset of shapes, same totals, same array addresses
        perm = [3, 1, 2, 0, 4, 5]
        dOL.copy_(hip.upload(csr(t1s[perm].tolist())))
        dOR.copy_(hip.upload(csr(t2s[perm].tolist())))
        torch.cuda.synchronize()
        assert hip.lib.csgn_mul_plan_validate(handle, hip.stream) == capi.CSGN_ERR_INVALID
        assert hip.lib.csgn_mul_planned(handle, n, L.data_ptr(), R.data_ptr(), out.data_ptr(), hip.stream) == capi.CSGN_ERR_INVALID
        assert b"changed since" in hip.lib.csgn_last_error()
        # plan again: right words for the shuffled batch
        check(hip.lib.csgn_mul_plan_ragged(handle, len(t1s), dOL.data_ptr(), dOR.data_ptr(), off_out.data_ptr(),
                                           C.byref(plan), hip.stream))
        assert int(plan[0]) == total
        check(hip.lib.csgn_mul_planned(handle, n, L.data_ptr(), R.data_ptr(), out.data_ptr(), hip.stream))
        got, mo = hip.download(out), hip.download(off_out)
        hl, hr = hip.download(L), hip.download(R)
        ol, orr = csr(t1s[perm].tolist()), csr(t2s[perm].tolist())
        for b in range(len(perm)):
            want, _ = oracle.mul(n, hl[int(ol[b]) * dl:int(ol[b + 1]) * dl], hr[int(orr[b]) * dl:int(orr[b + 1]) * dl])
            assert np.array_equal(got[int(mo[b]) * dl:int(mo[b + 1]) * dl], want), b
        assert not np.array_equal(got, first)
        # trust: the check is skipped (the caller's promise); a plan that was never made is refused
        check(hip.lib.csgn_mul_plan_trust(handle, 1))
        check(hip.lib.csgn_mul_planned(handle, n, L.data_ptr(), R.data_ptr(), out.data_ptr(), hip.stream))
        fresh = hip.mul_plan()
        assert hip.lib.csgn_mul_planned(fresh, n, L.data_ptr(), R.data_ptr(), out.data_ptr(), hip.stream) == capi.CSGN_ERR_INVALID
        hip.lib.csgn_mul_plan_destroy(fresh)
    finally:
        hip.lib.csgn_mul_plan_destroy(handle)


@pytest.mark.parametrize("n", [1247, 129])
def test_mul_ragged_async_matches_the_planned_multiply(hip, oracle, n):
    """csgn_mul_ragged_async: plan kernels + multiply enqueued back to back, nothing read back, the launch sized
    by the caller's bound.  Same words and offsets as plan + multiply for skewed batches, empty pairs, a batch of
    1x1 pairs (the device picks the AND stream) and a bound far above the real size; a bound that is too small
    writes nothing and says so."""
    import torch
    dl = oracle.default_len(n)
    rng = np.random.default_rng(n)
    cases = [
        (rng.integers(0, 9, size=700), rng.integers(0, 9, size=700)),
        (np.array([300] + [1] * 500 + [0, 0, 7]), np.array([250] + [1] * 500 + [3, 0, 2])),
        (np.ones(5000, dtype=np.int64), np.ones(5000, dtype=np.int64)),
        (np.array([0, 0, 0]), np.array([4, 0, 1])),
    ]
    for k, (t1s, t2s) in enumerate(cases):
        offL, offR = csr(t1s.tolist()), csr(t2s.tolist())
        L = hip.synth_fill(81 + k, n, 0, max(1, int(offL[-1])) * dl)
        R = hip.synth_fill(91 + k, n, 0, max(1, int(offR[-1])) * dl)
        dOL, dOR = hip.upload(offL), hip.upload(offR)
        ref, ref_off = hip.mul_ragged(n, L, dOL, R, dOR)
        total = int((t1s * t2s).sum())
        for cap in (total, total + 1, 3 * total + 1000):
            out, off, plan = hip.mul_ragged_async(n, L, dOL, R, dOR, cap)
            res = hip.mul_ragged_async_result(plan)
            assert res[0] == total and res[4] == 0, (k, cap, res)
            assert res[1] == int(t1s.max()) and res[2] == int(t2s.max())
            assert torch.equal(off, ref_off)
            assert torch.equal(out[:total * dl], ref[:total * dl]), (k, cap)
        if total > 1:
            guard = hip.empty_words(total * dl)
            guard.fill_(0x5A5A5A5A)
            out, off, plan = hip.mul_ragged_async(n, L, dOL, R, dOR, total - 1, out=guard)
            res = hip.mul_ragged_async_result(plan)
            assert res[0] == total and res[4] == 1
            assert bool((guard == 0x5A5A5A5A).all())          # nothing was written


@pytest.mark.parametrize("n", [129, 1247])
def test_mul_ragged_async_huge_pairs_ride_in_the_csr_launch(hip, oracle, n):
    """csgn_mul_ragged_async with pairs of 65 536 product terms and more: the plan kernel records up to 32 of them on the
    device, the first workgroups of the CSR kernel's launch multiply the recorded ones tile by tile and the CSR workgroups
    skip what lies inside them; pairs beyond the 32 records stay with the CSR kernel.  36 such pairs between singles,
    empties and a run of small pairs, one of them last; exact, loose and insufficient capacity.  Same words and offsets
    as plan + multiply."""
    import torch
    dl = oracle.default_len(n)
    rng = np.random.default_rng(n + 7)
    t1s, t2s = [], []
    for k in range(36):
        t1s += [260 + k % 3, 1, 0, 2]
        t2s += [256 - k % 2, 1, 5, 3]
        if k % 5 == 0:
            t1s += list(rng.integers(0, 9, size=40))
            t2s += list(rng.integers(0, 9, size=40))
    t1s += [300]
    t2s += [250]
    t1s, t2s = np.array(t1s, dtype=np.int64), np.array(t2s, dtype=np.int64)
    assert int((t1s * t2s >= 65536).sum()) == 37
    offL, offR = csr(t1s.tolist()), csr(t2s.tolist())
    L = hip.synth_fill(101, n, 0, int(offL[-1]) * dl)
    R = hip.synth_fill(102, n, 0, int(offR[-1]) * dl)
    dOL, dOR = hip.upload(offL), hip.upload(offR)
    ref, ref_off = hip.mul_ragged(n, L, dOL, R, dOR)
    total = int((t1s * t2s).sum())
    for cap in (total, total + 12345):
        out, off, plan = hip.mul_ragged_async(n, L, dOL, R, dOR, cap)
        res = hip.mul_ragged_async_result(plan)
        assert res[0] == total and res[4] == 0, (cap, res)
        assert torch.equal(off, ref_off)
        assert torch.equal(out[:total * dl], ref[:total * dl]), cap
    guard = hip.empty_words(total * dl)
    guard.fill_(0x5A5A5A5A)
    out, off, plan = hip.mul_ragged_async(n, L, dOL, R, dOR, total - 1, out=guard)
    assert hip.mul_ragged_async_result(plan)[4] == 1 and bool((guard == 0x5A5A5A5A).all())
    # spot check against the oracle: the last pair (a recorded one or not, it is the 37th)
    b = len(t1s) - 1
    hl, hr = hip.download(L), hip.download(R)
    want, _ = oracle.mul(n, hl[int(offL[b]) * dl:int(offL[b + 1]) * dl], hr[int(offR[b]) * dl:int(offR[b + 1]) * dl])
    ro = hip.download(ref_off)
    assert np.array_equal(hip.download(ref[int(ro[b]) * dl:int(ro[b + 1]) * dl]), want)


def test_ragged_forms_fuzz(hip, oracle, knobs):
    """36 random CSR batches (empty operands, runs of empty pairs -- some longer than the 256-pair
    offset window of the flat kernels -- one large pair among small ones, all-singles and all-equal
    batches that the default dispatch hands to the uniform kernels) through the flat ragged multiply
    and add with 1 / 2 / 8 / 16 chunks per workgroup, 1 / 2 / 4 chunks per turn and operand prefetch
    off / 32 / 5000 pairs ahead, and through the default dispatch: identical words; every fifth batch
    is compared pair by pair with the oracle."""
    import torch
    rng = np.random.default_rng(4242 + FUZZ_SEED)
    for it in range(36):
        n = int(rng.choice([65, 1247, 1300, 4096]))
        dl = oracle.default_len(n)
        batch = int(rng.choice([1, 7, 300, 2500, 9000]))
        t1s = rng.integers(0, 9, size=batch)
        t2s = rng.integers(0, 9, size=batch)
        if it % 3 == 0:
            t1s[rng.integers(0, batch)], t2s[rng.integers(0, batch)] = 200, 150
        if it % 4 == 0 and batch > 600:
            t1s[100:600] = 0                                   # a run of empty pairs longer than a workgroup's offset window
        if it % 6 == 1:
            t1s[:] = 1                                         # all singles: 1x1 products, 1+1 sums
            t2s[:] = 1
        if it % 6 == 4:
            t1s[:] = int(rng.integers(1, 6))                   # all pairs of one shape: a uniform batch in CSR clothes
            t2s[:] = int(rng.integers(1, 6))
        if it % 9 == 5 and batch > 2000:
            t1s[:] = (rng.integers(0, 40, size=batch) == 0)    # singles thinly spread among empty pairs
            t2s[:] = 1
        if not int(np.sum(t1s * t2s)):
            t1s[0] = t2s[0] = 2
        offL, offR = csr(t1s.tolist()), csr(t2s.tolist())
        L = hip.synth_fill(3 * it, n, 0, max(1, int(offL[-1])) * dl)
        R = hip.synth_fill(3 * it + 1, n, 0, max(1, int(offR[-1])) * dl)
        dOL, dOR = hip.upload(offL), hip.upload(offR)
        tot_add = int(offL[-1] + offR[-1])
        ref_mul = ref_add = None
        for env in ({}, {"CSGN_RAGGED_FLAT": "1", "CSGN_RAGGED_C": "1", "CSGN_RAGGED_PF": "0"},
                    {"CSGN_RAGGED_FLAT": "1", "CSGN_RAGGED_C": "8", "CSGN_RAGGED_PF": "32"},
                    {"CSGN_RAGGED_FLAT": "1", "CSGN_RAGGED_C": "16", "CSGN_RAGGED_PF": "5000"},
                    {"CSGN_RAGGED_FLAT": "1"},
                    {"CSGN_RAGGED_FLAT": "1", "CSGN_RAGGED_M": "1", "CSGN_RAGGED_C": "8"},
                    {"CSGN_RAGGED_FLAT": "1", "CSGN_RAGGED_M": "2", "CSGN_RAGGED_C": "2"},
                    {"CSGN_RAGGED_FLAT": "1", "CSGN_RAGGED_M": "4", "CSGN_RAGGED_C": "16"}):
            for k in ("CSGN_RAGGED_FLAT", "CSGN_RAGGED_C", "CSGN_RAGGED_PF", "CSGN_RAGGED_M"):
                knobs.unset(k)
            for k, v in env.items():
                knobs.set(k, v)
            m, moff = hip.mul_ragged(n, L, dOL, R, dOR)
            a, aoff = hip.add_ragged(n, L, dOL, R, dOR, total_terms_out=tot_add)
            if ref_mul is None:
                ref_mul, ref_moff, ref_add, ref_aoff = m.clone(), moff.clone(), a.clone(), aoff.clone()
            else:
                assert torch.equal(m, ref_mul) and torch.equal(moff, ref_moff), (it, env)
                assert torch.equal(a, ref_add) and torch.equal(aoff, ref_aoff), (it, env)
        assert np.array_equal(hip.download(ref_moff), csr((t1s * t2s).tolist()))
        if it % 5 == 0:
            hl, hr, hm, ha = (hip.download(x) for x in (L, R, ref_mul, ref_add))
            mo, ao = hip.download(ref_moff), hip.download(ref_aoff)
            for b in range(0, batch, max(1, batch // 40)):
                lh = hl[int(offL[b]) * dl:int(offL[b + 1]) * dl]
                rh = hr[int(offR[b]) * dl:int(offR[b + 1]) * dl]
                if t1s[b] and t2s[b]:
                    want, _ = oracle.mul(n, lh, rh)
                    assert np.array_equal(hm[int(mo[b]) * dl:int(mo[b + 1]) * dl], want), (it, b)
                want_s, _ = oracle.add(lh, rh)
                assert np.array_equal(ha[int(ao[b]) * dl:int(ao[b + 1]) * dl], want_s), (it, b)


@pytest.mark.parametrize("batch", [1, 2, 1023, 4095, 4096, 4097, 5000, 200000, 1300000])
@pytest.mark.parametrize("misaligned", [False, True])
def test_mul_ragged_plan_offsets(hip, batch, misaligned):
    """The plan kernel (4096-pair chunks chained by a look-back; tickets once the chunks outnumber the CUs: the
    1.3 M case) against numpy for batch sizes around the chunk boundaries, with zeros mixed in; 16-byte aligned
    arrays (the vector path) and arrays 8 bytes off."""
    import ctypes as C
    rng = np.random.default_rng(batch)
    t1 = rng.integers(0, 7, size=batch).astype(np.uint64)
    t2 = rng.integers(0, 5, size=batch).astype(np.uint64)
    offL, offR = csr(t1), csr(t2)
    skew = 1 if misaligned else 0
    off_out = hip.empty_words(batch + 1 + skew)[skew:]
    plan = (C.c_uint64 * 4)()
    from csgn_amd.capi import check
    d_off_l = hip.upload(np.concatenate([np.zeros(skew, np.uint64), offL]))[skew:]    # keep the tensors alive across the call
    d_off_r = hip.upload(np.concatenate([np.zeros(skew, np.uint64), offR]))[skew:]
    assert (d_off_l.data_ptr() % 16 == 8) == misaligned
    check(hip.lib.csgn_mul_ragged_plan(batch, d_off_l.data_ptr(), d_off_r.data_ptr(),
                                       off_out.data_ptr(), C.byref(plan), hip.stream))
    want = csr(t1 * t2)
    assert np.array_equal(hip.download(off_out), want)
    assert int(plan[0]) == int(want[-1])
    assert (int(plan[1]), int(plan[2]), int(plan[3])) == (int(t1.max()), int(t2.max()), int((t1 * t2).max()))


@pytest.mark.parametrize("batch", [4096, 300000, 1200000])
@pytest.mark.parametrize("odd_at", [None, 0, -1, 70000])
def test_mul_ragged_async_gate_across_chunks(hip, oracle, batch, odd_at):
    """The all-1x1 decision of csgn_mul_ragged_async rides the plan kernel's look-back chain: a single pair that is
    not 1 x 1 -- in the first chunk, the last, or in between -- must reach the last chunk across every window of the
    chain (and across tickets at 1.2 M pairs), or the AND stream would run on a batch it is wrong for."""
    import torch
    n = 64
    dl = oracle.default_len(n)
    t1s = np.ones(batch, dtype=np.int64)
    t2s = np.ones(batch, dtype=np.int64)
    if odd_at is not None:
        at = odd_at if odd_at >= 0 else batch - 1
        if at >= batch:
            pytest.skip("pair outside the batch")
        t1s[at], t2s[at] = 2, 0 if odd_at == 70000 else 1        # 2 x 1 (one more term) or 2 x 0 (one fewer)
    offL, offR = csr(t1s), csr(t2s)
    L = hip.synth_fill(5, n, 0, int(offL[-1]) * dl)
    R = hip.synth_fill(6, n, 0, max(1, int(offR[-1])) * dl)
    dOL, dOR = hip.upload(offL), hip.upload(offR)
    total = int((t1s * t2s).sum())
    out, off, plan = hip.mul_ragged_async(n, L, dOL, R, dOR, total + 3)
    res = hip.mul_ragged_async_result(plan)
    assert res[0] == total and res[4] == 0, res
    want_off = csr(t1s * t2s)
    assert np.array_equal(hip.download(off), want_off)
    # every product term against torch: term j of pair b = L term (offL[b] + j / t2) & R term (offR[b] + j % t2)
    pair = np.repeat(np.arange(batch), (t1s * t2s))
    j = np.arange(total) - want_off[:-1].astype(np.int64)[pair]
    li = offL[:-1].astype(np.int64)[pair] + j // np.maximum(t2s[pair], 1)
    ri = offR[:-1].astype(np.int64)[pair] + j % np.maximum(t2s[pair], 1)
    li_t = torch.from_numpy(li).to(hip.device)
    ri_t = torch.from_numpy(ri).to(hip.device)
    want = L.view(-1, dl)[li_t] & R.view(-1, dl)[ri_t]
    assert torch.equal(out[:total * dl].view(-1, dl), want)


def test_decrypt_ragged_skewed(hip, oracle):
    """Ragged decrypt where one ciphertext is far longer than the rest (lane-per-ciphertext pass
    for the short ones, wave-per-ciphertext pass for the long ones), with empty ones mixed in."""
    n, d = 1247, 16
    key = make_key(n, d, 77)
    dmask = hip.upload(hip.key_mask(n, key))
    # long ciphertexts are folded in 65 536-term chunks from a device-side work list: lengths around the
    # long/short threshold (4096) and around one and several chunks, at bit offsets that are not word-aligned
    for counts in ([3, 0, 100000, 1, 4096, 4097, 0, 0, 7, 70000, 2],
                   [5, 65536, 1, 65537, 0, 131072, 9, 131073, 65535, 3, 200001, 1]):
        parts = [planted(oracle, n, key, t, (t * 7 + i) % (t + 1), 300 + i) if t else np.zeros(0, np.uint64)
                 for i, t in enumerate(counts)]
        bits = hip.download(hip.decrypt_ragged(n, hip.upload(np.concatenate(parts)), hip.upload(csr(counts)), dmask))
        for i, t in enumerate(counts):
            want = oracle.decrypt_canonical(n, key, parts[i]) if t else 0
            assert bits[i] == want == (((t * 7 + i) % (t + 1)) % 2 if t else 0), (counts, i)
