"""Knobs of csgn_tuning.h that no other GPU test sets, each against the oracle: the tiled multiply's block order
(mul_xcd = 2) and block sizes (mul_bs), the persistent grid of the compaction's main kernel (compact_grid, compact_nt,
compact_stagger_us) and shared_gpu.  tests/test_tuning_ledger.py keeps the list of who sets which knob.
Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

from tests.model import hip  # noqa: F401
from tests.test_block_order_gpu import cdiv, units
from tests.test_gpu_parity import CONTEXTS, _check_compaction, _dup_ciphertext

pytestmark = pytest.mark.gpu

TILED_SHAPES = [(33, 65), (5, 300)]
TILED_BATCHES = (1, 2, 3, 7, 9)
# 10 units of 16 bytes a term, one unit of 16 bytes, three units of 8 bytes
TILED_CONTEXTS = [c for c in CONTEXTS if c[0] in (1247, 65, 129)]


def tiled_grid(n, t1, t2, batch, bs_knob=0, m_knob=0):
    """launch_tiled (csgn_mul.hip) at mul_ti = 4: batch * column tiles * row tiles workgroups"""
    U, unit_bytes = units(n)
    m = m_knob if m_knob else (2 if unit_bytes == 8 else 1)
    samek = next((b for b in range(256, 513, 64) if b % U == 0), 256)
    bs = bs_knob or (samek if m_knob > 1 else 256)
    while m > 1 and bs * (m // 2) >= t2 * U:
        m //= 2
    ti = min(4, 32768 // (U * unit_bytes), t1)
    return batch * cdiv(t2 * U, bs * m) * cdiv(t1, ti)


class Products:
    """Nine pairs of every shape at one N: the operands on the device and every pair's words from the oracle, once"""

    def __init__(self, hip, oracle, n):
        self.hip, self.n, dl = hip, n, oracle.default_len(n)
        self.shapes = {}
        for t1, t2 in TILED_SHAPES:
            top = max(TILED_BATCHES)
            L = oracle.synth(6000 + t1, n, 0, top * t1 * dl)
            R = oracle.synth(6100 + t2, n, 0, top * t2 * dl)
            want = np.concatenate([oracle.mul(n, L[b * t1 * dl:(b + 1) * t1 * dl], R[b * t2 * dl:(b + 1) * t2 * dl])[0]
                                   for b in range(top)])
            self.shapes[t1, t2] = (hip.upload(L), hip.upload(R), want)

    def check(self, what):
        dl = self.hip.default_len(self.n)
        for (t1, t2), (d_l, d_r, want) in self.shapes.items():
            for batch in TILED_BATCHES:
                assert self.hip.lib.csgn_mul_uniform_kernel(self.n, batch, t1, t2) == b"k_mul_tiled"
                got = self.hip.download(self.hip.mul_uniform(self.n, batch, t1, t2, d_l, d_r))
                assert np.array_equal(got, want[:batch * t1 * t2 * dl]), (self.n, t1, t2, batch, what)


@pytest.fixture(scope="module", params=TILED_CONTEXTS, ids=lambda c: "n%d" % c[0])
def products(request, hip, oracle):
    return Products(hip, oracle, request.param[0])


def test_tiled_grids_cover_every_residue():
    """Batches 1, 2, 3, 7 and 9 of 33 x 65 and 5 x 300 terms on the three contexts: 27 and 24 workgroups a pair at
    N = 1247, 9 and 4 at N = 65 and 129; every residue mod 8 with a whole round, and a grid of 4."""
    grids = [tiled_grid(n, t1, t2, b) for n, _ in TILED_CONTEXTS for t1, t2 in TILED_SHAPES for b in TILED_BATCHES]
    assert {g % 8 for g in grids if g >= 8} == set(range(8)) and 4 in grids
    assert [tiled_grid(1247, t1, t2, 1) for t1, t2 in TILED_SHAPES] == [27, 24]
    assert [tiled_grid(129, t1, t2, 1) for t1, t2 in TILED_SHAPES] == [9, 4]


def test_tiled_multiply_in_the_contiguous_block_order(products, knobs):
    """mul_flat = -1 with mul_xcd = 2: k_mul_tiled renumbers its workgroups on gridDim.x (a.xcd_remap); every word."""
    knobs.set("mul_flat", -1)
    knobs.set("mul_xcd", 2)
    products.check("mul_xcd 2")


@pytest.mark.parametrize("bs", [64, 128, 192, 320, 512, 100])
def test_tiled_multiply_block_sizes(products, knobs, bs):
    """mul_flat = -1 with mul_bs 64 to 512 by mul_m 0 and 2: the block size sets the column tiles and, where U divides
    it, the shared LDS read of a lane's columns (samek).  100 is no multiple of 64: refused, the default block, and
    still every word."""
    knobs.set("mul_flat", -1)
    knobs.set("mul_bs", bs)
    for m in (0, 2):
        knobs.set("mul_m", m)
        products.check(("mul_bs", bs, "mul_m", m))


def compaction_mix(oracle, n):
    """test_compaction_many_groups_and_sizes' mix (tests/test_gpu_parity.py) cut to 26 ciphertexts: every size class --
    empty, 1 to 39 terms (several share a workgroup), 40 to 699 (one fills a workgroup), 700 to 1399 -- with leading,
    trailing and adjacent empties.  A workgroup's group holds 1024 terms at N = 1247 and 320 at N = 4096: the
    ciphertexts of 1100 and 1399 terms (at 4096 also those of 333 to 700) go by hash partitions."""
    rng = np.random.default_rng(n + 12)
    draws = [0, 3, 39, 1, 17, 640, 0, 0, 0, 25, 1399, 8, 40, 333, 12, 700, 5, 699, 30, 2, 1100, 21, 90, 38, 7, 0]
    cts = []
    for b, d in enumerate(draws):
        pool = max(1, int(d * [0.05, 0.5, 1.0, 3.0][b % 4]))
        cts.append(_dup_ciphertext(oracle, rng, n, 3100 + b, pool, d))
    return cts


# (compact_grid, compact_stagger_us, compact_nt); None: the default (512 workgroups, 8 us, non-temporal stores).  Every
# value of one knob against the others' defaults, and two mixed rows.
COMPACT_ROWS = [(1, None, None), (2, None, None), (3, None, None), (7, None, None), (64, None, None),
                (None, 0, None), (None, 8, None), (None, None, 0), (None, None, 1), (3, 0, 0), (7, 0, 1)]


@pytest.mark.parametrize("n", [1247, 4096])
def test_compaction_on_small_and_odd_persistent_grids(hip, oracle, knobs, n):
    """k_compact_main takes its groups by ticket: grids far below the group count (one workgroup takes every group in
    turn), odd grids, the stagger off, both store kinds.  Term lists identical to oracle.compact."""
    cts = compaction_mix(oracle, n)
    for grid, stagger, nt in COMPACT_ROWS:
        for name, value in (("compact_grid", grid), ("compact_stagger_us", stagger), ("compact_nt", nt)):
            if value is None:
                knobs.unset(name)
            else:
                knobs.set(name, value)
        _check_compaction(hip, oracle, n, cts)


def test_compaction_wide_groups_on_grids_of_one_and_three(hip, oracle, knobs):
    """The wide build (a caller's bound between the narrow and the wide group size, test_compaction_wide_groups' sizes)
    runs one workgroup a CU, half of compact_grid -- at compact_grid = 1 still one workgroup."""
    n, sizes = 1247, [1100, 1792, 3, 1500, 0, 1025, 700]
    rng = np.random.default_rng(n)
    cts = [_dup_ciphertext(oracle, rng, n, 3200 + b, max(1, s // 2), s) for b, s in enumerate(sizes)]
    for grid in (1, 3):
        knobs.set("compact_grid", grid)
        _check_compaction(hip, oracle, n, cts, max_terms=max(sizes))


def test_shared_gpu_takes_the_tiled_kernel(hip, oracle, knobs):
    """shared_gpu = 1: a streaming batch that the operand touch and the flat kernel take by default (16 x 8 terms at
    N = 1247, one of test_mul_default_dispatch_of_streaming_small_shapes, 2000 pairs: 7.7 MB of operands, 41 MB of
    products) goes to the LDS-tiled kernel; the first, the last and sampled pairs against the oracle."""
    n, t1, t2, batch = 1247, 16, 8, 2000
    dl = oracle.default_len(n)
    knobs.unset("shared_gpu")
    assert hip.lib.csgn_mul_uniform_kernel(n, batch, t1, t2) == b"k_touch+k_mul_flat"
    knobs.set("shared_gpu", 1)
    assert hip.lib.csgn_mul_uniform_kernel(n, batch, t1, t2) == b"k_mul_tiled"
    L = hip.synth_fill(83, n, 0, batch * t1 * dl)
    R = hip.synth_fill(84, n, 0, batch * t2 * dl)
    out = hip.mul_uniform(n, batch, t1, t2, L, R)
    hl, hr = hip.download(L), hip.download(R)
    per = t1 * t2 * dl
    picks = {0, 1, batch // 2, batch - 2, batch - 1} | set(np.random.default_rng(5).integers(0, batch, 24).tolist())
    for b in sorted(picks):
        want, _ = oracle.mul(n, hl[b * t1 * dl:(b + 1) * t1 * dl], hr[b * t2 * dl:(b + 1) * t2 * dl])
        assert np.array_equal(hip.download(out[b * per:(b + 1) * per]), want), b
