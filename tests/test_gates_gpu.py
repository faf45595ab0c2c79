"""Gates and plaintext constants on the device (csgn_gate_uniform, csgn_const_fill), word for word against the
definition of include/csgn_hip.h (pinned against the reference and the oracle in tests/test_gates_cpu.py), in both
forms the knob gate_fused selects, and by decryption under random keys.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (ADD_PLAIN, GATES, GuardedOutputs, MUL_PLAIN, MUX, NOT, compose_gate, const_term, gate_clear,
                         gate_terms, hip, np_gate, oracle_ops, rand_terms)

pytestmark = pytest.mark.gpu

NS = [63, 64, 65, 129, 1247, 4096]
# (t_sel, t_a, t_b, batch): fresh operands up to past the fused / pitched cut (64 product terms per element)
SHAPES = [(1, 1, 1, 1), (1, 1, 1, 1000), (2, 1, 3, 3), (1, 4, 4, 1000), (1, 5, 4, 3), (3, 8, 8, 3), (1, 9, 8, 3),
          (1, 64, 64, 3)]


def run_gate(hip, n, gate, a, b, s, plain, want=None):
    """The output, downloaded.  With `want` (the definition's words) the output is a caller tensor of exactly that size
    between guard words, checked word for word and for writes outside it (tests/model.py, GuardedOutputs)."""
    batch, ta, _ = a.shape
    up = hip.upload
    guarded = GuardedOutputs(hip, [want.size]) if want is not None else None
    out = hip.gate_uniform(n, gate, batch, up(a.ravel()), ta, up(b.ravel()), b.shape[1], up(s.ravel()), s.shape[1],
                           up(plain), out=guarded.outs[0] if guarded else None)
    return guarded.check([want], gate)[0] if guarded else hip.download(out)


def operands(n, ts, ta, tb, batch, seed):
    a, b, s = rand_terms(n, batch, ta, seed), rand_terms(n, batch, tb, seed + 1), rand_terms(n, batch, ts, seed + 2)
    plain = np.random.default_rng(seed + 3).integers(0, 2, batch).astype(np.uint8)
    return a, b, s, plain


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("gate", sorted(GATES.values()))
@pytest.mark.parametrize("shape", SHAPES)
def test_gate_words(hip, oracle, knobs, n, gate, shape):
    ts, ta, tb, batch = shape
    if n == 4096 and ta == 64:
        batch = 1
    a, b, s, plain = operands(n, ts, ta, tb, batch, 1000 * gate + ta)
    want = np_gate(n, gate, a, b, s, plain).ravel()
    assert want.size == batch * gate_terms(gate, ts, ta, tb) * ((n + 63) // 64)
    # the first and last element also straight through the oracle's operators
    ops = oracle_ops(oracle, n)
    per = want.size // batch
    for e in {0, batch - 1}:
        o = compose_gate(ops, n, gate, a[e].ravel(), b[e].ravel(), s[e].ravel(), int(plain[e]))
        assert np.array_equal(want[e * per:(e + 1) * per], o)
    for fused in (-1, 0, 1):
        knobs.set("gate_fused", fused)
        got = run_gate(hip, n, gate, a, b, s, plain, want)
        assert np.array_equal(got, want), (fused, hip.lib.csgn_gate_uniform_kernel(n, gate, batch, ts, ta, tb))


@pytest.mark.parametrize("n", [65, 1247, 4096])
@pytest.mark.parametrize("gate", sorted(GATES.values()))
def test_gate_words_large_batch(hip, knobs, n, gate):
    """65 537 fresh elements: more than one workgroup row of every kind, odd element count."""
    a, b, s, plain = operands(n, 1, 1, 1, 65537, 77 + gate)
    want = np_gate(n, gate, a, b, s, plain).ravel()
    for fused in (0, 1):
        knobs.set("gate_fused", fused)
        assert np.array_equal(run_gate(hip, n, gate, a, b, s, plain, want), want), fused


@pytest.mark.parametrize("n", NS)
def test_const_fill(hip, n):
    batch = 1001
    plain = np.random.default_rng(n).integers(0, 256, batch).astype(np.uint8)   # bit 0 decides
    got = hip.download(hip.const_fill(n, batch, hip.upload(plain))).reshape(batch, -1)
    for e in range(batch):
        assert np.array_equal(got[e], const_term(n, plain[e] & 1)), e
    for bit in (0, 1):
        got = hip.download(hip.const_fill(n, batch, None, bit)).reshape(batch, -1)
        assert (got == const_term(n, bit)[None, :]).all()


@pytest.mark.parametrize("n,d", [(63, 4), (64, 4), (1247, 16), (4096, 32)])
def test_gate_truth_tables_decrypt(hip, oracle, n, d):
    """Dec(gate(a, b)) == gate(Dec a, Dec b) on the device, under several keys, for every input combination."""
    dl = (n + 63) // 64
    for k in range(3):
        key, _ = oracle.keygen(n, d, glibc_draws(300 + k, 64 * d + 64))
        mask = hip.upload(oracle.key_mask(n, key))
        combos = [(s, x, y, p) for s in (0, 1) for x in (0, 1) for y in (0, 1) for p in (0, 1)] * 2
        bits = np.array(combos, dtype=np.uint8)
        batch = len(combos)
        enc = lambda col, seed: oracle.encrypt_seq(n, key, bits[:, col], glibc_draws(seed, batch * (n + 2)))[0]
        s_ct, a_ct, b_ct = enc(0, 400 + k), enc(1, 500 + k), enc(2, 600 + k)
        for gate in GATES.values():
            out = hip.gate_uniform(n, gate, batch, hip.upload(a_ct), 1, hip.upload(b_ct), 1, hip.upload(s_ct), 1,
                                   hip.upload(bits[:, 3].copy()))
            terms = gate_terms(gate, 1, 1, 1)
            dec = hip.download(hip.decrypt_uniform(n, batch, terms, out, mask))
            host = hip.download(out).reshape(batch, terms * dl)
            for e, (s, x, y, p) in enumerate(combos):
                want = gate_clear(gate, x, y, s, p)
                assert dec[e] == want, (gate, s, x, y, p)
                assert oracle.decrypt_canonical(n, key, host[e]) == want


@pytest.mark.parametrize("n", [65, 1247])
def test_plain_gates_random_bits(hip, oracle, n):
    d = 8
    key, _ = oracle.keygen(n, d, glibc_draws(9, 64 * d + 64))
    mask = hip.upload(oracle.key_mask(n, key))
    batch = 257
    rng = np.random.default_rng(n)
    bits, plain = rng.integers(0, 2, batch).astype(np.uint8), rng.integers(0, 2, batch).astype(np.uint8)
    a = hip.upload(oracle.encrypt_seq(n, key, bits, glibc_draws(10, batch * (n + 2)))[0])
    for gate, terms in ((ADD_PLAIN, 2), (MUL_PLAIN, 1)):
        out = hip.gate_uniform(n, gate, batch, a, 1, plain=hip.upload(plain))
        dec = hip.download(hip.decrypt_uniform(n, batch, terms, out, mask))
        assert np.array_equal(dec, bits ^ plain if gate == ADD_PLAIN else bits & plain)


def test_not_not_compacts_to_the_operand(hip):
    """NOT(NOT a) = a + ONE + ONE: the two constants cancel in a mod-2 compaction, a's terms stay."""
    import torch
    n, batch, ta = 1247, 100, 3
    dl = (n + 63) // 64
    a = rand_terms(n, batch, ta, 5)
    na = hip.gate_uniform(n, NOT, batch, hip.upload(a.ravel()), ta)
    nna = hip.gate_uniform(n, NOT, batch, na, ta + 1)
    off = torch.arange(0, batch * (ta + 2) + 1, ta + 2, dtype=torch.int64, device=hip.device)
    words, off_out = hip.compact_ragged(n, nna, off)
    assert np.array_equal(hip.download(off_out), np.arange(0, batch * ta + 1, ta, dtype=np.uint64))
    assert np.array_equal(hip.download(words)[: batch * ta * dl], a.ravel())


def test_gate_argument_errors(hip):
    L = hip.lib
    x = hip.empty_words(64)
    p = x.data_ptr()
    assert L.csgn_gate_uniform(1247, 99, 1, 1, 1, 1, p, p, p, p, p, 0) == -1
    assert L.csgn_gate_uniform(1247, 4, 1, 0, 1, 1, None, p, None, None, p, 0) == -1     # OR reads b
    assert L.csgn_gate_uniform(1247, MUX, 1, 1, 1, 1, None, p, p, None, p, 0) == -1       # MUX reads sel
    assert L.csgn_gate_uniform(1247, ADD_PLAIN, 1, 0, 1, 0, None, p, None, None, p, 0) == -1
    assert L.csgn_gate_uniform(1247, NOT, 0, 0, 1, 0, None, None, None, None, None, 0) == 0   # empty batch
    assert L.csgn_const_fill(1247, 1, None, 1, None, 0) == -1
