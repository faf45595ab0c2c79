"""Gates and plaintext constants (csgn_gate_*, csgn_const_fill) on a box without a GPU: the term-count table, the
dispatch names, the loud failure without a device, and the DEFINITION of every gate -- the composition of the
reference's operator+ / operator* with an all-ones (ONE) or all-zero (ZERO) term -- pinned against the compiled
reference and the oracle.  The device side is tests/test_gates_gpu.py."""

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (ADD_PLAIN, GATES, MASK64, MUL_PLAIN, MUX, NAND, NOR, NOT, OR, compose_gate, const_term,
                         gate_clear, gate_terms, lib, np_gate, oracle_ops, rand_terms, ref_ops)


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_gate_terms_table(lib):
    for gate in GATES.values():
        for ts, ta, tb in [(1, 1, 1), (1, 2, 3), (3, 5, 2), (64, 64, 64), (7, 1, 9)]:
            assert lib.csgn_gate_terms(gate, ts, ta, tb) == gate_terms(gate, ts, ta, tb), (gate, ts, ta, tb)
    for bad in (0, 9, -1, 100):
        assert lib.csgn_gate_terms(bad, 1, 1, 1) == 0
    assert lib.csgn_gate_terms(NOT, 0, 0, 0) == 0                  # an operand the gate reads has no terms
    assert lib.csgn_gate_terms(NOT, 0, 5, 0) == 6                  # ... the ones it does not read may be 0
    assert lib.csgn_gate_terms(OR, 0, 1, 0) == 0
    assert lib.csgn_gate_terms(MUX, 0, 1, 1) == 0
    assert lib.csgn_gate_terms(NAND, 0, 1 << 32, 1 << 32) == 0     # overflow
    assert lib.csgn_gate_terms(MUX, 1 << 40, 1 << 30, 1) == 0
    assert lib.csgn_gate_terms(NOT, 0, MASK64, 0) == 0


def test_gate_dispatch_names(lib, knobs):
    knobs.unset("gate_fused")
    name = lambda g, ts, ta, tb, n=1247: lib.csgn_gate_uniform_kernel(n, g, 1 << 20, ts, ta, tb).decode()
    for g in GATES.values():
        assert name(g, 1, 1, 1) == "k_gate_fused", g               # fresh operands: one kernel
    for g in (NAND, OR, NOR):
        assert name(g, 0, 64, 64) == "pitched", g                  # large products: the tuned multiply launchers
    assert name(MUX, 1, 64, 64) == "pitched"
    assert name(MUX, 2, 64, 64) == "k_gate_fused"                  # no pitched form without an intermediate buffer
    assert name(MUL_PLAIN, 0, 64, 0) == "k_gate_fused"
    assert name(NOT, 0, 1000, 0) == "k_gate_fused"                 # copies and a constant: always one pass
    assert name(OR, 0, 8, 8) == "k_gate_fused" and name(OR, 0, 9, 8) == "pitched"   # the cut: 64 product terms
    assert name(0, 1, 1, 1) == ""
    knobs.set("gate_fused", 1)
    assert name(OR, 0, 64, 64) == "k_gate_fused"
    knobs.set("gate_fused", 0)
    assert name(OR, 0, 1, 1) == "pitched"


def test_gate_entry_points_fail_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gates_gpu.py covers the device")
    buf = np.zeros(4096, dtype=np.uint64)
    plain = np.ones(8, dtype=np.uint8)
    p = buf.ctypes.data
    rc = lib.csgn_gate_uniform(1247, OR, 4, 0, 1, 1, None, p, p, None, p, None)
    assert rc == -3, lib.csgn_last_error()
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert lib.csgn_gate_uniform(1247, ADD_PLAIN, 4, 0, 1, 0, None, p, None, plain.ctypes.data, p, None) == -3
    assert lib.csgn_const_fill(1247, 4, None, 1, p, None) == -3
    assert lib.csgn_const_fill(1247, 4, plain.ctypes.data, 0, p, None) == -3
    # argument errors are reported before the device is looked for
    assert lib.csgn_gate_uniform(1247, 42, 4, 0, 1, 1, None, p, p, None, p, None) == -1
    assert lib.csgn_gate_uniform(0, OR, 4, 0, 1, 1, None, p, p, None, p, None) == -1
    assert lib.csgn_gate_uniform(1247, NAND, 4, 0, 1 << 20, 1 << 20, None, p, p, None, p, None) == -2


# -- the definition against the genuine reference -----------------------------------------------------------------------
# N % 64 != 0 only: at N % 64 == 0 the reference writes one past its bitlen array in encrypt and permutation (VERDICT
# row a8); N = 64 and 4096 are pinned against the oracle below.
@pytest.mark.parametrize("n,d", [(63, 4), (65, 4), (129, 8), (1247, 16)])
@pytest.mark.parametrize("gate", sorted(GATES.values()))
@pytest.mark.parametrize("ts,ta,tb", [(1, 1, 1), (2, 1, 3), (1, 3, 2), (3, 2, 2)])
def test_gate_definition_matches_reference(oracle, ref, n, d, gate, ts, ta, tb):
    a, b, s = (rand_terms(n, 1, t, seed)[0].ravel() for t, seed in ((ta, 1), (tb, 2), (ts, 3)))
    for p in (0, 1):
        want = compose_gate(ref_ops(ref, n, d), n, gate, a, b, s, p)
        got = compose_gate(oracle_ops(oracle, n), n, gate, a, b, s, p)
        assert np.array_equal(got, want), (gate, p)
        assert got.size == gate_terms(gate, ts, ta, tb) * ((n + 63) // 64)
        words = np_gate(n, gate, a[None].reshape(1, ta, -1), b[None].reshape(1, tb, -1), s[None].reshape(1, ts, -1),
                        plain=[p])
        assert np.array_equal(words.ravel(), got)


@pytest.mark.parametrize("n", [64, 4096, 63, 1247])
@pytest.mark.parametrize("gate", sorted(GATES.values()))
def test_gate_definition_matches_oracle(oracle, n, gate):
    ts, ta, tb, batch = 2, 3, 2, 5
    a, b, s = rand_terms(n, batch, ta, 7), rand_terms(n, batch, tb, 8), rand_terms(n, batch, ts, 9)
    plain = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    words = np_gate(n, gate, a, b, s, plain)
    for e in range(batch):
        want = compose_gate(oracle_ops(oracle, n), n, gate, a[e].ravel(), b[e].ravel(), s[e].ravel(), int(plain[e]))
        assert np.array_equal(words[e].ravel(), want), e


@pytest.mark.parametrize("n,d", [(63, 4), (64, 4), (1247, 16), (4096, 32)])
def test_constants_and_truth_tables_decrypt(oracle, n, d):
    """ONE decrypts to 1 and ZERO to 0 under every key, and every gate's composition decrypts to the gate of the
    decryptions (the oracle's decrypt is the reference's, tests/test_oracle_vs_ref.py)."""
    dl = (n + 63) // 64
    for k in range(4):
        key, _ = oracle.keygen(n, d, glibc_draws(100 + k, 64 * d + 64))
        assert oracle.decrypt_canonical(n, key, const_term(n, 1)) == 1
        assert oracle.decrypt_canonical(n, key, const_term(n, 0)) == 0
        bits = [0, 1] * 4
        cts, _ = oracle.encrypt_seq(n, key, bits, glibc_draws(200 + k, len(bits) * (n + 2)))
        ct = [cts[i * dl:(i + 1) * dl] for i in range(len(bits))]
        ops = oracle_ops(oracle, n)
        for gate in GATES.values():
            for s in (0, 1):
                for x in (0, 1):
                    for y in (0, 1):
                        for p in (0, 1):
                            w = compose_gate(ops, n, gate, ct[x], ct[2 + y], ct[4 + s], p)
                            assert oracle.decrypt_canonical(n, key, w) == gate_clear(gate, x, y, s, p), \
                                (gate, s, x, y, p)
