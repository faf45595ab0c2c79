"""The inputs of tests/test_decrypt_gpu.py, checked on the CPU: np_decrypt (tests/model_decrypt.py) is pinned to the
oracle and to the compiled reference, and every batch the GPU tests decrypt is shown to notice a decryption that ignores
any ONE key position, in every slot of a pass-1 workgroup, and a pass 2 that loses any ONE of the boundary hits.  The
last test records that the inputs of the older decrypt tests (tests/model.py: planted) notice neither."""
import numpy as np
import pytest

from oracle.binding import canonical_bitlen
from tests.model import csr, make_key, np_add, np_mul, planted
from tests.model_decrypt import (CONTEXTS, FILLS, FUSED_SHAPES, LONG, LONG_T, RAGGED_COUNTS, RAGGED_RUNS, Table,
                                 boundary_positions, every_position, forms, fused_operands, lane_key, lanes, long_ragged,
                                 long_uniform, mutant_bits, near_misses, np_bits, np_decrypt, np_hits, np_key_mask,
                                 pass1_form, reachable_K, regroup, slot_coverage, slot_hits, slot_list, slot_need,
                                 slot_rotations, slot_terms, with_empties, without_hit)

POSITION_CONTEXTS = [(63, 4), (1247, 16), (4096, 32)]


def slot_cases(n, d):
    tab = Table(n, d)
    for r in slot_rotations(tab):
        c = slot_list(tab, r)
        yield c
        yield regroup(c, 3)


def position_cases(n, d):
    tab = Table(n, d)
    for hits in (0, 1, 2):
        c = every_position(tab, hits)
        yield c
        yield with_empties(c)


LONG_RUNS = ((False, False), (True, False), (False, True))           # (double, mirror)


def long_uniform_cases():
    for n, d, T in [(63, 4, T) for T in LONG_T] + [(1247, 16, 4097)]:
        for double, mirror in LONG_RUNS:
            yield long_uniform(Table(n, d), T, double, mirror)


def long_ragged_cases():
    for q in range(RAGGED_RUNS):
        yield long_ragged(Table(63, 4), q)


def oracle_bits(oracle, c):
    dl = c.words.shape[1]
    flat = c.words.reshape(-1)
    return np.array([oracle.decrypt_canonical(c.n, c.key, flat[int(s) * dl:int(e) * dl]) if e > s else 0
                     for s, e in zip(c.off[:-1], c.off[1:])], dtype=np.uint8)


def check_case(oracle, c):
    """np_decrypt is the oracle's decryption, and ignoring any one key position changes at least one bit."""
    want = c.want()
    assert np.array_equal(want, oracle_bits(oracle, c)), c.label
    changed = (mutant_bits(c.n, c.key, c.words, c.off) != want).any(axis=1)
    assert changed.all(), (c.label, "key positions no bit depends on", np.flatnonzero(~changed).tolist())
    return want


# -- the model itself --------------------------------------------------------------------------------------------------
def test_host_rule_table():
    """The forms tests/test_decrypt_gpu.py relies on, by the pure Python copy of the host rule; K = 4, 6 and 8 are out
    of the rule's reach at every term size."""
    for (n, d), (aligned, moved) in CONTEXTS.items():
        fs = forms(n)
        assert fs[0] == (False, aligned), (n, fs[0])
        assert (fs[1] == (True, moved)) if moved else len(fs) == 1, (n, fs)
    assert reachable_K() == [1, 2, 3, 5, 7]
    seg = {f[2] for (n, d) in CONTEXTS for _, f in forms(n)}
    assert seg == {0, 1, 2, 3, 5, 7}
    assert {f[:3] for (n, d) in CONTEXTS for _, f in forms(n) if f[2] == 7} == {(8, 7, 7), (16, 7, 7), (8, 14, 7)}
    assert pass1_form(8320, False)[1] == 65 and pass1_form(8320, True)[1] == 130


@pytest.mark.parametrize("n,d", list(CONTEXTS))
def test_near_misses_miss_exactly_one_position(oracle, n, d):
    key = lane_key(n, d)
    assert d < 4 or n < 128 or lanes(key) == {0, 1, 2, 3}
    assert np.array_equal(np_key_mask(n, key), oracle.key_mask(n, key))
    for fill in FILLS:
        misses, hit = near_misses(n, key, fill, 41)
        kb = np.stack([np_hits(n, [k], misses) for k in key], axis=1)       # [term, position]
        assert np.array_equal(kb, ~np.eye(d, dtype=bool)), fill
        assert np_decrypt(n, key, hit) == 1 == oracle.decrypt_canonical(n, key, hit)
        assert not np_hits(n, key, misses).any()
        assert all(oracle.decrypt_canonical(n, key, m) == 0 for m in misses)
        last = np.uint64((1 << (64 - n % 64)) - 1 if n % 64 else 0)
        assert not (misses[:, -1] & last).any() and not (hit[-1] & last)    # canonical terms
        assert np_decrypt(n, key, np.concatenate([misses.ravel(), hit])) == 1
    assert np_decrypt(n, key, np.zeros(0, np.uint64)) == 0


@pytest.mark.parametrize("n,d", list(CONTEXTS))
def test_near_misses_through_the_reference(ref, n, d):
    """The genuine reference's decrypt with the canonical bitlen: 0 for every near miss, 1 for the hit and for the d
    near misses and the hit as one ciphertext."""
    key = lane_key(n, d)
    for fill in FILLS:
        misses, hit = near_misses(n, key, fill, 41)
        for m in misses:
            assert ref.decrypt(n, d, key, m, canonical_bitlen(n, 1)) == 0 == np_decrypt(n, key, m)
        assert ref.decrypt(n, d, key, hit, canonical_bitlen(n, 1)) == 1
        both = np.concatenate([misses.ravel(), hit])
        assert ref.decrypt(n, d, key, both, canonical_bitlen(n, d + 1)) == 1 == np_decrypt(n, key, both)
        assert ref.decrypt(n, d, key, misses.ravel(), canonical_bitlen(n, d)) == 0


@pytest.mark.parametrize("n,d", [(1247, 16), (4096, 32), (63, 4), (129, 3)])
def test_np_decrypt_on_planted_inputs(oracle, n, d):
    key = make_key(n, d, 3)
    for terms, hits, seed in [(1, 0, 1), (1, 1, 2), (5, 3, 3), (64, 64, 4), (257, 100, 5), (1000, 501, 6)]:
        v = planted(oracle, n, key, terms, hits, seed)
        assert np_decrypt(n, key, v) == hits % 2 == oracle.decrypt_canonical(n, key, v)


# -- a. every key position, every slot ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", list(CONTEXTS))
def test_slot_lists_see_every_key_position_in_every_slot(oracle, n, d):
    tab = Table(n, d)
    rs = slot_rotations(tab)
    M = slot_terms(n)
    assert M >= 515 and all(M >= 2 * f[3] + 3 and M % f[3] for _, f in forms(n))
    for _, f in forms(n):
        seen = set()
        for r in rs:
            seen |= slot_coverage(tab, f, M, r, slot_hits(M))
        assert seen >= slot_need(tab, f), (f, sorted(slot_need(tab, f) - seen, key=str))
    for c in slot_cases(n, d):
        want = check_case(oracle, c)
        if c.T == 1:
            assert np.array_equal(np.flatnonzero(want), sorted(slot_hits(M)))       # near misses alone give 0
        assert 0 < want.sum() < c.batch


# -- b. one hit at every position --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", POSITION_CONTEXTS)
def test_every_position_batches(oracle, n, d):
    cases = list(position_cases(n, d))
    for c in cases:
        want = check_case(oracle, c)
        hits = int(c.label.split(",")[1].split()[0])
        full = np.diff(c.off.astype(np.int64)) > 0
        assert (want[full] == (hits == 1)).all() and not want[~full].any(), c.label
        assert c.batch == (130 if c.T else 133)
    one = cases[2]
    assert sorted({q % 64 for q in one.planted}) == list(range(64))                 # every bit of a bitmap word
    for b in (0, 1, 63, 64, 129):                                                   # clearing the one hit clears the bit
        got = without_hit(one, one.planted[b]).want()
        assert np.array_equal(np.flatnonzero(got != one.want()), [b])


# -- c. / d. long ciphertexts ------------------------------------------------------------------------------------------
def test_boundary_positions():
    assert boundary_positions(4097) == [0, 1, 62, 63, 64, 65, 4095, 4096]
    assert boundary_positions(65535) == [0, 1, 62, 63, 64, 65, 65533, 65534]
    assert boundary_positions(65537) == [0, 1, 62, 63, 64, 65, 65535, 65536]
    assert boundary_positions(131073) == [0, 1, 62, 63, 64, 65, 65535, 65536, 65537, 131071, 131072]
    assert RAGGED_RUNS == 11


def test_long_uniform_batches(oracle):
    for c in long_uniform_cases():
        want = check_case(oracle, c)
        double, mirror = "double" in c.label, "mirror" in c.label
        P = boundary_positions(c.T)[::-1] if mirror else boundary_positions(c.T)
        assert c.T > LONG and c.batch % 2 == 1 and c.T % 64 and c.batch in (len(P), len(P) + 1)
        assert (want[:len(P)] == (not double)).all() and not want[len(P):].any(), c.label
        assert len(c.planted) == len(P) * (2 if double else 1)
        if not double:                                                  # every boundary hit carries its ciphertext's bit
            assert c.planted[-1 if mirror else 0] % c.T == 0           # a hit at a ciphertext's first term ...
            assert (c.planted[0 if mirror else len(P) - 1] + 1) % c.T == 0     # ... and one at a last term
            for b, q in enumerate(c.planted):
                assert q == b * c.T + P[b]
                got = without_hit(c, q).want()
                assert np.array_equal(np.flatnonzero(got != want), [b]), (c.label, q)


def test_long_ragged_batches(oracle):
    off = csr(list(RAGGED_COUNTS)).astype(np.int64)
    assert [int(s) % 64 for s, t in zip(off, RAGGED_COUNTS) if t > LONG] == [3, 4, 6, 7]
    for q, c in enumerate(long_ragged_cases()):
        want = check_case(oracle, c)
        for b, t in enumerate(RAGGED_COUNTS):
            assert want[b] == (t > LONG and q < len(boundary_positions(t))), (q, b)
        for term in c.planted:
            b = int(np.searchsorted(off, term, side="right") - 1)
            assert term - off[b] == boundary_positions(RAGGED_COUNTS[b])[q]
            got = without_hit(c, term).want()
            assert np.array_equal(np.flatnonzero(got != want), [b]), (q, term)


# -- e. the fused product and sum --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(1247, 16), (129, 3)])
def test_fused_operands(oracle, n, d):
    tab = Table(n, d)
    seen = np.zeros(d, dtype=bool)
    for t1, t2 in FUSED_SHAPES:
        L, R = fused_operands(tab, t1, t2)
        batch = L.shape[0]
        dl_, dr_ = np_bits(n, tab.key, L, np.arange(batch + 1) * t1), np_bits(n, tab.key, R, np.arange(batch + 1) * t2)
        assert {(int(a), int(b)) for a, b in zip(dl_, dr_)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        prod, summ = np_mul(L, R), np_add(L, R)
        wp = np_bits(n, tab.key, prod, np.arange(batch + 1) * t1 * t2)
        ws = np_bits(n, tab.key, summ, np.arange(batch + 1) * (t1 + t2))
        assert np.array_equal(wp, dl_ & dr_) and np.array_equal(ws, dl_ ^ dr_)
        for b in range(batch):
            assert wp[b] == oracle.decrypt_canonical(n, tab.key, oracle.mul(n, L[b].ravel(), R[b].ravel())[0])
            assert ws[b] == oracle.decrypt_canonical(n, tab.key, oracle.add(L[b].ravel(), R[b].ravel())[0])
        # a fused decrypt that ignores one key position changes a bit of the product and of the sum, in one shape at least
        ml = mutant_bits(n, tab.key, L, np.arange(batch + 1) * t1)
        mr = mutant_bits(n, tab.key, R, np.arange(batch + 1) * t2)
        seen |= ((ml & mr) != wp).any(axis=1) & ((ml ^ mr) != ws).any(axis=1)
    assert seen.all(), np.flatnonzero(~seen).tolist()


# -- why this file exists ----------------------------------------------------------------------------------------------
def blind_positions(oracle, n, d):
    """The inputs of test_gpu_parity.py: test_decrypt_uniform_matches_oracle, rebuilt: how many of the d mutants (a
    decryption that ignores ONE key position) change any bit those inputs expect."""
    key = make_key(n, d, 3)
    seen = np.zeros(d, dtype=bool)
    for terms in (1, 2, 5, 64, 255, 256, 257, 1000):
        parts = [planted(oracle, n, key, terms, (b * 3) % (terms + 1), 100 + b) for b in range(7)]
        words, off = np.concatenate(parts), np.arange(8) * terms
        want = np_bits(n, key, words, off)
        assert np.array_equal(want, [((b * 3) % (terms + 1)) % 2 for b in range(7)])
        seen |= (mutant_bits(n, key, words, off) != want).any(axis=1)
    return seen


def test_planted_inputs_do_not_see_the_key_positions(oracle):
    """planted() clears only key[0] in its non-hits, and at d = 16 a random term carries the other fifteen key bits with
    probability 2^-15: 0 of the 16 mutants change any bit at N = 1247 (measured: 0 of 16; 0 of 32 at N = 4096 / d = 32;
    1 of 4 -- key[0] alone -- at N = 63 / d = 4).  The batches of tests/model_decrypt.py see 16 of 16 (check_case).  Do
    not fold the decrypt tests back onto planted()."""
    assert blind_positions(oracle, 1247, 16).sum() == 0
    assert blind_positions(oracle, 4096, 32).sum() == 0
    assert blind_positions(oracle, 63, 4).tolist() == [True, False, False, False]
