"""Operands and results that are 8-byte but not 16-byte aligned, at even word counts.

Every device entry point compiles its kernels for 16-byte units and for 8-byte units, and the host side takes the wide
form only when dL = ceil(N / 64) is even AND every pointer is 16-byte aligned.  The C ABI promises only uint64_t
alignment, so a caller's arena, a torch view at an odd word offset or a pinned buffer behind a header run the 8-byte form
at N = 1247 or 4096 -- with unit counts (U = 20, 64) and trip counts the rest of the suite, whose buffers are fresh
allocations, never gives it.  Here each pointer argument is moved one word into its buffer, alone and then all of them,
and the words (and bits) must equal the numpy or oracle definition AND the same call on aligned buffers.  N = 1300 (odd
dL, the 8-byte form either way) is the control.  Outputs carry a guard word on either side.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import (ADD_FULL, ADD_HALF, EQ, GATES, GE, GT, LE, LT, NE, STEPS, const_term, csr, explicit_randomness,
                         gate_terms, hip, make_key, np_add, np_gate, np_mul, np_plain, np_step, planted, rand_terms,
                         u64s)

pytestmark = pytest.mark.gpu

NS = [1247, 4096, 128, 1300]                # even dL (20, 64, 2) and one odd (21)
KEY_D = {1247: 16, 4096: 32, 128: 8, 1300: 4}
GUARD = 0x5A5A5A5A5A5A5A5A


def patterns(names):
    """No pointer moved (the reference call), each one alone, then all of them."""
    return [frozenset()] + [frozenset([x]) for x in names] + ([frozenset(names)] if len(names) > 1 else [])


# Device copies made for the current call.  A pointer handed to the library must outlive the launch: a tensor dropped
# right after data_ptr() goes back to torch's caching allocator and its block is handed out again at once.
HELD = []


def place(hip, a, moved):
    """Device copy of `a` (held until the call's pattern is done); with `moved` it starts one word (8 bytes) into its
    buffer."""
    a = np.ascontiguousarray(a).ravel()
    if a.dtype != np.uint64 or not moved:
        t = hip.upload(a)
        assert t.data_ptr() % 16 == 0
    else:
        t = hip.upload(np.concatenate([np.zeros(1, np.uint64), a]))[1:]
        assert t.data_ptr() % 16 == 8
    HELD.append(t)
    return t


def up(hip, a):
    return place(hip, a, False)


class Out:
    """`k` output words with a guard word before and after them (moved: the words start 8 bytes into the buffer)."""

    def __init__(self, hip, k, moved):
        self.hip, self.k, self.moved = hip, int(k), moved
        s = 1 if moved else 2
        self.buf = hip.empty_words(self.k + 3)
        self.buf.fill_(GUARD)
        self.view = self.buf[s:s + self.k]
        assert self.view.data_ptr() % 16 == (8 if moved else 0)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def words(self, k=None):
        h = self.hip.download(self.buf)
        s = 1 if self.moved else 2
        assert (h[:s] == np.uint64(GUARD)).all() and (h[s + self.k:] == np.uint64(GUARD)).all(), "write outside the output"
        return h[s:s + (self.k if k is None else int(k))]


def same_for_every_pattern(names, call):
    """call(moved) -> tuple of arrays; all patterns give the words of the aligned call, which is returned."""
    base = None
    for moved in patterns(names):
        got = tuple(np.asarray(g) for g in call(moved))
        torch.cuda.synchronize()
        HELD.clear()
        if base is None:
            base = got
            continue
        for i, (g, b) in enumerate(zip(got, base)):
            assert np.array_equal(g, b), (sorted(moved), i)
    return base


# ------------------------------------------------------------------------------ add

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("t1,t2,batch", [(1, 1, 9), (3, 5, 4), (17, 2, 3)])
def test_add_uniform(hip, n, t1, t2, batch):
    L, R = rand_terms(n, batch, t1, 1 + t1), rand_terms(n, batch, t2, 2 + t2)
    want = np_add(L, R).ravel()

    def call(moved):
        out = Out(hip, want.size, "out" in moved)
        dl_, dr_ = place(hip, L, "L" in moved), place(hip, R, "R" in moved)
        assert hip.lib.csgn_add_uniform(n, batch, t1, t2, dl_.data_ptr(), dr_.data_ptr(), out.ptr, hip.stream) == 0
        return (out.words(),)

    assert np.array_equal(same_for_every_pattern(["L", "R", "out"], call)[0], want)


def ragged_operands(n, t1s, t2s, seed):
    dl = (n + 63) // 64
    L = rand_terms(n, 1, max(1, int(sum(t1s))), seed).ravel()
    R = rand_terms(n, 1, max(1, int(sum(t2s))), seed + 1).ravel()
    offL, offR = csr(t1s), csr(t2s)
    pairs = [(L[int(offL[b]) * dl:int(offL[b + 1]) * dl].reshape(1, -1, dl),
              R[int(offR[b]) * dl:int(offR[b + 1]) * dl].reshape(1, -1, dl)) for b in range(len(t1s))]
    return L, R, offL, offR, pairs


@pytest.mark.parametrize("n", NS)
def test_add_ragged(hip, n):
    t1s, t2s = [1, 0, 3, 17, 1, 0, 2, 40], [1, 4, 0, 9, 33, 0, 2, 1]
    L, R, offL, offR, pairs = ragged_operands(n, t1s, t2s, 11)
    want = np.concatenate([np_add(a, b).ravel() for a, b in pairs])
    total = sum(t1s) + sum(t2s)

    def call(moved):
        out = Out(hip, want.size, "out" in moved)
        off_out = hip.empty_words(len(t1s) + 1)
        dl_, dr_ = place(hip, L, "L" in moved), place(hip, R, "R" in moved)
        assert hip.lib.csgn_add_ragged_bounded(n, len(t1s), 0, 0, dl_.data_ptr(), up(hip, offL).data_ptr(),
                                               dr_.data_ptr(), up(hip, offR).data_ptr(), out.ptr,
                                               off_out.data_ptr(), total, hip.stream) == 0
        return out.words(), hip.download(off_out)

    got, off_out = same_for_every_pattern(["L", "R", "out"], call)
    assert np.array_equal(off_out, offL + offR)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------ multiply

MUL_FORMS = [("stream", 1, 1, 300, {}, "k_and_stream"), ("flat", 3, 5, 7, {"mul_flat": 1}, None),
             ("tiled", 17, 9, 2, {"mul_flat": -1}, None), ("default", 5, 3, 4, {}, None)]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", MUL_FORMS, ids=[f[0] for f in MUL_FORMS])
def test_mul_uniform(hip, oracle, knobs, n, form):
    _, t1, t2, batch, kn, kernel = form
    for k, v in kn.items():
        knobs.set(k, v)
    if kernel:
        assert hip.lib.csgn_mul_uniform_kernel(n, batch, t1, t2).decode() == kernel
    L, R = rand_terms(n, batch, t1, 3 + t1), rand_terms(n, batch, t2, 4 + t2)
    want = np_mul(L, R).ravel()
    per = want.size // batch
    assert np.array_equal(want[:per], oracle.mul(n, L[0].ravel(), R[0].ravel())[0])
    assert np.array_equal(want[-per:], oracle.mul(n, L[-1].ravel(), R[-1].ravel())[0])

    def call(moved):
        out = Out(hip, want.size, "out" in moved)
        dl_, dr_ = place(hip, L, "L" in moved), place(hip, R, "R" in moved)
        assert hip.lib.csgn_mul_uniform(n, batch, t1, t2, dl_.data_ptr(), dr_.data_ptr(), out.ptr, 0, hip.stream) == 0
        return (out.words(),)

    assert np.array_equal(same_for_every_pattern(["L", "R", "out"], call)[0], want)


def ragged_batches(n):
    rng = np.random.default_rng(n)
    tail = lambda k: np.clip(rng.lognormal(1.2, 0.9, k), 1, 60).astype(int).tolist()
    return {
        # skewed and small, empty pairs: the CSR kernel
        "csr": ([1, 0, 3, 17, 1, 64, 2, 0, 5], [1, 4, 0, 9, 33, 65, 2, 0, 1], {"ragged_flat": 1, "ragged_coop": 0}),
        # nearly uniform large products: the LDS-tiled kernel of the default dispatch
        "tiled": ([30, 28, 30, 29], [30, 30, 29, 30], {}),
        # a long tail of small pairs behind a few large ones: the cooperative kernel
        "coop": ([90, 1, 0, 7, 120] + tail(1500), [70, 1, 5, 9, 100] + tail(1500), {"ragged_flat": 1, "ragged_coop": 1}),
    }


def ragged_want(pairs):
    return np.concatenate([np_mul(a, b).ravel() for a, b in pairs if a.size and b.size])


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", ["csr", "tiled", "coop"])
def test_mul_ragged(hip, oracle, knobs, n, kind):
    t1s, t2s, kn = ragged_batches(n)[kind]
    for k, v in kn.items():
        knobs.set(k, v)
    L, R, offL, offR, pairs = ragged_operands(n, t1s, t2s, 21)
    want = ragged_want(pairs)
    a, b = next(p for p in pairs if p[0].size and p[1].size)
    assert np.array_equal(want[:a.shape[1] * b.shape[1] * a.shape[2]], oracle.mul(n, a.ravel(), b.ravel())[0])
    off_out = csr([x * y for x, y in zip(t1s, t2s)])
    total = int(off_out[-1])
    batch = len(t1s)

    def call(moved):
        out = Out(hip, want.size, "out" in moved)
        dl_, dr_ = place(hip, L, "L" in moved), place(hip, R, "R" in moved)
        assert hip.lib.csgn_mul_ragged(n, batch, dl_.data_ptr(), up(hip, offL).data_ptr(), dr_.data_ptr(),
                                       up(hip, offR).data_ptr(), out.ptr, up(hip, off_out).data_ptr(),
                                       max(t1s), max(t2s), total, hip.stream) == 0
        return (out.words(),)

    assert np.array_equal(same_for_every_pattern(["L", "R", "out"], call)[0], want)

    # the same batch through a plan object (csgn_mul_plan_ragged + csgn_mul_planned)
    def planned(moved):
        out = Out(hip, want.size, "out" in moved)
        dl_, dr_ = place(hip, L, "L" in moved), place(hip, R, "R" in moved)
        d_off = hip.empty_words(batch + 1)
        handle = hip.mul_plan()
        try:
            head = (C.c_uint64 * 4)()
            assert hip.lib.csgn_mul_plan_ragged(handle, batch, up(hip, offL).data_ptr(), up(hip, offR).data_ptr(),
                                                d_off.data_ptr(), C.byref(head), hip.stream) == 0
            assert int(head[0]) == total
            assert hip.lib.csgn_mul_planned(handle, n, dl_.data_ptr(), dr_.data_ptr(), out.ptr, hip.stream) == 0
            return out.words(), hip.download(d_off)
        finally:
            hip.lib.csgn_mul_plan_destroy(handle)

    got, got_off = same_for_every_pattern(["L", "R", "out"], planned)
    assert np.array_equal(got_off, off_out)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", ["ones", "mixed"])
def test_mul_ragged_async(hip, n, kind):
    """A batch of 1 x 1 pairs (the gated AND stream) and a mixed one (the CSR kernel), bound above the real size."""
    if kind == "ones":
        t1s = t2s = [1] * 3000
    else:
        rng = np.random.default_rng(n + 1)
        t1s, t2s = rng.integers(0, 9, 400).tolist(), rng.integers(0, 9, 400).tolist()
    L, R, offL, offR, pairs = ragged_operands(n, t1s, t2s, 31)
    want = ragged_want(pairs)
    off_want = csr([x * y for x, y in zip(t1s, t2s)])
    total, batch = int(off_want[-1]), len(t1s)
    cap = total + 5
    dl = (n + 63) // 64

    def call(moved):
        out = Out(hip, cap * dl, "out" in moved)
        dl_, dr_ = place(hip, L, "L" in moved), place(hip, R, "R" in moved)
        off_out = hip.empty_words(batch + 1)
        plan = hip.empty_words(int(hip.lib.csgn_mul_ragged_async_plan_words(batch)))
        assert hip.lib.csgn_mul_ragged_async(n, batch, dl_.data_ptr(), up(hip, offL).data_ptr(), dr_.data_ptr(),
                                             up(hip, offR).data_ptr(), out.ptr, off_out.data_ptr(), cap,
                                             plan.data_ptr(), hip.stream) == 0
        res = hip.mul_ragged_async_result(plan)
        assert res[0] == total and res[4] == 0, res
        words = out.words()
        assert (words[total * dl:] == np.uint64(GUARD)).all()          # nothing past the real end
        return words[:total * dl], hip.download(off_out)

    got, got_off = same_for_every_pattern(["L", "R", "out"], call)
    assert np.array_equal(got_off, off_want)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------ decrypt

def decrypt_call(hip, fn, scratch_bytes, batch, *ptrs):
    bits = torch.zeros(max(batch, 1), dtype=torch.uint8, device=hip.device)
    scratch = torch.empty(int(scratch_bytes), dtype=torch.uint8, device=hip.device)
    assert fn(*ptrs, bits.data_ptr(), scratch.data_ptr(), hip.stream) == 0
    return hip.download(bits)[:batch]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("loop", [0, 1])
def test_decrypt_uniform(hip, oracle, knobs, n, loop):
    """The segment form (dec_loop=0) and the looping form (dec_loop=1) of the term pass."""
    knobs.set("dec_loop", loop)
    key = make_key(n, KEY_D[n], 13)
    mask = oracle.key_mask(n, key)
    for terms in (1, 9, 300):
        batch = 3
        parts = [planted(oracle, n, key, terms, (5 * b + terms) % (terms + 1), 700 + b) for b in range(batch)]
        flat = np.concatenate(parts)
        want = np.array([oracle.decrypt_canonical(n, key, p) for p in parts], dtype=np.uint8)
        assert np.array_equal(want, [((5 * b + terms) % (terms + 1)) % 2 for b in range(batch)])

        def call(moved):
            return (decrypt_call(hip, hip.lib.csgn_decrypt_uniform, hip.lib.csgn_decrypt_scratch_bytes(batch, batch * terms),
                                 batch, n, batch, terms, place(hip, flat, "terms" in moved).data_ptr(),
                                 place(hip, mask, "mask" in moved).data_ptr()),)

        assert np.array_equal(same_for_every_pattern(["terms", "mask"], call)[0], want), terms


@pytest.mark.parametrize("n", NS)
def test_decrypt_ragged(hip, oracle, n):
    key = make_key(n, KEY_D[n], 4)
    mask = oracle.key_mask(n, key)
    counts = [1, 0, 3, 300, 64, 0, 65, 1]
    parts = [planted(oracle, n, key, t, t // 2 + (t % 3 == 0), 200 + i) if t else np.zeros(0, np.uint64)
             for i, t in enumerate(counts)]
    flat, off = np.concatenate(parts), csr(counts)
    want = np.array([oracle.decrypt_canonical(n, key, p) if p.size else 0 for p in parts], dtype=np.uint8)
    batch, total = len(counts), sum(counts)

    def call(moved):
        return (decrypt_call(hip, hip.lib.csgn_decrypt_ragged_bounded, hip.lib.csgn_decrypt_scratch_bytes(batch, total),
                             batch, n, batch, total, 0, place(hip, flat, "terms" in moved).data_ptr(),
                             up(hip, off).data_ptr(), place(hip, mask, "mask" in moved).data_ptr()),)

    assert np.array_equal(same_for_every_pattern(["terms", "mask"], call)[0], want)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("product", [True, False])
def test_decrypt_product_and_sum(hip, oracle, n, product):
    key = make_key(n, KEY_D[n], 5)
    mask = oracle.key_mask(n, key)
    batch, t1, t2 = 6, 3, 4
    L, R = rand_terms(n, batch, t1, 40), rand_terms(n, batch, t2, 41)
    L[:3, 0] |= mask                                            # some terms that hit the key
    R[1:4, 1] |= mask
    whole = np_mul(L, R) if product else np_add(L, R)
    want = np.array([oracle.decrypt_canonical(n, key, whole[e].ravel()) for e in range(batch)], dtype=np.uint8)
    fn = hip.lib.csgn_decrypt_product_uniform if product else hip.lib.csgn_decrypt_sum_uniform

    def call(moved):
        return (decrypt_call(hip, fn, hip.lib.csgn_decrypt_combined_scratch_bytes(batch, t1, t2), batch, n, batch, t1, t2,
                             place(hip, L, "L" in moved).data_ptr(), place(hip, R, "R" in moved).data_ptr(),
                             place(hip, mask, "mask" in moved).data_ptr()),)

    assert np.array_equal(same_for_every_pattern(["L", "R", "mask"], call)[0], want)


# ------------------------------------------------------------------------------ encrypt

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("lds", [0, 1])
def test_encrypt_explicit(hip, oracle, knobs, n, lds):
    """Reference ciphertexts (oracle.encrypt_seq over a glibc rand() stream) rebuilt from explicit randomness."""
    knobs.set("enc_lds", lds)
    d = KEY_D[n]
    key = make_key(n, d, 6)
    bits = np.array([1, 0, 0, 1, 0, 1, 1, 0, 0], dtype=np.uint8)
    draws = glibc_draws(50 + n, (n + 2) * len(bits))
    want = oracle.encrypt_seq(n, key, bits, draws)[0]
    dl = (n + 63) // 64
    rnd = np.zeros(len(bits) * dl, dtype=np.uint64)
    chosen, last = np.zeros(len(bits), np.uint32), np.zeros(len(bits), np.uint8)
    pos = 0
    for i, b in enumerate(bits):
        r, c, l, used = explicit_randomness(n, key, int(b), draws[pos:])
        rnd[i * dl:(i + 1) * dl], chosen[i], last[i] = r, c, l
        pos += used
    mask = oracle.key_mask(n, key)

    def call(moved):
        out = Out(hip, want.size, "out" in moved)
        assert hip.lib.csgn_encrypt_explicit(n, d, len(bits), up(hip, bits).data_ptr(),
                                             place(hip, rnd, "rnd" in moved).data_ptr(), up(hip, chosen).data_ptr(),
                                             up(hip, last).data_ptr(), place(hip, mask, "mask" in moved).data_ptr(),
                                             out.ptr, hip.stream) == 0
        return (out.words(),)

    assert np.array_equal(same_for_every_pattern(["rnd", "mask", "out"], call)[0], want)


@pytest.mark.parametrize("n", NS)
def test_encrypt_keyed_and_fused_chain(hip, oracle, n):
    """csgn_encrypt_keyed and csgn_encrypt_mul_keyed against the restated definition, a window of the stream that starts
    and ends inside a group."""
    d = KEY_D[n]
    key = make_key(n, d, 16)
    mask = oracle.key_mask(n, key)
    dkey = hip.upload(key)
    _, _, group = oracle.keyed_layout(n)
    first, batch = group - 1, group + 9
    prng = np.random.default_rng(n)
    pa, pb = prng.integers(0, 2, batch).astype(np.uint8), prng.integers(0, 2, batch).astype(np.uint8)
    ra, rb = hip.rng_from_seed(300 + n, 8), hip.rng_from_seed(301 + n, 8)
    (ka, na), (kb, nb) = oracle.rng_from_seed(300 + n), oracle.rng_from_seed(301 + n)
    wa = oracle.encrypt_keyed(n, key, pa, ka, na, 8, first_ciphertext=first)
    wb = oracle.encrypt_keyed(n, key, pb, kb, nb, 8, first_ciphertext=first)

    def keyed(moved):
        out = Out(hip, wa.size, "out" in moved)
        assert hip.lib.csgn_encrypt_keyed(n, d, batch, first, up(hip, pa).data_ptr(), dkey.data_ptr(),
                                          place(hip, mask, "mask" in moved).data_ptr(), C.byref(ra), out.ptr,
                                          hip.stream) == 0
        return (out.words(),)

    assert np.array_equal(same_for_every_pattern(["mask", "out"], keyed)[0], wa)

    def fused(moved):
        out = Out(hip, wa.size, "out" in moved)
        bits = torch.full((batch,), 7, dtype=torch.uint8, device=hip.device)
        assert hip.lib.csgn_encrypt_mul_keyed(n, d, batch, first, up(hip, pa).data_ptr(), up(hip, pb).data_ptr(),
                                              dkey.data_ptr(), place(hip, mask, "mask" in moved).data_ptr(),
                                              C.byref(ra), C.byref(rb), out.ptr, bits.data_ptr(), hip.stream) == 0
        return out.words(), hip.download(bits)

    got, bits = same_for_every_pattern(["mask", "out"], fused)
    assert np.array_equal(got, wa & wb)
    want_bits = np.array([oracle.decrypt_canonical(n, key, (wa & wb)[e * ((n + 63) // 64):(e + 1) * ((n + 63) // 64)])
                          for e in range(batch)], dtype=np.uint8)
    assert np.array_equal(bits, want_bits)
    assert np.array_equal(want_bits, pa & pb)


# ------------------------------------------------------------------------------ compaction

def dup_ciphertext(oracle, rng, n, seed, pool, draws):
    dl = (n + 63) // 64
    if draws == 0:
        return np.zeros(0, dtype=np.uint64)
    base = oracle.synth(seed, n, 0, pool * dl).reshape(pool, dl)
    return np.ascontiguousarray(base[rng.integers(0, pool, size=draws)].reshape(-1))


def compaction_batches(oracle, n):
    rng = np.random.default_rng(n + 3)
    one_group = [dup_ciphertext(oracle, rng, n, 10 + i, p, t) for i, (p, t) in
                 enumerate([(1, 2), (1, 3), (5, 40), (300, 200), (0, 0), (64, 64), (7, 1)])]
    sizes = [1100, 1792, 3, 1500, 0, 1025, 700] if n != 4096 else [766, 321, 768, 5, 500]
    wide = [dup_ciphertext(oracle, rng, n, 40 + i, max(1, int(t * f)), t) for i, (t, f) in
            enumerate(zip(sizes, [1.5, 0.5, 1.0, 0.03, 1.0, 2.0, 0.3]))]
    partition = [dup_ciphertext(oracle, rng, n, 60, 5, 9), dup_ciphertext(oracle, rng, n, 61, 4000, 3000),
                 np.zeros(0, dtype=np.uint64), dup_ciphertext(oracle, rng, n, 62, 300, 5000),
                 dup_ciphertext(oracle, rng, n, 63, 2000, 2049)]
    return {"one_group": (one_group, 0), "wide": (wide, max(sizes)), "partition": (partition, 0)}


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", ["one_group", "wide", "partition"])
def test_compact_ragged(hip, oracle, n, kind):
    cts, max_terms = compaction_batches(oracle, n)[kind]
    dl = (n + 63) // 64
    off = csr([c.size // dl for c in cts])
    flat = np.concatenate(cts)
    total, batch = int(off[-1]), len(cts)
    wants = [oracle.compact(n, c) for c in cts]
    want = np.concatenate(wants)
    want_off = csr([w.size // dl for w in wants])

    def call(moved):
        out = Out(hip, total * dl, "out" in moved)
        off_out = hip.empty_words(batch + 1)
        scratch = hip.empty_words((int(hip.lib.csgn_compact_scratch_bytes(n, batch, total)) + 7) // 8)
        assert hip.lib.csgn_compact_ragged(n, batch, total, max_terms, place(hip, flat, "terms" in moved).data_ptr(),
                                           up(hip, off).data_ptr(), out.ptr, off_out.data_ptr(), scratch.data_ptr(),
                                           hip.stream) == 0
        got_off = hip.download(off_out)
        return out.words(int(got_off[-1]) * dl), got_off

    got, got_off = same_for_every_pattern(["terms", "out"], call)
    assert np.array_equal(got_off, want_off)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------ constants, gates, integers

@pytest.mark.parametrize("n", NS)
def test_const_fill(hip, n):
    batch = 333
    plain = np.random.default_rng(n).integers(0, 256, batch).astype(np.uint8)
    want = np.stack([const_term(n, p & 1) for p in plain]).ravel()

    def call(moved):
        out = Out(hip, want.size, "out" in moved)
        assert hip.lib.csgn_const_fill(n, batch, up(hip, plain).data_ptr(), 1, out.ptr, hip.stream) == 0
        return (out.words(),)

    assert np.array_equal(same_for_every_pattern(["out"], call)[0], want)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("fused", [0, 1])
def test_gate_uniform(hip, knobs, n, fused):
    """gate_fused=1: the fused kernel; 0: every segment by the pitched add / multiply / constant launches."""
    knobs.set("gate_fused", fused)
    ts, ta, tb, batch = 2, 3, 2, 5
    a, b, s = rand_terms(n, batch, ta, 71), rand_terms(n, batch, tb, 72), rand_terms(n, batch, ts, 73)
    plain = np.random.default_rng(74).integers(0, 2, batch).astype(np.uint8)
    for gate in sorted(GATES.values()):
        want = np_gate(n, gate, a, b, s, plain).ravel()
        assert want.size == batch * gate_terms(gate, ts, ta, tb) * ((n + 63) // 64)

        def call(moved):
            out = Out(hip, want.size, "out" in moved)
            assert hip.lib.csgn_gate_uniform(n, gate, batch, ts, ta, tb, place(hip, s, "sel" in moved).data_ptr(),
                                             place(hip, a, "a" in moved).data_ptr(), place(hip, b, "b" in moved).data_ptr(),
                                             up(hip, plain).data_ptr(), out.ptr, hip.stream) == 0
            return (out.words(),)

        assert np.array_equal(same_for_every_pattern(["sel", "a", "b", "out"], call)[0], want), gate


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("fused", [0, 1])
def test_uint_step(hip, knobs, n, fused):
    knobs.set("uint_fused", fused)
    tx, ta, tb, batch = 3, 1, 2, 5
    x, a, b = rand_terms(n, batch, tx, 81), rand_terms(n, batch, ta, 82), rand_terms(n, batch, tb, 83)
    for step in sorted(STEPS.values()):
        want = [w.ravel() for w in np_step(n, step, x, a, b)]
        carry = step in (ADD_HALF, ADD_FULL)
        reads_x = step not in (ADD_HALF, STEPS["lt_first"])
        names = (["x"] if reads_x else []) + ["a", "b", "out0"] + (["out1"] if carry else [])

        def call(moved):
            o0 = Out(hip, want[0].size, "out0" in moved)
            o1 = Out(hip, want[1].size, "out1" in moved) if carry else None
            dx = place(hip, x, "x" in moved).data_ptr() if reads_x else None
            assert hip.lib.csgn_uint_step(n, step, batch, dx, tx if reads_x else 0, place(hip, a, "a" in moved).data_ptr(),
                                          ta, place(hip, b, "b" in moved).data_ptr(), tb, o0.ptr,
                                          o1.ptr if carry else None, hip.stream) == 0
            return (o0.words(),) + ((o1.words(),) if carry else ())

        got = same_for_every_pattern(names, call)
        assert len(got) == len(want)
        for o in range(len(want)):
            assert np.array_equal(got[o], want[o]), (step, o)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("fused", [0, 1])
def test_uint_plain(hip, knobs, n, fused):
    knobs.set("uint_plain_fused", fused)
    ts, batch = [1, 2, 1, 1], 3
    planes = [rand_terms(n, batch, t, 90 + j) for j, t in enumerate(ts)]
    names = ["p0", "p1", "p2", "p3", "out"]
    for cmp, k in ((EQ, 5), (NE, 0), (LT, 9), (LE, 12), (GT, 3), (GE, 6), (LT, 0), (GT, 15)):
        want = np_plain(n, cmp, planes, k).ravel()

        def call(moved):
            out = Out(hip, want.size, "out" in moved)
            dev = [place(hip, p, f"p{j}" in moved) for j, p in enumerate(planes)]
            ptrs = (C.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
            assert hip.lib.csgn_uint_plain(n, cmp, batch, len(ts), k, ptrs, u64s(ts), out.ptr, hip.stream) == 0
            return (out.words(),)

        assert np.array_equal(same_for_every_pattern(names, call)[0], want), (cmp, k)
