"""Operands and results that are 8-byte but not 16-byte aligned, at even word counts.

Every device entry point compiles its kernels for 16-byte units and for 8-byte units, and the host side takes the wide
form only when dL = ceil(N / 64) is even AND every pointer is 16-byte aligned.  The C ABI promises only uint64_t
alignment, so a caller's arena, a torch view at an odd word offset or a pinned buffer behind a header run the 8-byte form
at N = 1247 or 4096 -- with unit counts (U = 20, 64) and trip counts the rest of the suite, whose buffers are fresh
allocations, never gives it.  Here each pointer argument is moved one word into its buffer, alone and then all of them,
and the words (and bits) must equal the numpy or oracle definition AND the same call on aligned buffers.  N = 1300 (odd
dL, the 8-byte form either way) is the control.  Outputs carry a guard word on either side.  Run with `pytest -m gpu`.

What is covered, entry point by entry point:
  add (uniform, ragged), multiply (uniform in every form, ragged, planned, async), decrypt (uniform, ragged, product and
  sum), encrypt (explicit, keyed, the fused chain), compaction, constants, gates, the integer steps and csgn_uint_plain:
  every pointer alone and all of them, at every N of NS;
  csgn_uint_lut_apply, csgn_gather (uniform and ragged), csgn_gather_planes, csgn_uint_read, csgn_uint_find,
  csgn_uint_lt_select, csgn_uint_pick and csgn_uint_write, whose arguments are ARRAYS of device pointers: every pointer
  class alone, the middle member of every class alone (one plane of many off a 16-byte boundary must already take the
  8-byte form), and all of them, at every N of NS, in the fused and in the composed form (and the ragged gather at 1
  and 4 chunks a workgroup), over fresh planes (subset tables in LDS) and planes of 1..3 terms (no tables);
  the same entry points where a term is cut into unit slices at an even word count (N = 8320 and 5185), KC asserted from
  csgn_uint_pick_plan and csgn_uint_write_plan;
  and their later launches (knob launch_blocks) at moved pointers, whose per-launch offsets then count 8-byte units.
csgn_uint_addk, csgn_matmul and csgn_count keep their one unaligned case each in their own files."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import (ADD_FULL, ADD_HALF, EQ, GATES, GE, GT, LE, LT, NE, STEPS, c_terms, const_term, csr,
                         explicit_randomness, gate_terms, hip, make_key, np_add, np_gate, np_gather, np_gather_offsets,
                         np_gather_uniform, np_lut, np_mul, np_plain, np_read_fast, np_step, planted, rand_terms,
                         random_table, tile_index, u64s)
from tests.model_find import np_find_fast
from tests.model_lt_select import minmax_requests, np_lt_select_fast
from tests.model_pick import EACH, OPS, np_pick_fast
from tests.model_write import np_write_fast

pytestmark = pytest.mark.gpu

NS = [1247, 4096, 128, 1300]                # even dL (20, 64, 2) and one odd (21)
KEY_D = {1247: 16, 4096: 32, 128: 8, 1300: 4}
GUARD = 0x5A5A5A5A5A5A5A5A


def member(cls, i):
    """The name of pointer i of the class `cls` moved alone."""
    return "%s[%d]" % (cls, i)


def patterns(names, counts=None):
    """No pointer moved (the reference call), each one alone, then all of them.  Where the arguments are arrays of
    device pointers the names are the pointer classes and counts[name] is the number of pointers in the class: every
    class of two or more also gives its middle member moved alone ("table[1]"), after the classes."""
    names = list(names)
    lone = [member(x, counts[x] // 2) for x in names if counts and counts.get(x, 1) >= 2]
    return [frozenset()] + [frozenset([x]) for x in names + lone] + ([frozenset(names)] if len(names) > 1 else [])


def is_moved(moved, cls, i):
    return cls in moved or member(cls, i) in moved


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


def place_all(hip, arrays, moved, cls):
    """The pointers of one class, each placed as the pattern says."""
    return [place(hip, a, is_moved(moved, cls, i)) for i, a in enumerate(arrays)]


def outs_for(hip, want, moved, cls):
    """One guarded output per wanted array, each placed as the pattern says."""
    return [Out(hip, np.asarray(w).size, is_moved(moved, cls, i)) for i, w in enumerate(want)]


def same_for_every_pattern(names, call, counts=None, only=None):
    """call(moved) -> tuple of arrays; all patterns (`only`: these, the aligned call first) give the words of the aligned
    call, which is returned."""
    base = None
    for moved in only or patterns(names, counts):
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


# ------------------------------------------------------------------------------ arrays of device pointers

# One operation on fixed operands: the pointer classes, the pointers in each, call(moved) and the definition's words.
Case = namedtuple("Case", "names counts call want")


def terms_of(planes):
    return [p.shape[1] for p in planes]


def ends(names):
    """No pointer moved, then all of them."""
    return [frozenset(), frozenset(names)]


def check_case(case, only=None):
    """Every pattern gives the aligned call's words, and those are the definition's."""
    got = same_for_every_pattern(case.names, case.call, case.counts, only)
    assert len(got) == len(case.want)
    for j, (g, w) in enumerate(zip(got, case.want)):
        assert np.array_equal(g, np.asarray(w).ravel()), j


def words_of(outs):
    return tuple(o.words() for o in outs)


def views(outs):
    return [o.view for o in outs]


def lut_case(hip, n, batch, handle, table, m, ts, seed):
    planes = [rand_terms(n, batch, t, seed + 7 * i + t) for i, t in enumerate(ts)]
    want = np_lut(n, planes, table, m)
    rc, T = c_terms(hip.lib, table, len(ts), m, ts)
    assert rc == 0 and terms_of(want) == T

    def call(moved):
        outs = outs_for(hip, want, moved, "out")
        hip.uint_lut_apply(handle, n, batch, place_all(hip, planes, moved, "planes"), T, outs=views(outs))
        return words_of(outs)

    return Case(["planes", "out"], {"planes": len(ts), "out": m}, call, want)


def gather_planes_case(hip, n, terms, count_in, count_out, idx, seed):
    dl = (n + 63) // 64
    planes = [rand_terms(n, count_in, t, seed + j).ravel() for j, t in enumerate(terms)]
    ref = idx if idx is not None else tile_index(count_in, count_out)
    want = [np_gather_uniform(p, t, ref, dl) for p, t in zip(planes, terms)]

    def call(moved):
        outs = outs_for(hip, want, moved, "out")
        hip.gather_planes(n, place_all(hip, planes, moved, "src"), terms, count_in, count_out,
                          up(hip, idx) if idx is not None else None, views(outs))
        return words_of(outs)

    return Case(["src", "out"], {"src": len(terms), "out": len(terms)}, call, want)


def read_case(hip, n, batch, s, rows, t, seed):
    index = [rand_terms(n, batch, sk, seed + 7 * k + sk) for k, sk in enumerate(s)]
    table = [rand_terms(n, rows, tj, seed + 100 + 11 * j + rows) for j, tj in enumerate(t)]
    want = np_read_fast(n, index, table)

    def call(moved):
        outs = outs_for(hip, want, moved, "out")
        hip.uint_read(n, batch, place_all(hip, index, moved, "index"), s, rows, place_all(hip, table, moved, "table"), t,
                      outs=views(outs))
        return words_of(outs)

    return Case(["index", "table", "out"], {"index": len(s), "table": len(t), "out": len(t)}, call, want)


def find_case(hip, n, batch, u, s, rows, t, seed):
    """With the member bit: the last output."""
    keys = [rand_terms(n, rows, uk, seed + 5 * k + rows) for k, uk in enumerate(u)]
    query = [rand_terms(n, batch, sk, seed + 50 + 7 * k + sk) for k, sk in enumerate(s)]
    values = [rand_terms(n, rows, tj, seed + 100 + 11 * j) for j, tj in enumerate(t)]
    outs, mem = np_find_fast(n, keys, query, values, True)
    want = list(outs) + [mem]
    w = len(t)

    def call(moved):
        outs = outs_for(hip, want[:w], moved, "out")
        mem = Out(hip, want[w].size, "member" in moved)
        hip.uint_find(n, batch, place_all(hip, query, moved, "query"), s, rows, place_all(hip, keys, moved, "keys"), u,
                      place_all(hip, values, moved, "values"), t, outs=views(outs), member=mem.view)
        return words_of(outs + [mem])

    return Case(["query", "keys", "values", "out", "member"], {"query": len(s), "keys": len(u), "values": w, "out": w},
                call, want)


def lt_select_case(hip, n, batch, ta, tb, seed):
    """min and max of a and b (request i of min is a_i : b_i, of max b_i : a_i) and the comparison, the last output."""
    w = len(ta)
    host = ([rand_terms(n, batch, t, seed + 7 * k + t) for k, t in enumerate(ta)] +
            [rand_terms(n, batch, t, seed + 50 + 5 * k + t) for k, t in enumerate(tb)])
    xi, yi = minmax_requests(list(range(w)), list(range(w, 2 * w)))              # planes named by index into host
    outs, lt = np_lt_select_fast(n, host[:w], host[w:], [host[h] for h in xi], [host[h] for h in yi], True)
    want = list(outs) + [lt]
    m = len(xi)

    def call(moved):
        placed = {}

        def dev(cls, i, h):
            # one device copy per (plane, moved or not): a request plane that is placed as the operand it names is
            # handed over as the very same pointer (X_i = a_j), else as a copy of it
            key = (h, is_moved(moved, cls, i))
            if key not in placed:
                placed[key] = place(hip, host[h], key[1])
            return placed[key]

        da, db = [dev("a", j, j) for j in range(w)], [dev("b", j, w + j) for j in range(w)]
        dx, dy = [dev("x", i, h) for i, h in enumerate(xi)], [dev("y", i, h) for i, h in enumerate(yi)]
        outs = outs_for(hip, want[:m], moved, "out")
        less = Out(hip, want[m].size, "less" in moved)
        hip.uint_lt_select(n, batch, da, ta, db, tb, dx, [host[h].shape[1] for h in xi], dy,
                           [host[h].shape[1] for h in yi], outs=views(outs), less=less.view)
        return words_of(outs + [less])

    return Case(["a", "b", "x", "y", "out", "less"], {"a": w, "b": w, "x": m, "y": m, "out": m}, call, want)


def pick_case(hip, n, batch, op, s, w, rows, t, seed):
    index = [rand_terms(n, batch, sk, seed + 7 * k + sk) for k, sk in enumerate(s)]
    src = [rand_terms(n, batch * (rows if op == EACH else 1), t, seed + 100 + 11 * j) for j in range(w)]
    want = np_pick_fast(n, op, index, src, rows)

    def call(moved):
        outs = outs_for(hip, want, moved, "out")
        hip.uint_pick(n, op, batch, place_all(hip, index, moved, "index"), s, place_all(hip, src, moved, "src"), t, rows,
                      outs=views(outs))
        return words_of(outs)

    return Case(["index", "src", "out"], {"index": len(s), "src": w, "out": w}, call, want)


def write_case(hip, n, batch, s, rows, tv, td, seed):
    index = [rand_terms(n, batch, sk, seed + 7 * k + sk) for k, sk in enumerate(s)]
    value = [rand_terms(n, batch, t, seed + 100 + 11 * j) for j, t in enumerate(tv)]
    arrays = [rand_terms(n, batch * rows, t, seed + 500 + 13 * j) for j, t in enumerate(td)]
    want = np_write_fast(n, index, value, arrays, rows)

    def call(moved):
        outs = outs_for(hip, want, moved, "out")
        hip.uint_write(n, batch, place_all(hip, index, moved, "index"), s, rows, place_all(hip, value, moved, "value"), tv,
                       place_all(hip, arrays, moved, "arrays"), td, outs=views(outs))
        return words_of(outs)

    w = len(tv)
    return Case(["index", "value", "arrays", "out"], {"index": len(s), "value": w, "arrays": w, "out": w}, call, want)


# -- the forms: the knob set and the form it selects asserted by the entry point's name function -----------------------
def lut_form(hip, knobs, fused, n, batch, handle):
    knobs.set("uint_lut_fused", fused)
    assert hip.lib.csgn_uint_lut_kernel(n, handle, batch) == (b"k_uint_lut" if fused else b"composed")


def read_form(hip, knobs, fused, n, batch, s, rows, t):
    knobs.set("uint_read_fused", fused)
    name = hip.lib.csgn_uint_read_kernel(n, batch, len(s), u64s(s), rows, len(t), u64s(t))
    assert name == (b"k_uint_read" if fused else b"composed")


def find_form(hip, knobs, fused, n, batch, u, s, rows, t):
    knobs.set("uint_find_form", fused)
    name = hip.lib.csgn_uint_find_kernel(n, batch, len(u), u64s(u), u64s(s), rows, len(t), u64s(t), 1)
    assert name == (b"k_uint_find" if fused else b"composed")


def lt_select_form(hip, knobs, fused, n, batch, ta, tb):
    knobs.set("uint_lt_select_form", fused)
    tx, ty = minmax_requests(ta, tb)
    name = hip.lib.csgn_uint_lt_select_kernel(n, batch, len(ta), u64s(ta), u64s(tb), len(tx), u64s(tx), u64s(ty), 1)
    assert name == (b"k_uint_lt_select" if fused else b"composed")


def pick_forms(hip, knobs, n, batch, op, s, w, rows, t, forms=(0, 1)):
    """Sets the form, then every staging of it, in turn: composed; the fused kernel without and with its LDS value slice."""
    for fused in forms:
        knobs.set("uint_pick_fused", fused)
        name = hip.lib.csgn_uint_pick_kernel(n, op, batch, len(s), u64s(s), w, rows, t)
        assert name == (b"k_uint_pick" if fused else b"composed")
        for stage in ((0, 1) if fused else (-1,)):
            knobs.set("uint_pick_stage", stage)
            yield fused, stage


def write_form(hip, knobs, fused, n, batch, s, rows, tv, td):
    knobs.set("uint_write_fused", fused)
    name = hip.lib.csgn_uint_write_kernel(n, batch, len(s), u64s(s), rows, len(tv), u64s(tv), u64s(td))
    assert name == (b"k_uint_write" if fused else b"composed")


BATCH = 3
LUT_TABLE = [(3 * x) % 16 for x in range(16)]
MIXED = {2: [2, 1], 3: [2, 1, 3]}                                       # index planes of 1..3 terms: no subset tables
GATHER_INDEX = np.array([6, 0, 0, 3, 3, 3, 1, 6, 4, 0, 6], dtype=np.uint64)    # 11 of 7 elements: repeats, 2 and 5 skipped


@pytest.mark.parametrize("n", NS)
def test_uint_lut_pointer_arrays(hip, knobs, n):
    """One handle per term list, applied at every pattern and in both forms: a handle does not remember a unit width."""
    shapes = [(4, LUT_TABLE, [1, 1, 1, 1]), (4, LUT_TABLE, [1, 2, 1, 1])]
    if n == 1247:
        shapes.append((6, random_table(6, 4, 61), [1] * 6))              # two subset tables
    for w, table, ts in shapes:
        handle = hip.uint_lut_create(table, w, 4, ts)
        try:
            case = lut_case(hip, n, BATCH, handle, table, 4, ts, 2000)
            for fused in (0, 1):
                lut_form(hip, knobs, fused, n, BATCH, handle)
                check_case(case)
        finally:
            torch.cuda.synchronize()
            hip.lib.csgn_uint_lut_destroy(handle)


@pytest.mark.parametrize("n", NS)
def test_gather_uniform_pointers(hip, n):
    """t = 3, 7 source elements, 11 output elements: by an index list that repeats and skips, and the tile form."""
    t, count_in, count_out = 3, 7, len(GATHER_INDEX)
    dl = (n + 63) // 64
    src = rand_terms(n, count_in, t, 2100).ravel()
    assert hip.lib.csgn_gather_kernel(n, count_out, 0, 1) == b"k_gather"
    for idx in (GATHER_INDEX, None):
        want = np_gather_uniform(src, t, idx if idx is not None else tile_index(count_in, count_out), dl)

        def call(moved):
            out = Out(hip, want.size, "out" in moved)
            d_idx = place(hip, idx, "index" in moved) if idx is not None else None
            hip.gather(n, count_in, place(hip, src, "src" in moved), t, count_out, d_idx, out.view)
            return (out.words(),)

        names = ["src", "index", "out"] if idx is not None else ["src", "out"]
        assert np.array_equal(same_for_every_pattern(names, call)[0], want), idx is None


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("chunks", [1, 4])
def test_gather_ragged_pointers(hip, knobs, n, chunks):
    """Knob ragged_c: 1 and 4 chunks a workgroup.  The plan writes the output offsets, themselves between guard words."""
    knobs.set("ragged_c", chunks)
    sizes = [1, 0, 3, 17, 2, 0, 40]
    idx = np.array([3, 0, 6, 6, 1, 2, 4, 3, 0, 5, 6], dtype=np.uint64)
    count_in, count_out = len(sizes), len(idx)
    dl = (n + 63) // 64
    src_off = csr(sizes)
    src = rand_terms(n, 1, sum(sizes), 2200).ravel()
    want, want_off = np_gather(src, src_off, idx, dl)
    assert np.array_equal(want_off, np_gather_offsets(src_off, idx))
    total = int(want_off[-1])
    assert hip.lib.csgn_gather_kernel(n, count_out, 1, 1) == b"k_gather_ragged"

    def call(moved):
        d_src, d_soff = place(hip, src, "src" in moved), place(hip, src_off, "src_off" in moved)
        d_idx = place(hip, idx, "index" in moved)
        out, out_off = Out(hip, want.size, "out" in moved), Out(hip, count_out + 1, "out_off" in moved)
        res = (C.c_uint64 * 2)()
        assert hip.lib.csgn_gather_plan(count_in, d_soff.data_ptr(), count_out, d_idx.data_ptr(), out_off.ptr, res,
                                        hip.stream) == 0
        assert (int(res[0]), int(res[1])) == (total, 0)
        assert hip.lib.csgn_gather(n, count_in, d_src.data_ptr(), d_soff.data_ptr(), 0, count_out, d_idx.data_ptr(),
                                   out.ptr, out_off.ptr, total, hip.stream) == 0
        return out.words(), out_off.words()

    got, got_off = same_for_every_pattern(["src", "src_off", "index", "out", "out_off"], call)
    assert np.array_equal(got_off, want_off)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", NS)
def test_gather_planes_pointer_arrays(hip, n):
    assert hip.lib.csgn_gather_kernel(n, len(GATHER_INDEX), 0, 3) == b"k_gather"
    for idx in (GATHER_INDEX, None):
        check_case(gather_planes_case(hip, n, [1, 2, 3], 7, len(GATHER_INDEX), idx, 2300))


@pytest.mark.parametrize("n", NS)
def test_uint_read_pointer_arrays(hip, knobs, n):
    shapes = [(s, rows, [1, 2]) for s in ([1, 1, 1], MIXED[3]) for rows in (5, 8)]
    if n == 1247:
        shapes.append(([1] * 6, 64, [1]))                                # two subset tables
    for s, rows, t in shapes:
        case = read_case(hip, n, BATCH, s, rows, t, 2400)
        for fused in (0, 1):
            read_form(hip, knobs, fused, n, BATCH, s, rows, t)
            check_case(case)


@pytest.mark.parametrize("n", NS)
def test_uint_find_pointer_arrays(hip, knobs, n):
    """Key width 3, 5 rows, two value planes and the member bit; fresh keys and query, then planes of 1..3 terms."""
    for u, s in (([1, 1, 1], [1, 1, 1]), ([1, 2, 1], MIXED[3])):
        case = find_case(hip, n, BATCH, u, s, 5, [1, 2], 2500)
        for fused in (0, 1):
            find_form(hip, knobs, fused, n, BATCH, u, s, 5, [1, 2])
            check_case(case)


@pytest.mark.parametrize("n", NS)
def test_uint_lt_select_pointer_arrays(hip, knobs, n):
    """Width 3, min and max of a and b, and the comparison; fresh operands, then planes of 1..3 terms."""
    for ta, tb in (([1, 1, 1], [1, 1, 1]), ([1, 2, 1], MIXED[3])):
        case = lt_select_case(hip, n, BATCH, ta, tb, 2600)
        for fused in (0, 1):
            lt_select_form(hip, knobs, fused, n, BATCH, ta, tb)
            check_case(case)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("op", sorted(OPS))
def test_uint_pick_pointer_arrays(hip, knobs, n, op):
    """The shifts and rotates at w = 4, v = 2; EACH at v = 3, 5 rows, w = 2.  Source planes of 1 and 2 terms."""
    op = OPS[op]
    v, w, rows = (3, 2, 5) if op == EACH else (2, 4, 0)
    for s in ([1] * v, MIXED[v]):
        for t in (1, 2):
            case = pick_case(hip, n, BATCH, op, s, w, rows, t, 2700)
            for _ in pick_forms(hip, knobs, n, BATCH, op, s, w, rows, t):
                check_case(case)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("v,rows,w", [(2, 3, 3), (3, 5, 2)])
def test_uint_write_pointer_arrays(hip, knobs, n, v, rows, w):
    for s in ([1] * v, MIXED[v]):
        for a, b in ((1, 1), (2, 3)):
            tv, td = [a] * w, [b] * w
            case = write_case(hip, n, BATCH, s, rows, tv, td, 2800)
            for fused in (0, 1):
                write_form(hip, knobs, fused, n, BATCH, s, rows, tv, td)
                check_case(case)


# ------------------------------------------------------------------------------ terms cut into unit slices, even dL

SLICED_N = 8320             # dL = 130


def test_unit_slices_at_an_even_word_count_cover_both_unit_sizes(hip):
    """What N = 8320 with five fresh selector planes is chosen for, from the fused forms' own tiles (csgn_uint_pick_plan,
    csgn_uint_write_plan): one element's subset table at whole terms, 32 entries x 130 words x 8 B = 33 280 B, passes the
    32 768 bytes a workgroup has for it, so a term is cut into two slices -- in 16-byte units (no pointer moved) 33 + 32
    of 65, a short last slice, and in 8-byte units (a pointer moved) 65 + 65 of 130, which no other N of the suite gives
    the 8-byte kernels (N = 8256: 65 + 64 of 129)."""
    v, rows, dl = 5, 32, (SLICED_N + 63) // 64
    s, one = u64s([1] * v), u64s([1])
    plan = (C.c_uint64 * 4)()
    seen = set()
    for wide, unit_bytes, want_kc in ((0, 8, 65), (1, 16, 33)):
        units = dl * 8 // unit_bytes
        assert (1 << v) * units * unit_bytes > 32768                   # at whole terms the table does not fit
        for what in ("pick", "write"):
            if what == "pick":
                rc = hip.lib.csgn_uint_pick_plan(SLICED_N, EACH, 2, v, s, 1, rows, 1, wide, plan)
            else:
                rc = hip.lib.csgn_uint_write_plan(SLICED_N, 2, v, s, rows, 1, one, one, wide, plan)
            assert rc == 0 and int(plan[1]) == want_kc, (what, wide, list(plan))
        assert (1 << v) * want_kc * unit_bytes <= 32768 and want_kc < units <= 2 * want_kc
        seen.add(("8-byte units, " if not wide else "16-byte units, ") +
                 ("two even slices" if units == 2 * want_kc else "a short last slice"))
    assert seen == {"8-byte units, two even slices", "16-byte units, a short last slice"}, seen


@pytest.mark.parametrize("entry", ["read", "pick", "write", "lut"])
def test_unit_slices_at_an_even_word_count(hip, knobs, entry):
    """N = 8320, five fresh selector planes, the fused form, no pointer moved and all of them (the slices:
    test_unit_slices_at_an_even_word_count_cover_both_unit_sizes).  32 rows, one plane of one term."""
    n, batch, s, rows = SLICED_N, 2, [1] * 5, 32
    if entry == "read":
        read_form(hip, knobs, 1, n, batch, s, rows, [1])
        case = read_case(hip, n, batch, s, rows, [1], 3000)
        check_case(case, ends(case.names))
    elif entry == "pick":
        case = pick_case(hip, n, batch, EACH, s, 1, rows, 1, 3100)
        for _ in pick_forms(hip, knobs, n, batch, EACH, s, 1, rows, 1, forms=(1,)):
            check_case(case, ends(case.names))
    elif entry == "write":
        write_form(hip, knobs, 1, n, batch, s, rows, [1], [1])
        case = write_case(hip, n, batch, s, rows, [1], [1], 3200)
        check_case(case, ends(case.names))
    else:
        table = random_table(5, 4, 33)
        handle = hip.uint_lut_create(table, 5, 4, s)
        try:
            lut_form(hip, knobs, 1, n, batch, handle)
            case = lut_case(hip, n, batch, handle, table, 4, s, 3300)
            check_case(case, ends(case.names))
        finally:
            torch.cuda.synchronize()
            hip.lib.csgn_uint_lut_destroy(handle)


@pytest.mark.parametrize("entry", ["find", "lt_select"])
def test_two_table_sets_cut_into_unit_slices_at_an_even_word_count(hip, knobs, entry):
    """csgn_uint_find and csgn_uint_lt_select hold two sets of subset tables and give each 20 480 bytes (kTableBudget);
    subset_plan cuts a term into slices when one element's tables at whole terms, entries x unit bytes x U, pass that.
    Five fresh planes are one table of 32 entries, and U units of a term are dL words of 8 bytes in either unit size
    (U = dL units of 8 bytes, or dL / 2 of 16), so the tables take 32 x 8 x dL = 256 dL bytes: past 20 480 from dL = 81
    on, and the smallest even dL is 82 -- N = 5185, the smallest N of 82 words, whose last word holds ONE bit, so ONE's
    last unit differs from every other in both unit sizes.  The slices are 41 + 41 units of 8 bytes (a pointer moved) or
    21 + 20 of 16 (none moved); the odd neighbour N = 5184 of the entry points' own files gives 41 + 40."""
    dl = next(d for d in range(2, 1000, 2) if 32 * 8 * d > 20480)
    n = 64 * (dl - 1) + 1
    assert (dl, n) == (82, 5185) and (n + 63) // 64 == dl and 32 * 8 * (dl - 2) <= 20480
    batch, one = 2, [1] * 5
    if entry == "find":
        find_form(hip, knobs, 1, n, batch, one, one, 3, [1, 2])
        case = find_case(hip, n, batch, one, one, 3, [1, 2], 3400)
    else:
        lt_select_form(hip, knobs, 1, n, batch, one, one)
        case = lt_select_case(hip, n, batch, one, one, 3500)
    check_case(case, ends(case.names))


# ------------------------------------------------------------------------------ later launches at moved pointers

def later_launch_runs(hip, knobs, entry, n, batch, handles):
    """(case, forms) pairs of one entry point at the small shapes above, fresh planes and planes of 1..3 terms: forms()
    sets the fused form's knobs and yields once per variant of it to run.  A lookup table's handle goes to `handles`."""
    def once(form, *args):
        return lambda: [form(hip, knobs, 1, n, batch, *args)]

    if entry == "read":
        return [(read_case(hip, n, batch, s, 5, [1, 2], 4000), once(read_form, s, 5, [1, 2])) for s in ([1, 1, 1], MIXED[3])]
    if entry == "find":
        return [(find_case(hip, n, batch, u, s, 5, [1, 2], 4100), once(find_form, u, s, 5, [1, 2]))
                for u, s in (([1, 1, 1], [1, 1, 1]), ([1, 2, 1], MIXED[3]))]
    if entry == "lt_select":
        return [(lt_select_case(hip, n, batch, ta, tb, 4200), once(lt_select_form, ta, tb))
                for ta, tb in (([1, 1, 1], [1, 1, 1]), ([1, 2, 1], MIXED[3]))]
    if entry == "pick":
        return [(pick_case(hip, n, batch, EACH, s, 2, 5, t, 4300),
                 lambda s=s, t=t: pick_forms(hip, knobs, n, batch, EACH, s, 2, 5, t, forms=(1,)))
                for s, t in (([1, 1, 1], 1), (MIXED[3], 2))]
    if entry == "write":
        return [(write_case(hip, n, batch, s, 5, [a] * 2, [b] * 2, 4400), once(write_form, s, 5, [a] * 2, [b] * 2))
                for s, a, b in (([1, 1, 1], 1, 1), (MIXED[3], 2, 3))]
    if entry == "lut":
        runs = []
        for ts in ([1, 1, 1, 1], [1, 2, 1, 1]):
            handles.append(hip.uint_lut_create(LUT_TABLE, 4, 4, ts))
            runs.append((lut_case(hip, n, batch, handles[-1], LUT_TABLE, 4, ts, 4600), once(lut_form, handles[-1])))
        return runs
    idx = np.random.default_rng(45).integers(0, 7, batch).astype(np.uint64)
    return [(gather_planes_case(hip, n, [1, 2, 3], 7, batch, i, 4500), lambda: [None]) for i in (idx, None)]


@pytest.mark.parametrize("entry", ["read", "find", "lt_select", "pick", "write", "lut", "gather_planes"])
def test_later_launches_at_moved_pointers(hip, knobs, entry):
    """N = 1247, 37 elements, the fused forms, no pointer moved and all of them: knob launch_blocks at 1 and 3 cuts the
    batch into several launches (the last one not full), each from its own operand and output offsets, which the host
    counts in units -- with the pointers moved in 8-byte units, 20 a term."""
    handles = []
    try:
        runs = later_launch_runs(hip, knobs, entry, 1247, 37, handles)
        assert len(runs) == 2
        for blocks in (1, 3):
            knobs.set("launch_blocks", blocks)
            for case, forms in runs:
                for _ in forms():
                    check_case(case, ends(case.names))
    finally:
        torch.cuda.synchronize()
        for h in handles:
            hip.lib.csgn_uint_lut_destroy(h)
