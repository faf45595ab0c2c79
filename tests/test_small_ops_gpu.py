"""csgn_small_ops -- the one launch behind the class layer's queued operator* / operator+ -- called directly with record
arrays built in numpy (layout pinned in tests/test_small_ops_cpu.py).  k_small_ops picks its unit width PER WORKGROUP
from the record's three pointers, so records with 16-byte-aligned operands and records with one pointer 8 bytes off are
mixed in one launch, at even and odd word counts; the records are read from device memory and from pinned host memory
through its device alias.  Every output against oracle.mul / oracle.add, guard words between the outputs.  Run with
`pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.model import SMALL_OP, hip, np_add, np_mul, rand_terms


pytestmark = pytest.mark.gpu

NS = [63, 64, 65, 128, 129, 1247, 1300, 4096]
GUARD = 0x5A5A5A5A5A5A5A5A
ADD, MUL = 0, 1


class Arena:
    """Words laid out on the host and uploaded once: operands and outputs at chosen word offsets (an even offset is
    16-byte aligned on the device, an odd one 8 bytes off), one guard word after every output."""

    def __init__(self):
        self.parts, self.size, self.outs = [], 0, []

    def put(self, words, odd=False):
        if (self.size % 2 == 1) != odd:
            self.parts.append(np.full(1, GUARD, np.uint64))
            self.size += 1
        at = self.size
        self.parts.append(np.ascontiguousarray(words, dtype=np.uint64).ravel())
        self.size += self.parts[-1].size
        return at

    def output(self, k, odd=False):
        at = self.put(np.full(k, GUARD, np.uint64), odd)
        self.put(np.full(1, GUARD, np.uint64), self.size % 2 == 1)
        self.outs.append((at, k))
        return at

    def upload(self, hip):
        host = np.concatenate(self.parts + [np.full(1, GUARD, np.uint64)])
        self.host = host
        self.dev = hip.upload(host)
        assert self.dev.data_ptr() % 16 == 0
        return self.dev.data_ptr()

    def download_checked(self, hip):
        """The arena after the launch; every word outside the outputs is what was uploaded."""
        got = hip.download(self.dev)
        inside = np.zeros(got.size, dtype=bool)
        for at, k in self.outs:
            inside[at:at + k] = True
        assert np.array_equal(got[~inside], self.host[~inside]), "a word outside the outputs changed"
        return got


def build(n, shapes, moved_of, seed):
    """Records for (kind, t1, t2) shapes; moved_of(i) in {None, 'left', 'right', 'out'} puts that pointer 8 bytes off.
    Returns the arena, the records (offsets in words until placed) and the expected words per record."""
    arena, recs, wants = Arena(), np.zeros(len(shapes), dtype=SMALL_OP), []
    for i, (kind, t1, t2) in enumerate(shapes):
        moved = moved_of(i)
        a, b = rand_terms(n, 1, t1, seed + 2 * i), rand_terms(n, 1, t2, seed + 2 * i + 1)
        want = (np_mul(a, b) if kind == MUL else np_add(a, b)).ravel()
        recs[i] = (arena.put(a, moved == "left"), arena.put(b, moved == "right"), arena.output(want.size, moved == "out"),
                   t1, t2, kind, 0)
        wants.append((a.ravel(), b.ravel(), want))
    return arena, recs, wants


def place(recs, base):
    out = recs.copy()
    for f in ("left", "right", "out"):
        out[f] = base + 8 * recs[f].astype(np.uint64)
    return out


def launch(hip, n, recs, pinned=False):
    """Records from device memory, or from pinned host memory through the device alias."""
    if not pinned:
        d = hip.upload(recs.view(np.uint8))
        rc = hip.lib.csgn_small_ops(n, len(recs), d.data_ptr(), hip.stream)
        torch.cuda.synchronize()
        return rc
    h, dev = C.c_void_p(), C.c_void_p()
    assert hip.lib.csgn_host_alloc(C.byref(h), C.byref(dev), recs.nbytes) == 0
    try:
        C.memmove(h, recs.ctypes.data, recs.nbytes)
        rc = hip.lib.csgn_small_ops(n, len(recs), dev, hip.stream)
        torch.cuda.synchronize()                                  # the records stay put until the launch has run
        return rc
    finally:
        hip.lib.csgn_host_free(h)


def check(hip, oracle, n, arena, recs, wants, exact_oracle=True):
    got = arena.download_checked(hip)
    for i, (a, b, want) in enumerate(wants):
        at, kind = int(recs["out"][i]), int(recs["kind"][i])
        words = got[at:at + want.size]
        assert np.array_equal(words, want), (i, kind, int(recs["t1"][i]), int(recs["t2"][i]))
        if exact_oracle and a.size and b.size:
            o = oracle.mul(n, a, b)[0] if kind == MUL else oracle.add(a, b)[0]
            assert np.array_equal(words, o), i


MOVES = [None, None, "left", None, "right", "out"]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("pinned", [False, True])
def test_every_shape_mixed_alignment_one_launch(hip, oracle, n, pinned):
    """Every (t1, t2) in 0..8 x 0..8 for both kinds, empty operands included, in ONE launch; a third of the records
    with one pointer 8 bytes off (the rest 16-byte aligned), so workgroups of both unit widths share the launch."""
    shapes = [(kind, t1, t2) for kind in (ADD, MUL) for t1 in range(9) for t2 in range(9)]
    arena, recs, wants = build(n, shapes, lambda i: MOVES[i % len(MOVES)], 1000 * n)
    base = arena.upload(hip)
    assert launch(hip, n, place(recs, base), pinned) == 0
    check(hip, oracle, n, arena, recs, wants)


@pytest.mark.parametrize("n,count", [(n, c) for n in (1247, 63, 4096) for c in (1, 255, 256, 257)] + [(1247, 70000), (63, 70000)])
@pytest.mark.parametrize("pinned", [False, True])
def test_record_counts(hip, oracle, n, count, pinned):
    """1 to 70 000 records (grids of one to many thousand workgroups), operands shared between records, every output
    its own and checked; every fifth record with its output 8 bytes off."""
    dl = (n + 63) // 64
    rng = np.random.default_rng(count + n)
    pool_terms = 16
    pool = rand_terms(n, 1, pool_terms, count).reshape(pool_terms, dl)
    arena = Arena()
    pool_at = arena.put(pool)
    pool_odd = arena.put(pool, True)
    kinds = rng.integers(0, 2, count)
    t1s, t2s = rng.integers(1, 4, count), rng.integers(1, 4, count)
    starts1 = rng.integers(0, pool_terms - 3, count)
    starts2 = rng.integers(0, pool_terms - 3, count)
    recs = np.zeros(count, dtype=SMALL_OP)
    wants = []
    for i in range(count):
        a, b = pool[starts1[i]:starts1[i] + t1s[i]][None], pool[starts2[i]:starts2[i] + t2s[i]][None]
        want = (np_mul(a, b) if kinds[i] == MUL else np_add(a, b)).ravel()
        left = (pool_odd if i % 7 == 3 else pool_at) + int(starts1[i]) * dl
        recs[i] = (left, pool_at + int(starts2[i]) * dl, arena.output(want.size, i % 5 == 2), t1s[i], t2s[i], kinds[i], 0)
        wants.append((a.ravel(), b.ravel(), want))
    base = arena.upload(hip)
    assert launch(hip, n, place(recs, base), pinned) == 0
    check(hip, oracle, n, arena, recs, wants, exact_oracle=count <= 257)


def test_refusals_before_any_launch(hip):
    lib = hip.lib
    assert lib.csgn_small_ops(1247, 1, None, hip.stream) == -1                       # null records
    assert lib.csgn_small_ops(1247, 0, None, hip.stream) == 0                        # nothing to do
    assert lib.csgn_small_ops(0, 1, None, hip.stream) == -1                          # N = 0
    # 2^24 records: refused (CSGN_ERR_UNSUPPORTED).  The array is all empty additions, so that even a launch would
    # read only records that write nothing.
    count = 1 << 24
    zeros = torch.zeros(count * SMALL_OP.itemsize, dtype=torch.uint8, device=hip.device)
    assert lib.csgn_small_ops(1247, count, zeros.data_ptr(), hip.stream) == -2
    assert b"2^24" in lib.csgn_last_error()
    torch.cuda.synchronize()
