"""The life cycle of the per-thread device memory behind the kernels: the temporary blocks of the twelve composed forms
(csgn_amd/csrc/csgn_scratch.cpp: one block per user and stream, grown with hipFree + hipMalloc, the least recently used
evicted at a ninth stream, a temporary past 256 MiB owned by its call, allocation refused under capture, a block or row
table that a capture has seen kept until the thread ends) and the row tables of csgn_uint_pick_rows.

Every output lies between guard words and is compared word for word with the numpy model of its operation
(tests/model*.py), never with another run; every test asserts the form it forced by the entry point's name function; and
growth, eviction, re-use and retirement are ASSERTED from csgn_scratch_stats, not inferred.  The state is per host thread,
so every test body runs in a host thread of its own, which starts with no block, no table and its own knobs and gives
everything back when it ends: the counts below are exact whatever ran before.

Shapes: N = 1247 (even dL: 16-byte units) and 1300 (odd dL: 8-byte units), index width 3 with planes of 1..3 terms, 5
rows (8 in the nine-stream read), a small batch of 7 and a large one of 56.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C
import gc
import threading

import numpy as np
import pytest
import torch

from csgn_amd import capi
from tests.model import (EQ, FILL, GuardedOutputs, c_terms, hip, np_lut, np_plain, np_read_fast, rand_terms,  # noqa: F401
                         read_terms, u64s)
from tests.model_addk import np_addk
from tests.model_arith import ADD, np_arith_chain
from tests.model_count import np_count
from tests.model_find import np_find_fast
from tests.model_lt_select import minmax_requests, np_lt_select_fast
from tests.model_matmul import np_matmul
from tests.model_pick import EACH, np_pick_fast
from tests.model_pick_rows import np_pick_rows_fast, write_shaped
from tests.model_write import np_write_fast
from tests.test_alignment_gpu import LUT_TABLE, MIXED

pytestmark = pytest.mark.gpu

NS = [1247, 1300]
SMALL, LARGE = 7, 56                    # large = 8 * small: every temporary is linear in the batch
S3 = MIXED[3]                           # index planes of 2, 1 and 3 terms: csgn_uint_plain's EQ chain takes a block
ROWS = 5
KEEP = 256 << 20                        # kScratchKeep
STREAMS = 8                             # kScratchStreams
TABLES = 128                            # kRowsTables
FILL_I64 = int(np.uint64(FILL).astype(np.int64))       # the fill word as torch holds it


def in_thread(body, *args):
    """body(*args) in a host thread of its own; what it raises is raised here, what it returns is returned."""
    box = {}

    def run():
        try:
            torch.cuda.set_device(0)
            box["value"] = body(*args)
            torch.cuda.synchronize()
        except BaseException as e:      # noqa: BLE001 -- handed to the test's thread
            box["error"] = e

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box.get("value")


class Job:
    """One call of one entry point on fixed operands, already on the device: launch() enqueues it into fresh outputs
    between guard words and returns at once; check() compares them with the model's words."""

    def __init__(self, hip, want, launch, name, close=None):
        self.hip, self._launch, self.name, self.close = hip, launch, name, close
        self.want = [np.asarray(w).ravel() for w in want]
        self.fresh()

    def fresh(self):
        self.guarded = GuardedOutputs(self.hip, [w.size for w in self.want])
        return self

    def launch(self):
        self._launch(self.guarded.outs)

    def refill(self):
        for whole in self.guarded.whole:
            whole.fill_(FILL_I64)

    def untouched(self):
        return all((self.hip.download(t) == FILL).all() for t in self.guarded.whole)

    def check(self, what):
        self.guarded.check(self.want, what)


def up(hip, planes):
    return [hip.upload(p.ravel()) for p in planes]


def planes_of(n, batch, terms, seed):
    return [rand_terms(n, batch, t, seed + 7 * k + t) for k, t in enumerate(terms)]


# -- the twelve composed forms: knob, and a builder (hip, n, batch, seed) -> Job ---------------------------------------

def plain_job(hip, n, batch, seed, k=0):            # EQ with 0: every factor is a plane plus ONE, written to the block
    planes = planes_of(n, batch, S3, seed)
    dev = up(hip, planes)
    return Job(hip, [np_plain(n, EQ, planes, k)], lambda o: hip.uint_plain(n, EQ, batch, dev, S3, k, out=o[0]),
               lambda: hip.lib.csgn_uint_plain_kernel(n, EQ, batch, 3, k, u64s(S3)))


def addk_job(hip, n, batch, seed, k=5):
    planes = planes_of(n, batch, S3, seed)
    dev = up(hip, planes)
    outs, carry = np_addk(n, planes, k)
    return Job(hip, list(outs) + [carry],
               lambda o: hip.uint_addk(n, batch, dev, S3, k, carry=True, outs=o[:3], carry_out=o[3]),
               lambda: hip.lib.csgn_uint_addk_kernel(n, batch, 3, k, u64s(S3), 1))


def lut_job(hip, n, batch, seed):
    ts = [1, 2, 1, 1]
    planes = planes_of(n, batch, ts, seed)
    dev = up(hip, planes)
    rc, T = c_terms(hip.lib, LUT_TABLE, 4, 4, ts)
    assert rc == 0
    handle = hip.uint_lut_create(LUT_TABLE, 4, 4, ts)
    return Job(hip, np_lut(n, planes, LUT_TABLE, 4), lambda o: hip.uint_lut_apply(handle, n, batch, dev, T, outs=o),
               lambda: hip.lib.csgn_uint_lut_kernel(n, handle, batch), lambda: hip.lib.csgn_uint_lut_destroy(handle))


def read_job(hip, n, batch, seed, s=S3, rows=ROWS, t=(1, 2)):
    s, t = list(s), list(t)
    index, table = planes_of(n, batch, s, seed), planes_of(n, rows, t, seed + 100)
    dx, dt = up(hip, index), up(hip, table)
    return Job(hip, np_read_fast(n, index, table), lambda o: hip.uint_read(n, batch, dx, s, rows, dt, t, outs=o),
               lambda: hip.lib.csgn_uint_read_kernel(n, batch, len(s), u64s(s), rows, len(t), u64s(t)))


def find_job(hip, n, batch, seed):
    u, t = [1, 2, 1], [1, 2]
    keys, query, values = planes_of(n, ROWS, u, seed), planes_of(n, batch, S3, seed + 50), planes_of(n, ROWS, t, seed + 100)
    dk, dq, dv = up(hip, keys), up(hip, query), up(hip, values)
    outs, member = np_find_fast(n, keys, query, values, True)
    return Job(hip, list(outs) + [member],
               lambda o: hip.uint_find(n, batch, dq, S3, ROWS, dk, u, dv, t, outs=o[:2], member=o[2]),
               lambda: hip.lib.csgn_uint_find_kernel(n, batch, 3, u64s(u), u64s(S3), ROWS, 2, u64s(t), 1))


def lt_select_job(hip, n, batch, seed):
    ta, tb = [1, 2, 1], S3
    host = planes_of(n, batch, ta, seed) + planes_of(n, batch, tb, seed + 50)
    dev = up(hip, host)
    xi, yi = minmax_requests([0, 1, 2], [3, 4, 5])
    tx, ty = [host[h].shape[1] for h in xi], [host[h].shape[1] for h in yi]
    outs, less = np_lt_select_fast(n, host[:3], host[3:], [host[h] for h in xi], [host[h] for h in yi], True)
    m = len(xi)
    return Job(hip, list(outs) + [less],
               lambda o: hip.uint_lt_select(n, batch, dev[:3], ta, dev[3:], tb, [dev[h] for h in xi], tx,
                                            [dev[h] for h in yi], ty, outs=o[:m], less=o[m]),
               lambda: hip.lib.csgn_uint_lt_select_kernel(n, batch, 3, u64s(ta), u64s(tb), m, u64s(tx), u64s(ty), 1))


def pick_job(hip, n, batch, seed):
    w, t = 2, 2
    index = planes_of(n, batch, S3, seed)
    src = [rand_terms(n, batch * ROWS, t, seed + 100 + 11 * j) for j in range(w)]
    dx, ds = up(hip, index), up(hip, src)
    return Job(hip, np_pick_fast(n, EACH, index, src, ROWS),
               lambda o: hip.uint_pick(n, EACH, batch, dx, S3, ds, t, ROWS, outs=o),
               lambda: hip.lib.csgn_uint_pick_kernel(n, EACH, batch, 3, u64s(S3), w, ROWS, t))


def write_job(hip, n, batch, seed):
    tv, td = [2, 2], [3, 3]
    index, value = planes_of(n, batch, S3, seed), planes_of(n, batch, tv, seed + 100)
    arrays = planes_of(n, batch * ROWS, td, seed + 500)
    dx, dv, da = up(hip, index), up(hip, value), up(hip, arrays)
    return Job(hip, np_write_fast(n, index, value, arrays, ROWS),
               lambda o: hip.uint_write(n, batch, dx, S3, ROWS, dv, tv, da, td, outs=o),
               lambda: hip.lib.csgn_uint_write_kernel(n, batch, 3, u64s(S3), ROWS, 2, u64s(tv), u64s(td)))


def arith_job(hip, n, batch, seed):
    ta, tb = [1, 2, 1], S3
    a, b = planes_of(n, batch, ta, seed), planes_of(n, batch, tb, seed + 50)
    da, db = up(hip, a), up(hip, b)
    outs, carry = np_arith_chain(n, ADD, a, b, True)
    return Job(hip, list(outs) + [carry],
               lambda o: hip.uint_arith(n, ADD, batch, da, ta, db, tb, outs=o[:3], carry=o[3]),
               lambda: hip.lib.csgn_uint_arith_kernel(n, ADD, batch, 3, u64s(ta), u64s(tb), 1))


def rows_tables(rows=ROWS, salt=0):
    """Two planes of different row tables: what csgn_uint_write leaves, and rows of 1..5 terms."""
    return [write_shaped(S3, rows), [1 + (3 * r + salt) % 5 for r in range(rows)]]


def pick_rows_job(hip, n, batch, seed, T=None):
    T = T or rows_tables()
    flat = [t for plane in T for t in plane]
    index = planes_of(n, batch, S3, seed)
    arrays = [rand_terms(n, batch, sum(t), seed + 500 + 13 * j) for j, t in enumerate(T)]
    dx, da = up(hip, index), up(hip, arrays)
    assert hip.lib.csgn_uint_pick_rows_check(n, batch, 3, u64s(S3), len(T[0]), len(T), u64s(flat)) == 0
    return Job(hip, np_pick_rows_fast(n, index, arrays, T),
               lambda o: hip.uint_pick_rows(n, batch, dx, S3, len(T[0]), da, T, outs=o),
               lambda: hip.lib.csgn_uint_pick_rows_kernel(n, batch, 3, u64s(S3), len(T[0]), len(T), u64s(flat)))


def count_job(hip, n, batch, seed):
    g, t, js = 5, 2, [0, 1, 2]
    x = rand_terms(n, batch * g, t, seed)
    dev = hip.upload(x.ravel())
    return Job(hip, np_count(x, g, js), lambda o: hip.count(n, batch, g, t, [dev], js, outs=o),
               lambda: hip.lib.csgn_count_kernel(n, batch, g, t, 1, len(js), u64s(js)))


def matmul_job(hip, n, batch, seed):
    inner, cols, ta, tb = 3, 2, 1, 2
    a, b = rand_terms(n, batch * inner, ta, seed), rand_terms(n, inner * cols, tb, seed + 50)
    da, db = hip.upload(a.ravel()), hip.upload(b.ravel())
    return Job(hip, [np_matmul(a, b, batch, inner, cols)],
               lambda o: hip.matmul(n, batch, inner, cols, da, ta, db, tb, False, out=o[0]),
               lambda: hip.lib.csgn_matmul_kernel(n, batch, inner, cols, ta, tb, 0))


FORMS = {
    "uint_plain": ("uint_plain_fused", plain_job), "uint_addk": ("uint_addk_fused", addk_job),
    "uint_lut": ("uint_lut_fused", lut_job), "uint_read": ("uint_read_fused", read_job),
    "uint_find": ("uint_find_form", find_job), "uint_lt_select": ("uint_lt_select_form", lt_select_job),
    "uint_pick": ("uint_pick_fused", pick_job), "uint_write": ("uint_write_fused", write_job),
    "uint_arith": ("uint_arith_form", arith_job), "uint_pick_rows": ("uint_pick_rows_form", pick_rows_job),
    "count": ("count_form", count_job), "matmul": ("matmul_form", matmul_job),
}
NESTED = ["uint_read", "uint_pick", "uint_write", "uint_pick_rows"]    # each calls csgn_uint_plain with a slot of its own


def composed(form, jobs):
    """The calling thread's knob of `form` forced to the composed form, and every job asserted to take it."""
    capi.set_tuning(FORMS[form][0], 0)
    for job in jobs:
        assert job.name() == b"composed", (form, job.name())


def plain_fused(hip, n, batches, s=S3, rows=ROWS):
    """csgn_uint_plain's fused kernel forced, so that a form that calls it for EQ takes no block but its own."""
    capi.set_tuning("uint_plain_fused", 1)
    for batch in batches:
        for r in range(rows):
            assert hip.lib.csgn_uint_plain_kernel(n, EQ, batch, len(s), r, u64s(s)) == b"k_uint_plain"


def close(jobs):
    torch.cuda.synchronize()
    for job in jobs:
        if job.close:
            job.close()


def delta(after, before, *names):
    return tuple(after[k] - before[k] for k in names)


# ------------------------------------------------------------------------------ small, large, small: no host sync between

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_calls_back_to_back_on_one_stream(hip, form, n):
    """Small, large, small and the same small call again on one stream, different operands and outputs, ONE
    synchronisation at the end: a later call re-uses (and the large one replaces) the block that earlier launches still
    read, ordered only by the stream.  The large call grows the form's block once, to 8 times its bytes; the third and
    fourth calls allocate nothing.  (csgn_uint_plain runs fused inside the forms that call it: one block a form.)"""
    def body():
        make = FORMS[form][1]
        jobs = [make(hip, n, SMALL, 10), make(hip, n, LARGE, 20), make(hip, n, SMALL, 30)]
        plain_fused(hip, n, (SMALL, LARGE))                                # first: csgn_uint_plain's own knob is the same
        composed(form, jobs)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stats = [hip.scratch_stats()]
        assert stats[0]["blocks"] == stats[0]["mallocs"] == stats[0]["retired"] == 0           # a thread starts empty
        again = None
        with torch.cuda.stream(stream):
            for job in jobs:
                job.launch()
                stats.append(hip.scratch_stats())
            third = jobs[2].guarded
            again = jobs[2].fresh().guarded                                # the third call once more, into new outputs
            jobs[2].launch()
            stats.append(hip.scratch_stats())
        stream.synchronize()
        try:
            first, large, small, same = stats[1:]
            assert first["blocks"] == 1 and first["mallocs"] == 1 and first["frees"] == 0 and first["bytes"] > 0
            assert delta(large, first, "mallocs", "frees") == (1, 1), (first, large)    # one growth
            assert large["blocks"] == 1 and large["bytes"] == 8 * first["bytes"] and large["retired"] == 0
            assert small == large and same == large, (large, small, same)  # nothing allocated, freed or moved
            jobs[0].check("small"), jobs[1].check("large")
            third.check(jobs[2].want, "small again")
            again.check(jobs[2].want, "the same call again")
        finally:
            close(jobs)

    in_thread(body)


# ------------------------------------------------------------------------------ two streams, nine streams

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", ["uint_read", "uint_find", "uint_write"])
def test_two_streams_interleaved(hip, form, n):
    """Calls on streams A and B in turn with no host synchronisation: each stream has a block of its own in the slot."""
    def body():
        make = FORMS[form][1]
        jobs = [make(hip, n, SMALL, 40 + 10 * i) for i in range(4)]
        composed(form, jobs)
        plain_fused(hip, n, (SMALL,))
        torch.cuda.synchronize()
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        assert a.cuda_stream != b.cuda_stream
        stats = []
        for job, stream in zip(jobs, (a, b, a, b)):
            with torch.cuda.stream(stream):
                job.launch()
            stats.append(hip.scratch_stats())
        torch.cuda.synchronize()
        assert stats[0]["blocks"] == 1 and stats[1]["blocks"] == 2 and stats[1]["bytes"] == 2 * stats[0]["bytes"]
        assert stats[1]["mallocs"] == 2 and stats[1]["frees"] == 0
        assert stats[2] == stats[1] and stats[3] == stats[1]
        for i, job in enumerate(jobs):
            job.check(("A", "B")[i % 2])

    in_thread(body)


@pytest.mark.parametrize("n", NS)
def test_nine_streams_evict_the_least_recently_used(hip, n):
    """One composed csgn_uint_read (8 rows) on each of nine streams: the ninth evicts the first stream's block, the one used least
    recently, and the first stream's next call allocates again (and evicts the second's).  Then a hit on the third stream
    and a tenth stream: the fourth stream's block leaves, not the third's, which the next call on it shows."""
    def body():
        streams = [torch.cuda.Stream() for _ in range(10)]
        assert len({s.cuda_stream for s in streams}) == 10
        order = list(range(9)) + [0, 2, 9, 2, 3]
        jobs = [read_job(hip, n, SMALL, 100 + 10 * i, rows=8) for i in range(len(order))]
        composed("uint_read", jobs)
        plain_fused(hip, n, (SMALL,), rows=8)
        torch.cuda.synchronize()
        stats = [hip.scratch_stats()]
        for job, i in zip(jobs, order):
            with torch.cuda.stream(streams[i]):
                job.launch()
            stats.append(hip.scratch_stats())
        torch.cuda.synchronize()
        assert stats[1]["blocks"] == 1                                     # one block a call: EQ runs fused
        moves = [delta(stats[i + 1], stats[i], "mallocs", "frees") for i in range(len(order))]
        assert moves[:8] == [(1, 0)] * 8 and stats[8]["blocks"] == STREAMS
        assert moves[8] == (1, 1)                                          # the ninth stream: stream 0's block leaves
        assert moves[9] == (1, 1)                                          # stream 0 again: allocated again, stream 1's leaves
        assert moves[10] == (0, 0)                                         # stream 2: a hit, now the most recently used
        assert moves[11] == (1, 1)                                         # the tenth stream: the least recently used leaves
        assert moves[12] == (0, 0)                                         # ... which was not stream 2's
        assert moves[13] == (1, 1)                                         # but stream 3's
        assert stats[-1]["blocks"] == STREAMS and stats[-1]["retired"] == 0
        for job, i in zip(jobs, order):
            job.check(("stream", i))

    in_thread(body)


# ------------------------------------------------------------------------------ nested composed forms

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", NESTED)
def test_nested_composed_forms_keep_separate_blocks(hip, form, n):
    """The composed forms that call csgn_uint_plain -- csgn_uint_read, csgn_uint_pick, csgn_uint_write and
    csgn_uint_pick_rows -- with csgn_uint_plain's own composed form forced too: the EQ chain over index planes of 2, 1 and
    3 terms takes a block while the caller's block holds the caller's temporaries.  Two slots, two blocks; with one
    block between them the chain would overwrite the caller's rows."""
    def body():
        jobs = [FORMS[form][1](hip, n, SMALL, 200), FORMS[form][1](hip, n, LARGE, 210)]
        composed(form, jobs)
        capi.set_tuning("uint_plain_fused", 0)
        for r in range(ROWS):
            for batch in (SMALL, LARGE):
                assert hip.lib.csgn_uint_plain_kernel(n, EQ, batch, 3, r, u64s(S3)) == b"composed"
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stats = []
        with torch.cuda.stream(stream):
            for job in jobs:
                job.launch()
                stats.append(hip.scratch_stats())
        stream.synchronize()
        # two live blocks (the chain's may grow from one constant r to the next inside a call), both 8 times as large
        # behind the large call
        for st in stats:
            assert st["blocks"] == 2 and st["mallocs"] - st["frees"] == 2 and st["retired"] == 0, stats
        assert stats[1]["bytes"] == 8 * stats[0]["bytes"] and stats[1]["mallocs"] >= stats[0]["mallocs"] + 2
        jobs[0].check("small"), jobs[1].check("large")

    in_thread(body)


# ------------------------------------------------------------------------------ a temporary past 256 MiB

def test_a_temporary_past_the_kept_size_belongs_to_its_call(hip):
    """Composed csgn_uint_read at the smallest batch whose temporary, batch * (max_eq + sumt) * dL * 8 bytes
    (read_composed), passes 256 MiB: allocated for the call and freed behind it, one hipMalloc and one hipFree, nothing
    kept.  Fresh index planes, 5 rows, one table plane of one term: max_eq = 8, sumt = 1, E = 22.  The words are checked
    against the model on the first element, the last and both sides of the middle, and the whole output against the fused
    form on the same operands.  About 0.66 GB of output at a time and the 256 MiB temporary."""
    n, s, t = 1247, [1, 1, 1], [1]
    dl = (n + 63) // 64
    max_eq, sumt = int(np.prod([x + 1 for x in s])), sum(t)
    per_element = (max_eq + sumt) * dl * 8
    batch = KEEP // per_element + 1
    assert batch * per_element > KEEP >= (batch - 1) * per_element and per_element == 1440 and batch == 186414
    E = read_terms(s, ROWS)
    assert E == 22

    def body():
        index, table = planes_of(n, batch, s, 300), planes_of(n, ROWS, t, 310)
        dx, dt = up(hip, index), up(hip, table)
        name = lambda: hip.lib.csgn_uint_read_kernel(n, batch, 3, u64s(s), ROWS, 1, u64s(t))    # noqa: E731
        capi.set_tuning("uint_read_fused", 0)
        assert name() == b"composed"
        plain_fused(hip, n, (batch,), s)
        words = batch * E * dl
        guarded = GuardedOutputs(hip, [words])
        torch.cuda.synchronize()
        before = hip.scratch_stats()
        hip.uint_read(n, batch, dx, s, ROWS, dt, t, outs=guarded.outs)
        after = hip.scratch_stats()
        torch.cuda.synchronize()
        assert delta(after, before, "mallocs", "frees", "bytes", "blocks", "retired") == (1, 1, 0, 0, 0), (before, after)
        whole = hip.download(guarded.whole[0])
        first = guarded.first
        assert (whole[:first] == FILL).all() and (whole[first + words:] == FILL).all()
        got = whole[first:first + words].reshape(batch, E * dl)
        sample = [0, batch // 2 - 1, batch // 2, batch - 1]
        want = np_read_fast(n, [p[sample] for p in index], table)[0].reshape(len(sample), E * dl)
        for i, e in enumerate(sample):
            assert np.array_equal(got[e], want[i]), e
        del guarded
        torch.cuda.empty_cache()
        capi.set_tuning("uint_read_fused", 1)
        assert name() == b"k_uint_read"
        fused = hip.uint_read(n, batch, dx, s, ROWS, dt, t)[0]
        torch.cuda.synchronize()
        assert hip.scratch_stats() == after
        assert np.array_equal(hip.download(fused).reshape(batch, E * dl), got)

    in_thread(body)


# ------------------------------------------------------------------------------ capture

def capture(stream, body):
    """body() captured on `stream`.  The capture is in torch's global error mode, where a HIP call that capture forbids,
    from any thread, breaks the capture and can end the process; a cyclic collection that starts inside it may finalize whatever an earlier test
    left behind, device memory and graphs among it, and torch.cuda.graph no longer collects before it begins.  So the
    garbage goes first and the collector stays off until the capture has ended."""
    g = torch.cuda.CUDAGraph()
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, stream=stream):
            body()
    finally:
        if was_on:
            gc.enable()
    torch.cuda.synchronize()
    return g


def warm_and_capture(hip, job, stream):
    """The call once outside capture on `stream` (its words checked), then captured into fresh outputs; returns the graph,
    its outputs holding the fill again."""
    with torch.cuda.stream(stream):
        job.launch()
    stream.synchronize()
    job.check("warm")
    job.fresh()
    torch.cuda.synchronize()
    before = hip.scratch_stats()
    g = capture(stream, job.launch)
    assert hip.scratch_stats() == before                                   # a warm call under capture allocates nothing
    job.refill()                                                           # every word back to the fill
    torch.cuda.synchronize()
    assert job.untouched()
    return g


CAPTURED = ["uint_read", "uint_find", "uint_arith", "count", "matmul", "uint_pick_rows"]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", CAPTURED)
def test_capture_of_a_warm_call(hip, form, n):
    """A composed call whose block is large enough (csgn_uint_pick_rows: the fused form, its row tables on the device) is
    captured on a side stream and replayed into outputs that hold the fill again."""
    def body():
        job = FORMS[form][1](hip, n, SMALL, 400)
        if form == "uint_pick_rows":
            capi.set_tuning("uint_pick_rows_form", 1)
            assert job.name() == b"k_uint_pick_rows"
        else:
            composed(form, [job])
        plain_fused(hip, n, (SMALL,))
        stream = torch.cuda.Stream()
        g = warm_and_capture(hip, job, stream)
        g.replay()
        torch.cuda.synchronize()
        job.check("replay")
        del g

    in_thread(body)


def capture_text(hip):
    """hipGetErrorString(hipErrorStreamCaptureUnsupported = 900) of the HIP runtime the library is linked with."""
    get = hip.lib.hipGetErrorString
    get.restype, get.argtypes = C.c_char_p, [C.c_int]
    return get(900).decode()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("why", ["a stream never used", "a larger shape"])
def test_capture_of_a_call_that_must_allocate_is_refused(hip, why, n):
    """Composed csgn_uint_read under capture with no block for the stream, or one that is too small: CSGN_ERR_HIP with
    hipErrorStreamCaptureUnsupported's text, the outputs keep their fill, the stats do not move, and the capture -- it
    also holds a torch fill -- still ends and replays."""
    def body():
        warm, job = read_job(hip, n, SMALL, 500), read_job(hip, n, LARGE, 510)
        composed("uint_read", [warm, job])
        plain_fused(hip, n, (SMALL, LARGE))
        stream, other = torch.cuda.Stream(), torch.cuda.Stream()
        assert stream.cuda_stream != other.cuda_stream
        with torch.cuda.stream(other if why == "a stream never used" else stream):
            warm.launch()
        torch.cuda.synchronize()
        warm.check("warm")
        marks = torch.zeros(1000, dtype=torch.int64, device=hip.device)
        before = hip.scratch_stats()
        seen = {}

        def captured():
            marks.fill_(7)
            with pytest.raises(capi.CsgnError) as err:
                job.launch()
            seen["error"] = err.value

        g = capture(stream, captured)
        assert seen["error"].status == capi.CSGN_ERR_HIP
        assert seen["error"].message.startswith("csgn::uint_read(") and seen["error"].message.endswith(": " + capture_text(hip))
        assert hip.lib.csgn_last_error().decode() == seen["error"].message
        assert hip.scratch_stats() == before
        assert int(marks.sum()) == 0                                       # captured, not run
        g.replay()
        torch.cuda.synchronize()
        assert int(marks.sum()) == 7000 and job.untouched()
        with torch.cuda.stream(stream):                                    # outside capture the same call allocates and runs
            job.launch()
        stream.synchronize()
        job.check("eager")
        assert delta(hip.scratch_stats(), before, "mallocs")[0] == 1

    in_thread(body)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("how", ["growth", "eviction"])
def test_replay_after_the_captured_block_was_replaced(hip, how, n):
    """A warm composed csgn_uint_read is captured; then a larger eager call on the same stream grows the stream's block, or
    eight further streams -- nine in all -- evict it.  The captured block is retired, not freed: asserted from the stats
    BEFORE the replay, which then gives the model's words."""
    def body():
        job = read_job(hip, n, SMALL, 600)
        later = [read_job(hip, n, LARGE, 610)] if how == "growth" else [read_job(hip, n, SMALL, 620 + i) for i in range(STREAMS)]
        composed("uint_read", [job] + later)
        plain_fused(hip, n, (SMALL, LARGE))
        stream = torch.cuda.Stream()
        others = [torch.cuda.Stream() for _ in range(STREAMS)]
        assert len({s.cuda_stream for s in others + [stream]}) == STREAMS + 1
        g = warm_and_capture(hip, job, stream)
        before = hip.scratch_stats()
        assert before["blocks"] == 1 and before["retired"] == 0 and before["frees"] == 0
        for i, x in enumerate(later):
            with torch.cuda.stream(stream if how == "growth" else others[i]):
                x.launch()
        torch.cuda.synchronize()
        after = hip.scratch_stats()
        assert delta(after, before, "retired", "frees", "mallocs") == (1, 0, len(later)), (before, after)
        assert after["blocks"] == (1 if how == "growth" else STREAMS)
        g.replay()
        torch.cuda.synchronize()
        job.check("replay")
        for x in later:
            x.check("later")
        assert delta(hip.scratch_stats(), after, "retired", "frees", "mallocs") == (0, 0, 0)
        del g

    in_thread(body)


@pytest.mark.parametrize("n", NS)
def test_replay_after_the_captured_row_tables_left_the_cache(hip, n):
    """A warm csgn_uint_pick_rows call (the fused form) is captured; 128 further table shapes through the host-only
    csgn_uint_pick_rows_check then push its two tables out of the cache.  Their device copies are retired, not freed:
    asserted from the stats BEFORE the replay, which then gives the model's words."""
    def body():
        T = rows_tables()
        job = pick_rows_job(hip, n, SMALL, 700, T)
        capi.set_tuning("uint_pick_rows_form", 1)
        assert job.name() == b"k_uint_pick_rows"
        g = warm_and_capture(hip, job, torch.cuda.Stream())
        before = hip.scratch_stats()
        assert before["tables"] == 2 and before["tables_retired"] == 0 and before["tables_freed"] == 0
        for i in range(TABLES):
            rows = [7 + i] + [1] * (ROWS - 1)                              # no table of the captured call
            assert rows not in T
            assert hip.lib.csgn_uint_pick_rows_check(n, SMALL, 3, u64s(S3), ROWS, 1, u64s(rows)) == 0
        after = hip.scratch_stats()
        assert after["tables"] == TABLES and after["tables_retired"] == 2 and after["tables_freed"] == 0, (before, after)
        g.replay()
        torch.cuda.synchronize()
        job.check("replay")
        # the same shape again builds and uploads new tables; the graph keeps the retired ones
        again = pick_rows_job(hip, n, SMALL, 710, T)
        again.launch()
        torch.cuda.synchronize()
        again.check("eager, tables built again")
        job.refill()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        job.check("second replay")
        assert hip.scratch_stats()["tables_freed"] == 0
        del g

    in_thread(body)


def test_tables_never_captured_are_freed_when_they_leave(hip):
    """The other side of the rule: a table whose device copy no capture has seen gives the copy back when it leaves."""
    def body():
        n = 1247
        job = pick_rows_job(hip, n, SMALL, 800)
        capi.set_tuning("uint_pick_rows_form", 1)
        assert job.name() == b"k_uint_pick_rows"
        job.launch()
        torch.cuda.synchronize()
        job.check("eager")
        for i in range(TABLES):
            assert hip.lib.csgn_uint_pick_rows_check(n, SMALL, 3, u64s(S3), ROWS, 1, u64s([7 + i] + [1] * (ROWS - 1))) == 0
        stats = hip.scratch_stats()
        assert stats["tables"] == TABLES and stats["tables_retired"] == 0 and stats["tables_freed"] == 2

    in_thread(body)


# ------------------------------------------------------------------------------ two host threads

def test_two_host_threads(hip, knobs):
    """Two host threads at once, each with its own knobs (knobs are per thread), its own stream and twenty composed calls,
    csgn_uint_read and csgn_uint_find in turn, on fresh operands: the right words in both, and each thread's stats show
    its own two blocks only -- the batches differ, 5 and 11, and so do the bytes, in that ratio.  After both have ended a
    call on the test's own thread is still right."""
    n, calls = 1247, 20
    start = threading.Barrier(2)
    results, errors = {}, []

    def worker(batch, seed):
        try:
            torch.cuda.set_device(0)
            assert capi.get_tuning("uint_read_fused") != 0 and capi.get_tuning("uint_find_form") != 0   # a thread's own knobs
            jobs = [(read_job if i % 2 == 0 else find_job)(hip, n, batch, seed + 10 * i) for i in range(calls)]
            composed("uint_read", jobs[0::2])
            composed("uint_find", jobs[1::2])
            plain_fused(hip, n, (batch,))
            torch.cuda.synchronize()
            stream = torch.cuda.Stream()
            assert hip.scratch_stats()["blocks"] == 0
            start.wait(timeout=60)
            with torch.cuda.stream(stream):
                for job in jobs:
                    job.launch()
            stream.synchronize()
            for i, job in enumerate(jobs):
                job.check((batch, i))
            results[batch] = hip.scratch_stats()
        except BaseException as e:      # noqa: BLE001 -- handed to the test's thread
            errors.append(e)
            start.abort()

    threads = [threading.Thread(target=worker, args=(5, 1000)), threading.Thread(target=worker, args=(11, 2000))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    a, b = results[5], results[11]
    for stats in (a, b):
        assert stats["blocks"] == 2 and stats["mallocs"] == 2 and stats["frees"] == 0 and stats["retired"] == 0, stats
    assert a["bytes"] * 11 == b["bytes"] * 5 and a["bytes"] > 0
    knobs.set("uint_read_fused", 0)
    job = read_job(hip, n, SMALL, 3000)
    assert job.name() == b"composed"
    job.launch()
    torch.cuda.synchronize()
    job.check("the test's own thread")
