"""Gather / tile / broadcast on the device (csgn_gather_plan, csgn_gather, csgn_gather_planes), word for word against the
numpy model of tests/test_gather_cpu.py.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from tests.model import INVALID, OK, GuardedOutputs, hip, np_gather, np_gather_offsets, np_gather_uniform, tile_index


pytestmark = pytest.mark.gpu


def words(seed, n):
    return np.random.default_rng(seed).integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(seed & 1)


def index_cases(rng, count_in):
    return {
        "perm": rng.permutation(count_in),
        "repeat": rng.integers(0, count_in, size=3 * count_in + 5),
        "fewer": rng.integers(0, count_in, size=max(count_in // 3, 1)),
        "reversed": np.arange(count_in)[::-1],
        "empty": np.zeros(0, dtype=np.int64),
    }


def up_index(hip, idx):
    idx = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64))
    return hip.upload(idx) if len(idx) else None


def gather_checked(hip, n, count_in, d_src, t, count_out, d_idx, want, what):
    """csgn_gather into a caller tensor of exactly the wanted size between guard words: the words are the model's and
    nothing outside the output was written (tests/model.py, GuardedOutputs)."""
    guarded = GuardedOutputs(hip, [want.size])
    hip.gather(n, count_in, d_src, t, count_out, d_idx, guarded.outs[0])
    return guarded.check([want], what)[0]


@pytest.mark.parametrize("n", [63, 65, 129, 1247, 4096])
@pytest.mark.parametrize("t", [1, 2, 3, 37])
def test_uniform_gather_words(hip, n, t):
    dl = (n + 63) // 64
    count_in = 97
    src = words(n * 100 + t, count_in * t * dl)
    d_src = hip.upload(src)
    rng = np.random.default_rng(n + t)
    for name, idx in index_cases(rng, count_in).items():
        d_idx = up_index(hip, idx)
        rc, total, bad, _ = hip.gather_plan(count_in, len(idx), d_idx)
        assert (rc, total, bad) == (OK, 0, 0), name
        want = np_gather_uniform(src, t, idx, dl)
        got = gather_checked(hip, n, count_in, d_src, t, len(idx), d_idx, want, name)
        assert np.array_equal(got, want), name
    for count_out in (1, 96, 97, 98, 1000):                           # tile
        want = np_gather_uniform(src, t, tile_index(count_in, count_out), dl)
        got = gather_checked(hip, n, count_in, d_src, t, count_out, None, want, count_out)
        assert np.array_equal(got, want), count_out
    want = np.tile(src[: t * dl], 300)                               # broadcast of element 0
    assert np.array_equal(gather_checked(hip, n, 1, d_src, t, 300, None, want, "broadcast"), want)


@pytest.mark.parametrize("n", [63, 65, 129, 1247, 4096])
def test_ragged_gather_words_and_offsets(hip, n):
    dl = (n + 63) // 64
    rng = np.random.default_rng(n)
    count_in = 300
    sizes = rng.integers(0, 6, size=count_in)
    sizes[::7] = 0                                                   # 0-term elements
    sizes[5] = 700                                                   # one large element among small ones
    src_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    src = words(n + 7, int(src_off[-1]) * dl)
    d_src, d_off = hip.upload(src), hip.upload(src_off)
    cases = index_cases(rng, count_in)
    cases["tile"] = None
    for name, idx in cases.items():
        count_out = 2 * count_in + 3 if idx is None else len(idx)
        ref_idx = tile_index(count_in, count_out) if idx is None else idx
        want, want_off = np_gather(src, src_off, ref_idx, dl)
        guarded = []

        def place(n_words):                                          # the planned size decides the output's size
            guarded.append(GuardedOutputs(hip, [n_words]))
            return guarded[0].outs[0]

        got, got_off = hip.gather_ragged(n, count_in, d_src, d_off, count_out,
                                         up_index(hip, idx) if idx is not None else None, out=place)
        assert np.array_equal(hip.download(got_off), want_off), name
        assert np.array_equal(guarded[0].check([want], name)[0], want), name
    # broadcast of a ragged element (the large one)
    one_off = np.array([0, 700], dtype=np.uint64)
    one = src[int(src_off[5]) * dl:int(src_off[6]) * dl]
    got, got_off = hip.gather_ragged(n, 1, hip.upload(one), hip.upload(one_off), 50)
    assert np.array_equal(hip.download(got_off), np.arange(51, dtype=np.uint64) * 700)
    assert np.array_equal(hip.download(got), np.tile(one, 50))


def test_ragged_plan_large_prefix_sum(hip):
    """A plan over more elements than one look-back chunk (4096): the device prefix sum against numpy."""
    rng = np.random.default_rng(5)
    count_in, count_out = 50_000, 300_001
    sizes = rng.integers(0, 4, size=count_in)
    src_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    idx = rng.integers(0, count_in, size=count_out)
    rc, total, bad, out_off = hip.gather_plan(count_in, count_out, up_index(hip, idx), hip.upload(src_off))
    want = np_gather_offsets(src_off, idx)
    assert (rc, bad, total) == (OK, 0, int(want[-1]))
    assert np.array_equal(hip.download(out_off), want)


def test_plan_reports_bad_indices_and_writes_nothing(hip):
    count_in = 40
    src_off = np.arange(count_in + 1, dtype=np.uint64) * 2
    idx = np.arange(10_000, dtype=np.uint64) % count_in
    idx[[3, 77, 9999]] = [count_in, 1 << 40, (1 << 64) - 1]
    d_idx = up_index(hip, idx)
    sentinel = torch.full((len(idx) + 1,), -5, dtype=torch.int64, device=hip.device)
    rc, total, bad, _ = hip.gather_plan(count_in, len(idx), d_idx, hip.upload(src_off), sentinel)
    assert (rc, bad, total) == (INVALID, 3, 0)
    assert bool((sentinel == -5).all())                              # d_out_off untouched
    rc, total, bad, _ = hip.gather_plan(count_in, len(idx), d_idx)  # a uniform source: validation only
    assert (rc, bad) == (INVALID, 3)


@pytest.mark.parametrize("n", [65, 1247])
def test_planes_of_mixed_terms_one_launch(hip, n):
    dl = (n + 63) // 64
    count_in = 123
    terms = [1, 3, 1, 2, 37, 1, 0, 5]                                # a plane of 0 terms writes nothing
    planes = [words(n + 31 * j, count_in * t * dl) for j, t in enumerate(terms)]
    dev = [hip.upload(p) if len(p) else hip.empty_words(1) for p in planes]
    assert hip.lib.csgn_gather_kernel(n, 500, 0, len(terms)) == b"k_gather"
    rng = np.random.default_rng(n)
    idx = rng.integers(0, count_in, size=500)
    wants = [np_gather_uniform(planes[j], t, idx, dl) if t else np.zeros(0, dtype=np.uint64) for j, t in enumerate(terms)]
    guarded = GuardedOutputs(hip, [x.size for x in wants])
    outs = hip.gather_planes(n, dev, terms, count_in, 500, up_index(hip, idx), guarded.outs)
    guarded.check(wants, "planes")
    for j, want in enumerate(wants):
        assert np.array_equal(hip.download(outs[j]), want), j
    outs = hip.gather_planes(n, dev, terms, 1, 77)                  # broadcast of integer 0
    for j, t in enumerate(terms):
        assert np.array_equal(hip.download(outs[j]), np.tile(planes[j][: t * dl], 77)), j


def test_broadcast_past_4_gib(hip):
    """One 1-term element at N=1247 broadcast to 2^25 elements: 5.4 GB of output, past 2^32 bytes."""
    n, count = 1247, 1 << 25
    dl = (n + 63) // 64
    src = hip.upload(words(11, dl))
    out = hip.gather(n, 1, src, 1, count)
    torch.cuda.synchronize()
    assert out.numel() * 8 > (1 << 32)
    assert torch.equal(out.view(count, dl), src.view(1, dl).expand(count, dl))
    del out
    torch.cuda.empty_cache()


def test_gather_graph_capture_and_replay(hip):
    n, t, count_in = 1247, 2, 300
    dl = (n + 63) // 64
    src = words(21, count_in * t * dl)
    d_src = hip.upload(src)
    idx = np.random.default_rng(3).permutation(count_in)
    d_idx = up_index(hip, idx)
    out = hip.empty_words(count_in * t * dl)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        hip.gather(n, count_in, d_src, t, count_in, d_idx, out)      # warm-up outside the capture
    s.synchronize()
    out.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        hip.gather(n, count_in, d_src, t, count_in, d_idx, out)
    out.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(hip.download(out), np_gather_uniform(src, t, idx, dl))
