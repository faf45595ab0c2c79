"""Gather / tile / broadcast of ciphertext batches (csgn_gather*) on a box without a GPU: argument checks, dispatch names,
the loud failure without a device, and the numpy model of the definition in include/csgn_hip.h that
tests/test_gather_gpu.py checks the device against."""
import ctypes as C

import numpy as np
import pytest

from tests.model import (INVALID, NO_DEVICE, UNSUPPORTED, lib, np_gather, np_gather_offsets, np_gather_uniform,
                         tile_index, u64s)


def vps(xs):
    return (C.c_void_p * max(len(xs), 1))(*xs)


# -- the model --------------------------------------------------------------------------------------------------------
def np_concat(parts):
    """parts: [(words, offsets)] -> (words, offsets) of their concatenation."""
    words = np.concatenate([w for w, _ in parts]).astype(np.uint64)
    off = [0]
    for _, o in parts:
        o = np.asarray(o, dtype=np.uint64)
        base = off[-1]
        off.extend(base + int(x) for x in (o[1:] - o[0]))
    return words, np.array(off, dtype=np.uint64)


def test_model_offsets_by_hand():
    off = [0, 2, 2, 5, 6]                       # terms 2, 0, 3, 1
    assert np_gather_offsets(off, [3, 1, 0, 0, 2]).tolist() == [0, 1, 1, 3, 5, 8]
    assert np_gather_offsets(off, [1, 1]).tolist() == [0, 0, 0]            # 0-term elements stay 0 terms
    assert np_gather_offsets(off, []).tolist() == [0]                      # count_out == 0
    assert np_gather_offsets(off, tile_index(4, 6)).tolist() == [0, 2, 2, 5, 6, 8, 8]
    assert np_gather_offsets([0, 3], tile_index(1, 3)).tolist() == [0, 3, 6, 9]   # broadcast


def test_model_words_by_hand():
    dl = 2
    off = np.array([0, 1, 1, 3], dtype=np.uint64)                  # terms 1, 0, 2
    words = np.arange(6, dtype=np.uint64) + 100                    # term k = words 100+2k, 101+2k
    out, out_off = np_gather(words, off, [2, 1, 0, 2], dl)
    assert out_off.tolist() == [0, 2, 2, 3, 5]
    assert out.tolist() == [102, 103, 104, 105, 100, 101, 102, 103, 104, 105]
    out, out_off = np_gather(words, off, [], dl)
    assert out.tolist() == [] and out_off.tolist() == [0]
    uni = np.arange(12, dtype=np.uint64)
    assert np_gather_uniform(uni, 1, [2, 0, 2], 2).tolist() == [4, 5, 0, 1, 4, 5]
    assert np_gather_uniform(uni, 3, tile_index(1, 2), 2).tolist() == list(range(6)) * 2


def test_model_concat_by_hand():
    a = (np.array([1, 2, 3], dtype=np.uint64), np.array([0, 1, 1, 3]))        # dl = 1: terms 1, 0, 2
    b = (np.array([9], dtype=np.uint64), np.array([5, 6]))                   # a slice: offsets need not start at 0
    c = (np.zeros(0, dtype=np.uint64), np.array([0]))                        # an empty part
    words, off = np_concat([a, c, b])
    assert words.tolist() == [1, 2, 3, 9]
    assert off.tolist() == [0, 1, 1, 3, 4]


def test_dispatch_names(lib):
    name = lambda *a: lib.csgn_gather_kernel(*a).decode()      # noqa: E731
    assert name(1247, 100, 0, 1) == "k_gather"                  # uniform, indexed or tile
    assert name(1247, 100, 0, 8) == "k_gather"                  # a plane table: the same kernel, one launch
    assert name(1247, 100, 0, 64) == "k_gather"
    assert name(1247, 100, 1, 1) == "k_gather_ragged"
    assert name(1247, 0, 0, 1) == "none"
    assert name(1247, 0, 1, 1) == "none"
    assert name(0, 100, 0, 1) == ""
    assert name(1247, 100, 0, 0) == ""
    assert name(1247, 100, 0, 65) == ""
    assert name(1247, 100, 1, 2) == ""                          # ragged planes are gathered one by one


def test_argument_errors_before_the_device(lib):
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    res = u64s([7, 7])
    # n_bits == 0, null pointers with nonzero counts
    assert lib.csgn_gather(0, 4, p, None, 1, 4, p, p, None, 0, None) == INVALID
    assert lib.csgn_gather(1247, 4, None, None, 1, 4, p, p, None, 0, None) == INVALID
    assert lib.csgn_gather(1247, 4, p, None, 1, 4, p, None, None, 0, None) == INVALID
    assert lib.csgn_gather(1247, 4, p, p, 0, 4, p, p, None, 8, None) == INVALID          # ragged without output offsets
    assert lib.csgn_gather(1247, 4, p, None, 1, 4, p, p, p, 0, None) == INVALID          # uniform with output offsets
    assert lib.csgn_gather(1247, 4, None, p, 0, 4, p, p, p, 8, None) == INVALID
    assert lib.csgn_gather(1247, 0, p, None, 1, 4, None, p, None, 0, None) == INVALID    # output from an empty source
    assert lib.csgn_gather(1247, 1 << 32, p, None, 1, 4, None, p, None, 0, None) == INVALID
    assert lib.csgn_gather(1247, 4, p, None, 1, 1 << 32, None, p, None, 0, None) == INVALID
    assert lib.csgn_gather(1247, 4, p, None, 1 << 40, 4, None, p, None, 0, None) == UNSUPPORTED
    assert lib.csgn_gather_plan(4, None, 4, p, None, None, None) == INVALID                # no result array
    assert lib.csgn_gather_plan(4, p, 4, p, None, res, None) == INVALID                    # ragged without d_out_off
    res = u64s([7, 7])
    assert lib.csgn_gather_plan(0, None, 5, p, None, res, None) == INVALID                 # every index is bad
    assert list(res) == [0, 5]
    src, dst = vps([p, p]), vps([p, None])
    assert lib.csgn_gather_planes(0, 2, src, u64s([1, 2]), 4, 4, p, vps([p, p]), None) == INVALID
    assert lib.csgn_gather_planes(1247, 2, src, u64s([1, 2]), 4, 4, p, dst, None) == INVALID
    assert lib.csgn_gather_planes(1247, 2, vps([None, p]), u64s([1, 2]), 4, 4, p, vps([p, p]), None) == INVALID
    assert lib.csgn_gather_planes(1247, 0, src, u64s([1]), 4, 4, p, vps([p]), None) == INVALID
    assert lib.csgn_gather_planes(1247, 65, vps([p] * 65), u64s([1] * 65), 4, 4, p, vps([p] * 65), None) == INVALID
    assert lib.csgn_gather_planes(1247, 2, None, u64s([1, 2]), 4, 4, p, vps([p, p]), None) == INVALID


def test_entry_points_fail_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gather_gpu.py covers the device")
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    res = u64s([0, 0])
    rc = lib.csgn_gather(1247, 4, p, None, 1, 4, p, p, None, 0, None)
    assert rc == NO_DEVICE, lib.csgn_last_error()
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert lib.csgn_gather(1247, 4, p, None, 1, 4, None, p, None, 0, None) == NO_DEVICE                # tile
    assert lib.csgn_gather(1247, 4, p, p, 0, 4, p, p, p, 8, None) == NO_DEVICE                         # ragged
    assert lib.csgn_gather_plan(4, p, 4, p, p, res, None) == NO_DEVICE
    assert lib.csgn_gather_plan(4, None, 4, p, None, res, None) == NO_DEVICE
    assert lib.csgn_gather_planes(1247, 2, vps([p, p]), u64s([1, 3]), 4, 4, p, vps([p, p]), None) == NO_DEVICE
