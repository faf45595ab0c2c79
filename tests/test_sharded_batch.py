"""certFHE::ShardGroup / ShardedBatch (include/certfhe/ShardedBatch.h, libcertFHE_shard.so): the
class-level face of the sharded batch, driven through
tests/cpp/sharded_driver.cpp.

CPU box: the library and the driver build, the library exports the class surface, and the driver
fails LOUDLY without a GPU (no CPU fallback).
GPU box (-m gpu): on every visible GPU (world 1 on the one-GPU box) the sharded batch holds exactly
the words certFHE::CiphertextBatch holds, for both forms of the gather; a failing rank surfaces as
an exception instead of a hang.
"""
import os
import subprocess

import pytest

from tests.cpp_driver import LIBDIR, SHARDED, fixture, run

driver = fixture("tests/cpp/sharded_driver.cpp", libs=SHARDED)


def test_library_exports_the_class_surface(driver):
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libcertFHE_shard.so")],
                         capture_output=True, text=True, check=True).stdout
    for sym in ("certFHE::ShardGroup::ShardGroup(", "certFHE::ShardGroup::collective", "certFHE::ShardGroup::injectFailure(",
                "certFHE::ShardedBatch::encrypt(", "certFHE::ShardedBatch::encryptProduct(", "certFHE::ShardedBatch::operator*(",
                "certFHE::ShardedBatch::operator+(", "certFHE::ShardedBatch::decrypt(", "certFHE::ShardedBatch::termCounts()",
                "certFHE::ShardedBatch::digest()", "certFHE::ShardedBatch::values(", "certFHE::ShardedBatch::applyPermutation(",
                "certFHE::ShardedBatch::decryptProduct(", "certFHE::ShardedBatch::decryptSum("):
        assert sym in out, sym
    # RCCL comes in through libcsgn_shard.so only; the single-GPU class library must stay free of it
    needed = lambda lib: " ".join(l for l in subprocess.run(["readelf", "-d", os.path.join(LIBDIR, lib)], capture_output=True,
                                                              text=True, check=True).stdout.splitlines() if "NEEDED" in l)
    assert "libcsgn_shard.so" in needed("libcertFHE_shard.so")
    assert "rccl" not in needed("libcertFHE.so") and "csgn_shard" not in needed("libcertFHE.so")


def test_fails_loudly_without_gpu(driver):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = run(driver, "compare", 16, timeout=120, check=False)
    assert p.returncode == 3 and ("no HIP device" in p.stderr or "no CPU fallback" in p.stderr or "no ROCm-capable" in p.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("count,n,d", [(1, 1247, 16), (1000, 1247, 16), (70001, 1247, 16), (257, 4096, 32), (5, 64, 2)])
def test_sharded_batch_equals_the_one_gpu_batch(driver, count, n, d):
    p = run(driver, "compare", count, n, d)
    assert "FAIL" not in p.stdout and p.stdout.count("OK ") >= 28
    assert "grouped ncclBroadcast" in p.stdout and "RCCL 2." in p.stdout


@pytest.mark.gpu
def test_a_failing_rank_is_an_exception_not_a_hang(driver):
    p = run(driver, "fail", 4096, timeout=120)
    assert "FAIL" not in p.stdout and "injected failure" in p.stdout
