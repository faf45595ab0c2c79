"""The drop-in certFHE:: C++ API (include/certfhe/ + libcertFHE.so over the C ABI), driven
through tests/cpp/dropin_driver.cpp -- user-style C++ code mirroring the reference's
tests/basic_operations.cpp, tests/permutations.cpp and tests/timings.cpp, with assertions.

CPU box: the driver builds, and running it fails LOUDLY (no CPU fallback).
GPU box (-m gpu): every flow runs on the device; printed words are compared with the golden
vectors (genuine reference) and with the oracle.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.cpp_driver import LIBDIR, ROOT, fixture, run

KAT_PATH = os.path.join(ROOT, "tests", "golden", "csgn_kat.json")

driver = fixture("tests/cpp/dropin_driver.cpp")


def test_driver_builds_against_dropin_headers(driver):
    assert os.path.exists(driver)
    # the public headers carry the reference's class surface
    for h in ("certFHE.h", "Context.h", "Plaintext.h", "Ciphertext.h", "SecretKey.h",
              "Permutation.h", "Helpers.h", "Timer.h", "utils.h"):
        assert os.path.exists(os.path.join(ROOT, "include", "certfhe", h))


def test_dropin_fails_loudly_without_gpu(driver):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = run(driver, "basic", 1, check=False)
    assert p.returncode == 3
    assert "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_deferred_queue_equals_one_launch_per_operation(driver):
    """Small operator* / operator+ are queued per thread and evaluated together (csgn_small_ops): 20 random expression
    DAGs -- results feeding results, reassigned and destroyed operands, copies, more than a queue-full of operations --
    give the words and plaintexts of the same program with one launch per operation."""
    p = run(driver, "deferred", 20)
    assert "deferred ok rounds=20 n=1247 d=16" in p.stdout
    # ... at odd word counts (the queue's kernel on 8-byte units throughout) and other even ones
    for n, d in ((63, 4), (129, 3), (1300, 4), (4096, 32)):
        p = run(driver, "deferred", 8, n, d)
        assert f"deferred ok rounds=8 n={n} d={d}" in p.stdout
    # ... and a ciphertext whose operation is still queued in one host thread used as an operand in another
    p = run(driver, "deferred_threads", 50)
    assert "deferred threads ok rounds=50" in p.stdout
    # ... a worker's queue evaluated when the worker ends, its results read by the main thread; and one queued const
    # ciphertext decrypted and sized by 4 threads at once
    p = run(driver, "deferred_exit", 20)
    assert "deferred exit ok rounds=20" in p.stdout


@pytest.mark.gpu
def test_basic_operations_flow(driver):
    p = run(driver, "basic", 25)
    assert "Dec ( Enc (1) + Enc (0) ) = 1" in p.stdout
    assert "Dec ( Enc (1) * Enc (0) ) = 0" in p.stdout
    assert "basic ok rounds=25" in p.stdout


@pytest.mark.gpu
def test_permutations_flow(driver):
    assert "permutations ok" in run(driver, "permutations", 3).stdout


@pytest.mark.gpu
def test_timings_flow_and_sizes(driver):
    out = run(driver, "timings").stdout
    assert "sizes 144 352 352 672" in out          # tests/timings.cpp:69-72 of the reference
    assert "Key generation  : " in out and "Decryption  : " in out
    assert out.startswith("N= 1247\nD= 16\nS= 38\n")


@pytest.mark.gpu
def test_api_semantics_and_bitlen_rules(driver):
    assert "api ok" in run(driver, "api").stdout
    assert "bitlen ok" in run(driver, "bitlen").stdout


def parse_cts(stdout, label):
    out = []
    for line in stdout.splitlines():
        if line.startswith(label + " "):
            hexs = line.split("v=")[1].strip()
            out.append(np.array([int(hexs[i:i + 16], 16) for i in range(0, len(hexs), 16)], dtype=np.uint64))
    return out


@pytest.mark.gpu
def test_encrypt_matches_reference_golden(driver):
    """SecretKey::encrypt through the public API under setKey + srand(seed) reproduces the
    genuine reference's fresh ciphertexts bit for bit (golden vectors)."""
    kat = json.load(open(KAT_PATH))
    for case in kat["encrypt"]:
        n, d, seed, bits, key = case["n"], case["d"], case["seed"], case["bits"], case["key"]
        p = run(driver, "encrypt", n, d, seed, len(bits), *bits, *key)
        cts = parse_cts(p.stdout, "ct")
        want = np.array([int(h, 16) for h in case["ct"]], dtype=np.uint64)
        assert np.array_equal(np.concatenate(cts), want), (n, d, seed)
        decs = [int(l.split()[1]) for l in p.stdout.splitlines() if l.startswith("dec ")]
        assert decs == case["dec"]
        dl = (n + 63) // 64
        rem = n % 64
        expect_bl = " ".join(["64"] * (dl - 1) + [str(rem if rem else 64)])
        assert all(l == "bitlen " + expect_bl for l in p.stdout.splitlines() if l.startswith("bitlen"))


@pytest.mark.gpu
@pytest.mark.parametrize("n,d", [(1247, 16), (4096, 32), (130, 3)])
def test_circuit_matches_oracle(driver, oracle, n, d):
    seed = 777
    p = run(driver, "circuit", n, d, seed)
    key = np.array([(i * 37 + 11) % n for i in range(d)], dtype=np.uint64)
    bits = [1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 0, 1]
    fresh_want, _ = oracle.encrypt_seq(n, key, bits, glibc_draws(seed, len(bits) * (n + 2)))
    fresh = parse_cts(p.stdout, "fresh")
    assert np.array_equal(np.concatenate(fresh), fresh_want)
    stages = parse_cts(p.stdout, "stage")
    x, k = fresh[0], 1
    for level in range(1, 7):
        if level % 2:
            x, _ = oracle.add(x, fresh[k]); k += 1
        else:
            rhs, _ = oracle.add(fresh[k], fresh[k + 1])
            x, _ = oracle.mul(n, x, rhs); k += 2
        assert np.array_equal(stages[level - 1], x), level
    decs = [l.split() for l in p.stdout.splitlines() if l.startswith("stage_dec")]
    assert len(decs) == 6 and all(t[1] == t[3] for t in decs)
    assert int(decs[-1][5]) == x.size // oracle.default_len(n)


@pytest.mark.gpu
def test_wire_format_roundtrip(driver, oracle, tmp_path):
    """Ciphertext::serialize / deserialize: the file is the documented layout and
    its words are what the oracle computes for the same seeded inputs."""
    path = tmp_path / "ct.csgn"
    out = run(driver, "wire", path).stdout
    assert "wire ok" in out
    raw = path.read_bytes()
    assert raw[:4] == b"CSGN" and raw[4:8] == bytes([1, 0, 0, 0])
    n, d, words = np.frombuffer(raw[8:32], dtype="<u8")
    assert (n, d, words) == (1247, 16, 80)
    prod = np.frombuffer(raw[32:32 + 8 * 80], dtype="<u8")
    second = raw[32 + 8 * 80:]
    assert second[:4] == b"CSGN" and len(second) == 32 + 8 * 20
    a_words = np.frombuffer(second[32:], dtype="<u8")
    key = np.array([i * 71 + 5 for i in range(16)], dtype=np.uint64)
    fresh, _ = oracle.encrypt_seq(1247, key, [1, 0, 1], glibc_draws(2024, 3 * 1249))
    a, b, c = fresh[:20], fresh[20:40], fresh[40:]
    lhs, _ = oracle.add(a, b)
    rhs, _ = oracle.add(c, a)
    want, _ = oracle.mul(1247, lhs, rhs)
    assert np.array_equal(prod, want) and np.array_equal(a_words, a)
    assert np.array_equal(parse_cts(out, "wire_prod")[0], want)


@pytest.mark.gpu
def test_wire_format_and_host_mirror_throughput(driver):
    """Row f3's staging path: a 2^20-term ciphertext (168 MB) serialised from HBM through the pinned staging
    pair, deserialised the same way, the host mirror of a fresh product -- round trip checked, rates printed
    (tools/prof_r04.sh keeps the lines in profiles/r04/wirebench.log)."""
    out = run(driver, "wirebench").stdout
    assert "wirebench ok" in out
    rates = [float(ln.split("GB/s")[0].split()[-1]) for ln in out.splitlines() if "GB/s" in ln]
    assert len(rates) == 7 and min(rates) > 0.2, out      # the per-word loops of round 3 ran at ~0.1 GB/s
    # the buffer forms (round 5): one copy between HBM and a page-locked buffer, no stream sink's memcpy in between
    to_pinned = [float(ln.split("GB/s")[0].split()[-1]) for ln in out.splitlines() if "(pinned buffer)" in ln]
    assert len(to_pinned) == 2 and min(to_pinned) > 20.0, out


@pytest.mark.gpu
def test_batch_extension(driver):
    """certFHE::CiphertextBatch: 4096 depth-6 circuits in lock step vs the clear evaluation,
    the fused decryptProduct, and the per-object API."""
    assert "batch ok count=4096" in run(driver, "batch", 4096).stdout
    assert "batch ok count=7" in run(driver, "batch", 7).stdout


@pytest.mark.gpu
def test_batch_circuit_graph_extension(driver):
    """certFHE::BatchCircuit: BASELINE config 5 captured into a hipGraph, replayed on three input
    sets, against the same circuit done operation by operation and in the clear."""
    assert "graph ok count=1" in run(driver, "graph", 1).stdout
    assert "graph ok count=37" in run(driver, "graph", 37).stdout


def test_libcertfhe_exports_the_reference_class_surface(driver):
    """libcertFHE.so defines every public member of the reference's classes that user code can
    call (src/Ciphertext.h:65-143, src/SecretKey.h:67-143, src/Context.h:28-69,
    src/Permutation.h:27-89, src/Helpers.h:21,38,43, src/Timer.h)."""
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libcertFHE.so")],
                         capture_output=True, text=True, check=True).stdout
    expected = [
        "certFHE::Context::Context(unsigned long, unsigned long)", "certFHE::Context::getN() const",
        "certFHE::Context::getD() const", "certFHE::Context::getS() const",
        "certFHE::Context::getDefaultN() const", "certFHE::Context::setN(unsigned long)",
        "certFHE::Context::setD(unsigned long)",
        "certFHE::Ciphertext::Ciphertext()",
        "certFHE::Ciphertext::Ciphertext(unsigned long const*, unsigned long const*, unsigned long, certFHE::Context const&)",
        "certFHE::Ciphertext::Ciphertext(certFHE::Ciphertext const&)",
        "certFHE::Ciphertext::operator+(certFHE::Ciphertext const&) const",
        "certFHE::Ciphertext::operator+=(certFHE::Ciphertext const&)",
        "certFHE::Ciphertext::operator*(certFHE::Ciphertext const&) const",
        "certFHE::Ciphertext::operator*=(certFHE::Ciphertext const&)",
        "certFHE::Ciphertext::operator=(certFHE::Ciphertext const&)",
        "certFHE::Ciphertext::setValues(unsigned long const*, unsigned long)",
        "certFHE::Ciphertext::setBitlen(unsigned long const*, unsigned long)",
        "certFHE::Ciphertext::setContext(certFHE::Context const&)",
        "certFHE::Ciphertext::getLen() const", "certFHE::Ciphertext::getContext() const",
        "certFHE::Ciphertext::getValues() const", "certFHE::Ciphertext::getBitlen() const",
        "certFHE::Ciphertext::applyPermutation_inplace(certFHE::Permutation const&)",
        "certFHE::Ciphertext::applyPermutation(certFHE::Permutation const&)",
        "certFHE::Ciphertext::size()",
        "certFHE::SecretKey::SecretKey(certFHE::Context const&)",
        "certFHE::SecretKey::SecretKey(certFHE::SecretKey const&)",
        "certFHE::SecretKey::encrypt(certFHE::Plaintext&)", "certFHE::SecretKey::decrypt(certFHE::Ciphertext&)",
        "certFHE::SecretKey::applyPermutation_inplace(certFHE::Permutation const&)",
        "certFHE::SecretKey::applyPermutation(certFHE::Permutation const&)",
        "certFHE::SecretKey::operator=(certFHE::SecretKey const&)",
        "certFHE::SecretKey::getLength() const", "certFHE::SecretKey::getKey() const",
        "certFHE::SecretKey::setKey(unsigned long*, unsigned long)", "certFHE::SecretKey::size()",
        "certFHE::Permutation::Permutation()", "certFHE::Permutation::Permutation(unsigned long const*, unsigned long)",
        "certFHE::Permutation::Permutation(certFHE::Context const&)", "certFHE::Permutation::Permutation(unsigned long)",
        "certFHE::Permutation::getInverse()", "certFHE::Permutation::operator+(certFHE::Permutation const&) const",
        "certFHE::Permutation::operator+=(certFHE::Permutation const&)",
        "certFHE::Permutation::getLength() const", "certFHE::Permutation::getPermutation() const",
        "certFHE::Permutation::setPermutation(unsigned long*, unsigned long)", "certFHE::Permutation::setLength(unsigned long)",
        "certFHE::Library::initializeLibrary()", "certFHE::Helper::exists(unsigned long const*, unsigned long, unsigned long)",
        "certFHE::Helper::deletePointer(void*, bool)",
        "certFHE::Timer::start()", "certFHE::Timer::stop()", "certFHE::Timer::stopAndPrint()", "certFHE::Timer::getValue()",
        "certFHE::operator<<(std::ostream&, certFHE::Ciphertext const&)",
        "certFHE::operator<<(std::ostream&, certFHE::SecretKey const&)",
        "certFHE::operator<<(std::ostream&, certFHE::Context const&)",
        "certFHE::operator<<(std::ostream&, certFHE::Plaintext const&)",
        "certFHE::operator<<(std::ostream&, certFHE::Permutation const&)",
    ]
    missing = [e for e in expected if e not in out]
    assert not missing, missing


@pytest.mark.parametrize("prog", ["basic_operations.cpp", "permutations.cpp", "timings.cpp"])
def test_reference_demo_programs_compile_and_link_against_the_dropin(driver, prog):
    """Source-level drop-in check: the reference's OWN demo programs, fed to g++ unchanged except for the path of
    the umbrella include, compile and link against include/certfhe + libcertFHE.so.  build() does the compiling
    (oracle/Makefile, target demos: a failure there fails the build) into oracle/_ref/demo_*; this test reads
    only what it made.  (Nothing of the programs is stored in this repo; where build() had no reference sources
    to compile, this test skips -- tests/cpp/dropin_driver.cpp carries the same flows everywhere, with assertions.)"""
    exe = os.path.join(ROOT, "oracle", "_ref", "demo_" + prog.replace(".cpp", ""))
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/demo_* not built (reference sources absent)")
    dyn = subprocess.run(["readelf", "-d", exe], capture_output=True, text=True, check=True).stdout
    assert "[libcertFHE.so]" in dyn, dyn
    import torch
    if not torch.cuda.is_available():
        # no GPU here: the program must fail loudly at library bring-up, not compute on the CPU
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0
        assert "no CPU fallback" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_reference_demo_programs_run_on_the_gpu_through_the_dropin():
    """oracle/_ref/demo_* are the reference's own tests/*.cpp (built in the dev container by
    oracle/Makefile against libcertFHE.so); here they RUN on the MI355X and must print what the
    reference prints: Dec(Enc(1)+Enc(0)) = 1, Dec(Enc(1)*Enc(0)) = 0, Dec(Enc(1)) = 1 after a
    permutation, and the sizes 144 / 352 / 352 / 672."""
    ddir = os.path.join(ROOT, "oracle", "_ref")
    exe = {n: os.path.join(ddir, "demo_" + n) for n in ("basic_operations", "permutations", "timings")}
    if not all(os.path.exists(p) for p in exe.values()):
        pytest.skip("oracle/_ref/demo_* not prebuilt")
    out = subprocess.run([exe["basic_operations"]], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Dec ( Enc (1) + Enc (0) ) = 1" in out.stdout and "Dec ( Enc (1) * Enc (0) ) = 0" in out.stdout
    out = subprocess.run([exe["permutations"]], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Dec ( Enc ( 1 ) ) = 1" in out.stdout
    out = subprocess.run([exe["timings"]], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    for line in ("Secret key size: 144 bytes", "Fresh ciphertext size: 352 bytes",
                 "After multiplication ciphertext size: 352 bytes", "After addition ciphertext size: 672 bytes"):
        assert line in out.stdout
