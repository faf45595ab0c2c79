"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/csgn_hip.h
declares, its host-only metadata helpers agree with the oracle, and -- on a box without a
GPU -- compute entry points fail loudly instead of falling back to the CPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.model import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "csgn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(csgn_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound(lib):
    from csgn_amd import capi
    names = declared_symbols()
    assert len(names) >= 30
    for name in names:
        assert hasattr(lib, name), f"{name} declared in csgn_hip.h but not exported"
        assert name in capi.SIGNATURES, f"{name} missing from csgn_amd.capi.SIGNATURES"
    assert sorted(capi.SIGNATURES) == names
    assert lib.csgn_abi_version() == 1


def test_no_torch_types_or_oracle_in_the_product():
    """The boundary is plain C; the product never reaches into oracle/."""
    hdr = open(os.path.join(ROOT, "include", "csgn_hip.h")).read()
    assert "torch" not in hdr and "at::" not in hdr
    for base, _, files in os.walk(os.path.join(ROOT, "csgn_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(base, f)).read()
                assert "oracle.binding" not in src and "libcsgn_oracle" not in src and "csgn_oracle_" not in src, f
    for base, _, files in os.walk(os.path.join(ROOT, "include")):
        for f in files:
            assert "csgn_oracle_" not in open(os.path.join(base, f)).read(), f


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 1247, 4096, 4097])
def test_metadata_helpers_match_oracle(lib, oracle, n):
    assert lib.csgn_default_len(n) == oracle.default_len(n)
    dl = oracle.default_len(n)
    for d in (1, 4, 16):
        assert lib.csgn_context_s(n, d) == oracle.context_s(n, d)
    for (l1, l2) in [(dl, dl), (dl, 2 * dl), (3 * dl, 5 * dl), (0, dl), (dl, 0)]:
        assert lib.csgn_mul_len(n, l1, l2) == oracle.lib.csgn_oracle_mul_len(dl, l1, l2)
    bl = np.zeros(3 * dl, dtype=np.uint64)
    assert lib.csgn_bitlen_canonical(n, 3, bl.ctypes.data) == 0
    assert np.array_equal(bl, oracle.bitlen(n, 3))
    if n >= 16:
        key = np.random.default_rng(n).permutation(n)[:min(16, n)].astype(np.uint64)
        mask = np.zeros(dl, dtype=np.uint64)
        assert lib.csgn_key_mask(n, key.ctypes.data, key.size, mask.ctypes.data) == 0
        assert np.array_equal(mask, oracle.key_mask(n, key))
        bad = key.copy()
        bad[0] = n
        assert lib.csgn_key_mask(n, bad.ctypes.data, bad.size, mask.ctypes.data) == -1
        assert b"outside" in lib.csgn_last_error()


def test_mul_dispatch_names(lib, knobs):
    """csgn_mul_uniform_kernel reports the measured dispatch rule without a GPU."""
    for k in ("CSGN_MUL_FLAT", "CSGN_MUL_TOUCH"):
        knobs.unset(k)
    name = lambda n, t1, t2, pairs=1 << 16: lib.csgn_mul_uniform_kernel(n, pairs, t1, t2).decode()
    assert name(1247, 1, 1) == "k_and_stream"
    assert name(1247, 1024, 1024, 128) == "k_touch+k_mul_flat"     # the bench launch: 128 pairs, 42 MB of operands
    assert name(1247, 1024, 1024, 1) == "k_mul_tiled"              # a single product is not a stream
    assert name(4096, 256, 256) == "k_touch+k_mul_flat"
    assert name(1247, 16, 8) == "k_touch+k_mul_flat"               # output >= 4x operands: touch + flat
    assert name(1247, 8, 8) == "k_mul_tiled"                       # a whole small pair per 128-thread workgroup
    assert name(1247, 64, 64, 1) == "k_mul_tiled"
    assert name(1247, 4, 4) == "k_mul_tiled"                       # thin and small: 64-thread workgroups, 8 rows per tile
    assert name(1247, 2, 2) == "k_mul_flat"                        # two rows: the flat kernel
    assert name(1247, 1024, 1) == "k_mul_flat"                     # rows of 10 units: the flat kernel
    assert name(4096, 64, 4) == "k_mul_tiled" and name(4096, 2, 2) == "k_mul_flat"
    assert name(1247, 2, 383) == "k_mul_tiled"                     # thin product, long rows
    assert name(1300, 128, 128) == "k_mul_tiled"                   # odd dL: 8-byte units
    assert name(1300, 200, 2) == "k_mul_flat"
    knobs.set("CSGN_MUL_FLAT", "-1")
    assert name(1247, 1024, 1024, 128) == "k_mul_tiled"


def test_fastdiv_helper_is_exact(lib):
    rng = np.random.default_rng(0)
    ds = list(range(1, 130)) + [320, 1000, 4095, 4096, 4097, 10240, 65535, 65536, 3276800, 2**31 - 1, 2**31, 2**32 - 1]
    for d in ds:
        ns = [0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, 2**31 - 1, 2**31, 2**32 - 1] + rng.integers(0, 2**32, 40).tolist()
        for n in ns:
            n &= 0xFFFFFFFF
            assert lib.csgn_debug_fastdiv(n, d) == n // d, (n, d)


BLOCK_ORDER_GROUPS = (0, 1, 2, 3, 5, 64, 100)


def test_block_orders_are_bijections_with_the_documented_runs(lib):
    """xcd_contiguous_block and xcd_grouped_block (csgn_device.h) through csgn_debug_block_order, for every grid of 1 to
    4104 workgroups (eight rounds of group 64 and a tail of 8) and every group the kernels run with or a test sets.
    Workgroup b runs on XCD b % 8.
    Every (grid, group): the image of [0, nblocks) is [0, nblocks).
    group 0: the workgroups of XCD x, in order of b, take one run of consecutive indices, and the runs of x = 0..7 follow
    one another from 0: XCD x owns the x-th contiguous eighth.
    group > 0: every workgroup at or past the last whole round of 8 * group keeps its index; inside the whole rounds
    the workgroups of XCD x, in order of b, take runs of `group` consecutive indices: groups x, x + 8, x + 16, ...
    Then grids around kMaxBlocks256 = (2^32 - 1) / 256, every residue mod 8: the first and the last 64 workgroups land
    inside the grid, on different indices (the arithmetic is 32-bit)."""
    from tests.cpp_driver import build
    fill = C.CDLL(build("tests/cpp/block_order_fill.cpp", "tests/cpp/libblock_order_fill.so", libs=("csgn_hip",),
                        shared=True)).block_order_fill
    fill.argtypes, fill.restype = [C.c_uint32, C.c_uint32, C.c_void_p], None
    top = 4104
    ident = np.arange(top, dtype=np.uint32)
    img = np.empty(top, dtype=np.uint32)
    for group in BLOCK_ORDER_GROUPS:
        for nb in range(1, top + 1):
            img[:] = 0xFFFFFFFF
            fill(nb, group, img.ctypes.data)
            got = img[:nb]
            assert np.array_equal(np.sort(got), ident[:nb]), (nb, group, "not a bijection")
            if group == 0:
                runs = np.concatenate([got[x::8] for x in range(8)])
                assert np.array_equal(runs, ident[:nb]), (nb, "XCD runs are not the contiguous eighths, in order")
                continue
            full = nb - nb % (8 * group)
            assert np.array_equal(got[full:], ident[full:nb]), (nb, group, "a workgroup of the tail moved")
            rounds = full // (8 * group)
            for x in range(8 if rounds else 0):
                mine = got[x:full:8].reshape(rounds, group)
                starts = (np.arange(rounds, dtype=np.uint32) * 8 + x) * group
                assert np.array_equal(mine, starts[:, None] + ident[None, :group]), (nb, group, x)
    k_max_blocks_256 = (2**32 - 1) // 256
    for nb in range(k_max_blocks_256 - 8, k_max_blocks_256 + 2):
        for group in BLOCK_ORDER_GROUPS:
            ends = list(range(64)) + list(range(nb - 64, nb))
            got = [lib.csgn_debug_block_order(b, nb, group) for b in ends]
            assert all(0 <= g < nb for g in got) and len(set(got)) == len(ends), (nb, group)
    assert lib.csgn_debug_block_order(5, 19, 0) == 13 and lib.csgn_debug_block_order(9, 19, 1) == 9   # by hand


def test_plane_entry_points_reject_in_order(lib):
    """csgn_uint_plain and csgn_uint_addk over the sweep of tests/test_uint_plain_cpu.py: the status is that of the
    first check that fails -- n_bits, the comparison, width and constant, host pointers, the term counts (INVALID),
    2^31 words per element and 2^60 per batch (UNSUPPORTED) -- and only then is the device asked for (NO_DEVICE on a
    box without one; with one, the calls that pass every check are not made: their pointers are not device memory)."""
    import torch
    from tests.model import CMPS, plain_terms, u64s
    from tests.model_addk import addk_terms
    from tests.test_uint_plain_cpu import sweep_constants, sweep_term_vectors
    buf = np.zeros(8, dtype=np.uint64)
    planes = (C.c_void_p * 65)(*([buf.ctypes.data] * 65))
    gpu = torch.cuda.is_available()
    rng = np.random.default_rng(19)

    def status(n, batch, counts):
        """counts: each output's terms per element from the model; None or a 0: an argument is refused"""
        dl = (n + 63) // 64
        if n == 0:
            return -1
        if dl * 8 > 16384:
            return -2
        if not counts or not all(counts):
            return -1
        if any(c * dl >= 1 << 31 or batch * c * dl >= 1 << 60 for c in counts):
            return -2
        return -3

    for n, batch in ((1247, 4), (0, 4), (64, 1 << 56), (64, 0), (131073, 4), (1247, 1 << 40)):
        for w in (0, 1, 3, 8, 27, 33, 64, 65):
            for ts in sweep_term_vectors(w, rng):
                for k in sweep_constants(w, rng):
                    fits = 1 <= w <= 64 and k >> w == 0 and all(0 < t < (1 << 62) for t in ts[:w])
                    for cmp in list(CMPS.values()) + [0, 7]:
                        counts = [plain_terms(cmp, w, k, ts[:w])] if fits and cmp in CMPS.values() else None
                        want = status(n, batch, counts)
                        if want != -3 or not gpu:
                            got = lib.csgn_uint_plain(n, cmp, batch, w, k, planes, u64s(ts), buf.ctypes.data, None)
                            assert got == want, (n, batch, cmp, w, k, ts[:w], lib.csgn_last_error())
                    if fits and k and ts[(k & -k).bit_length() - 1] == (1 << 62) - 1:
                        continue                                     # see test_addk_terms_sweep
                    counts = addk_terms(w, k, ts[:w]) if fits else None
                    for negate, carry in ((0, None), (1, None), (0, buf.ctypes.data), (1, buf.ctypes.data)):
                        sized = counts and [c + negate for c in counts[:w]] + ([counts[w]] if carry else [])
                        want = status(n, batch, sized)
                        if want != -3 or not gpu:
                            got = lib.csgn_uint_addk(n, batch, w, k, negate, planes, u64s(ts), planes, carry, None)
                            assert got == want, (n, batch, w, k, negate, carry, ts[:w], lib.csgn_last_error())
    # host pointers are asked for after width and constant and before the term counts
    one = u64s([1] * 65)
    assert lib.csgn_uint_plain(1247, 1, 4, 3, 1, None, one, buf.ctypes.data, None) == -1
    assert lib.csgn_uint_plain(1247, 1, 4, 3, 1, planes, None, buf.ctypes.data, None) == -1
    assert lib.csgn_uint_addk(1247, 4, 3, 1, 0, planes, one, None, None, None) == -1


def test_fails_loudly_without_gpu(lib):
    """No CPU fallback: on a box with no HIP device csgn_init and compute calls report
    CSGN_ERR_NO_DEVICE / HIP errors.  (On a GPU box this test just checks init succeeds.)"""
    import torch
    n = C.c_int(0)
    rc = lib.csgn_device_count(C.byref(n))
    if torch.cuda.is_available():
        assert rc == 0 and n.value >= 1
        return
    assert rc == -3 and n.value == 0
    assert lib.csgn_init(0) == -3
    assert b"no CPU fallback" in lib.csgn_last_error()
    from csgn_amd.capi import CsgnError
    from csgn_amd.batch import HipPath
    with pytest.raises(CsgnError):
        HipPath(0)
    buf = np.zeros(64, dtype=np.uint64)
    rc = lib.csgn_mul_uniform(1247, 1, 1, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 0, None)
    assert rc < 0, "compute call must not succeed without a GPU"
    # a circuit can be described on the host, but building it (allocation + graph capture) cannot succeed
    c = C.c_void_p()
    assert lib.csgn_circuit_create(1247, 4, C.byref(c)) == 0
    a, b, r = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert lib.csgn_circuit_input(c, 1, C.byref(a)) == 0 and lib.csgn_circuit_input(c, 2, C.byref(b)) == 0
    assert lib.csgn_circuit_mul(c, a, b, C.byref(r)) == 0 and lib.csgn_circuit_value_terms(c, r) == 2
    assert lib.csgn_circuit_add(c, r, 17, C.byref(r)) == -1         # no such value
    assert lib.csgn_circuit_build(c) < 0
    assert lib.csgn_circuit_run(c, None) == -1
    lib.csgn_circuit_destroy(c)


def test_integration_md_binding_stub_compiles(tmp_path):
    """The reference-side binding shown in INTEGRATION.md (section B) is real code: extract it
    and compile it against include/csgn_hip.h and the Context class."""
    import subprocess
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```cpp\n(.*?)```", text, flags=re.S)
    stub = [b for b in blocks if "namespace hipbind" in b]
    assert len(stub) == 1
    src = tmp_path / "binding_stub.cpp"
    src.write_text('#include <vector>\n#include "Context.h"\n' + stub[0] +
                   "\nint main() { certFHE::Context c(1247, 16); uint64_t n = 0; (void)c; (void)n;"
                   " (void)&certFHE::hipbind::multiply; (void)&certFHE::hipbind::add;"
                   " (void)&certFHE::hipbind::decrypt; return 0; }\n")
    p = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "include", "certfhe"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_integration_md_sharded_class_snippet_compiles(tmp_path):
    """INTEGRATION.md section C's C++ example of certFHE::ShardedBatch is real code against the shipped
    header: wrapped into a function and compiled (syntax and types only)."""
    import subprocess
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```cpp\n(.*?)```", text, flags=re.S) if "ShardGroup gpus" in b]
    assert len(blocks) == 1
    lines = blocks[0].splitlines()
    head = [l for l in lines if l.startswith("#include") or l.startswith("using namespace")]
    body = [l for l in lines if l not in head]
    src = tmp_path / "sharded_snippet.cpp"
    src.write_text("\n".join(head) + "\nvoid example(const SecretKey &key, const std::vector<unsigned char> &bits_a,\n"
                   "             const std::vector<unsigned char> &bits_b, uint64_t seed_a, uint64_t seed_b, const Permutation &perm)\n{\n"
                   + "\n".join(body) + "\n(void)counts; (void)plain; (void)fast;\n}\nint main() { return 0; }\n")
    p = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "include", "certfhe"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_tuning_knobs_api(lib, knobs):
    """csgn_set_tuning / csgn_get_tuning / csgn_reset_tuning: per-thread knobs, no environment
    reads after load."""
    from csgn_amd import capi
    names = capi.tuning_names()
    assert {"mul_flat", "mul_touch", "ragged_c", "perm_ballot", "dec_loop", "enc_lds"} <= set(names)
    assert len(names) == len(set(names))
    before = capi.get_tuning("mul_ti")
    capi.set_tuning("mul_ti", 9)
    assert capi.get_tuning("mul_ti") == 9 and capi.get_tuning("CSGN_MUL_TI") == 9
    os.environ["CSGN_MUL_TI"] = "77"                 # the environment is NOT consulted again
    try:
        assert capi.get_tuning("mul_ti") == 9
        capi.reset_tuning()
        assert capi.get_tuning("mul_ti") == before
    finally:
        del os.environ["CSGN_MUL_TI"]
    v = C.c_int(0)
    assert lib.csgn_set_tuning(b"no_such_knob", 1) == -1 and b"no_such_knob" in lib.csgn_last_error()
    assert lib.csgn_get_tuning(b"no_such_knob", C.byref(v)) == -1
    assert lib.csgn_set_tuning(None, 1) == -1


def test_launch_blocks_knob_is_last_and_off_by_default(lib, knobs):
    """Knob launch_blocks (the workgroups of one launch where the host splits a call; tests/test_launch_split_gpu.py):
    the newest knob, 0 = the HIP limit unless a test sets it, and no dispatch name depends on it."""
    from csgn_amd import capi
    assert capi.tuning_names()[-1] == "launch_blocks"
    knobs.unset("launch_blocks")
    assert capi.get_tuning("launch_blocks") == 0
    names = lambda: (lib.csgn_mul_uniform_kernel(1247, 3001, 1, 1), lib.csgn_matmul_kernel(1247, 37, 3, 3, 1, 1, 0),  # noqa: E731
                     lib.csgn_gather_kernel(1247, 3001, 1, 1), lib.csgn_gather_kernel(1247, 3001, 0, 2))
    before = names()
    knobs.set("launch_blocks", 15)
    assert capi.get_tuning("launch_blocks") == 15 and names() == before
    assert before == (b"k_and_stream", b"k_matmul", b"k_gather_ragged", b"k_gather")


def test_tuning_knobs_are_per_host_thread(lib, knobs):
    """a knob set by one host thread must not change another thread's dispatch (the C ABI
    is called from one host thread per GPU).  Each thread starts from the defaults and keeps its own values."""
    import threading
    from csgn_amd import capi
    default = capi.get_tuning("mul_flat")
    capi.set_tuning("mul_flat", -1)
    seen = {}

    def other():
        seen["start"] = capi.get_tuning("mul_flat")            # NOT the main thread's -1
        capi.set_tuning("mul_flat", 3)
        capi.set_tuning("mul_touch", 0)
        capi.set_tuning("perm_ballot", 1)
        seen["own"] = capi.get_tuning("mul_flat")
        # dispatch follows the thread's own knobs (no GPU needed for the name)
        seen["kernel"] = lib.csgn_mul_uniform_kernel(1247, 128, 1024, 1024).decode()

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen["start"] == default and seen["own"] == 3 and seen["kernel"] == "k_mul_flat"
    assert capi.get_tuning("mul_flat") == -1 and capi.get_tuning("perm_ballot") == 0
    assert lib.csgn_mul_uniform_kernel(1247, 128, 1024, 1024).decode() == "k_mul_tiled"
    capi.reset_tuning()
    assert lib.csgn_mul_uniform_kernel(1247, 128, 1024, 1024).decode() == "k_touch+k_mul_flat"
    # a caller that shares its GPU asks for the kernel that does not lean on the memory-side cache
    capi.set_tuning("shared_gpu", 1)
    assert lib.csgn_mul_uniform_kernel(1247, 128, 1024, 1024).decode() == "k_mul_tiled"
    capi.reset_tuning()


def test_environment_is_read_in_one_place_only():
    """getenv appears in csgn_tuning.cpp (a load-time snapshot) and nowhere else in the library."""
    src = os.path.join(ROOT, "csgn_amd", "csrc")
    hits = []
    for f in sorted(os.listdir(src)):
        p = os.path.join(src, f)
        if os.path.isfile(p) and "getenv(" in open(p).read():
            hits.append(f)
    assert hits == ["csgn_tuning.cpp"], hits


def test_size_guards_do_not_wrap(lib):
    """Shape limits are evaluated without 64-bit wrap-around and before any device call
    (t1 = t2 = 2^30 at dL = 16 wrapped to 0 and passed)."""
    p = 0x1000                                        # never dereferenced: the guards come first
    assert lib.csgn_mul_uniform(1024, 1, 1 << 30, 1 << 30, p, p, p, 0, None) == -2
    assert lib.csgn_mul_uniform(1247, 1, 1 << 20, 1 << 20, p, p, p, 0, None) == -2
    assert lib.csgn_mul_uniform(1247, 1 << 62, 4, 4, p, p, p, 0, None) == -2
    assert lib.csgn_mul_ragged(1024, 5, p, p, p, p, p, p, 1 << 30, 1 << 30, 7, None) == -2
    assert lib.csgn_add_uniform(1247, 1, 1 << 63, 1 << 63, p, p, p, None) == -2
    assert lib.csgn_add_uniform(1247, 1 << 61, 100, 100, p, p, p, None) == -2
    assert lib.csgn_decrypt_uniform(1247, 1 << 40, 1 << 40, p, p, p, p, None) == -2
    assert lib.csgn_decrypt_product_uniform(1247, 1 << 40, 1 << 40, 1, p, p, p, p, p, None) == -2
    # compaction keeps slot indices in 32 bits: 2^31 terms or more are refused
    assert lib.csgn_compact_ragged(1247, 3, 1 << 31, 0, p, p, p + 0x100000, p, p, None) == -2
    assert b"2^31" in lib.csgn_last_error()
    c = C.c_void_p()
    assert lib.csgn_circuit_create(1024, 1 << 40, C.byref(c)) == 0
    v = C.c_uint32(0)
    assert lib.csgn_circuit_input(c, 1 << 30, C.byref(v)) == -2
    assert lib.csgn_circuit_input(c, 1, C.byref(v)) == 0
    lib.csgn_circuit_destroy(c)
    c = C.c_void_p()
    assert lib.csgn_circuit_create(1024, 2, C.byref(c)) == 0
    a, b, o = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert lib.csgn_circuit_input(c, 1 << 30, C.byref(a)) == 0
    assert lib.csgn_circuit_input(c, 1 << 30, C.byref(b)) == 0
    assert lib.csgn_circuit_mul(c, a, b, C.byref(o)) == -2
    lib.csgn_circuit_destroy(c)


def test_coop_kernel_isa_keeps_loaded_registers_untouched():
    """k_mul_ragged_coop's pipelined form issues its operand loads from inline assembly and retires them with
    hand-counted `s_waitcnt vmcnt(N)`: the compiler believes the loaded registers hold their values at once, so a copy
    of one (a live-range split, a phi) placed in front of the wait would read a register the load has not written yet.
    tools/check_coop_isa.py compiles csgn_mul.hip to gfx950 assembly and walks the control-flow graph from every such
    load to the wait that retires it; no instruction on the way may touch the destination."""
    import shutil
    import subprocess
    import sys
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc on this machine")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_coop_isa.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" 0 findings") == 8, r.stdout          # unit16 / unit8 x 2 / 4 blocks per group x pipelined / plain


def test_form_knobs_are_spelt_alike_everywhere(lib):
    """The six form knobs: the enumerators of csgn_tuning.h, the names csgn_tuning.cpp stores and reads from the
    environment (CSGN_<NAME IN CAPITALS>), the names the class-level driver tests force (tests/cpp_driver.py) and the
    names the Python GPU tests set through the `knobs` fixture are the same six words.  A misspelt name silently
    leaves the default form, and a forced-form test then passes without having forced anything."""
    from tests.cpp_driver import FORM_KNOBS, form_env
    csrc = os.path.join(ROOT, "csgn_amd", "csrc")
    header = open(os.path.join(csrc, "csgn_tuning.h")).read()
    source = open(os.path.join(csrc, "csgn_tuning.cpp")).read()
    enumerators = re.findall(r"^\s*TUNE_(\w+_FUSED),", header, re.M)
    assert sorted(enumerators) == sorted(k.upper() for k in FORM_KNOBS.values())
    for driver, knob in FORM_KNOBS.items():
        assert '{"%s", -1}' % knob in source, knob                     # stored under that name, per shape by default
        assert list(form_env(driver, 0)) == ["CSGN_" + knob.upper()]
        v = C.c_int(7)
        assert lib.csgn_get_tuning(knob.encode(), C.byref(v)) == 0 and v.value in (-1, 0, 1), knob
        module = "test_gates_gpu.py" if driver == "gates" else "test_%s_gpu.py" % driver
        text = open(os.path.join(ROOT, "tests", module)).read()
        used = set(re.findall(r"knobs\.(?:set|unset)\(\s*\"(\w+_fused)\"", text))
        assert knob in used and used <= set(FORM_KNOBS.values()), (module, used)   # its own knob; any other is one of the six
