"""The circuit compiler (csgn_circuit_optimize / csgn_circuit_build, csgn_amd/csrc/csgn_circuit.hip) on the HOST:
csgn_circuit_plan_json runs its passes -- decrypt fusion, dead-node removal, placement of producers into the sums that
consume them, liveness-driven layout of the block -- without a device, and this file EXECUTES the resulting plan in
numpy (every kept node reads and writes one byte array at the plan's offsets and pitches) against the same circuit
evaluated value by value with the oracle.  A wrong offset, an overlapping pair of live regions, a fusion that fired on a
shared sub-expression or a node dropped while something still read it all show up as wrong words or bits here, before
any GPU is involved.  The GPU tests (tests/test_gpu_parity.py::test_circuit_compiled_*) repeat the property on the
real kernels.  Reference semantics: src/Ciphertext.cpp:107-122 (add = concatenation), :146-163 (all-pairs AND),
src/SecretKey.cpp:104-147 (decrypt = XOR over terms of AND over key positions)."""
import ctypes as C

import numpy as np
import pytest

from csgn_amd import capi
from csgn_amd.capi import check
from tests.model import Described, config5, decrypt_masked, evaluate, execute, lib, random_circuit

REUSE, PLACE, FUSE, PUSHDOWN, HOIST = 1, 2, 4, 8, 16
CORE, ALL = 7, 23
FOREVER = 2 ** 31 - 1


def check_regions(plan):
    """No two regions that are live at the same node overlap."""
    regs = plan["regions"]
    for i, a in enumerate(regs):
        assert a["at"] % 256 == 0 and a["at"] + a["bytes"] <= plan["bytes"]
        for b in regs[i + 1:]:
            if a["from"] <= b["to"] and b["from"] <= a["to"]:
                assert a["at"] + a["bytes"] <= b["at"] or b["at"] + b["bytes"] <= a["at"], (a, b)


@pytest.mark.parametrize("flags", [ALL, CORE, REUSE, PLACE, FUSE, HOIST, REUSE | HOIST, PLACE | FUSE, ALL | PUSHDOWN, REUSE | PUSHDOWN])
def test_compiled_plans_of_random_circuits_compute_what_the_tape_computes(lib, flags):
    """60 random DAGs per flag set (chains, shared sub-expressions, squares a*a and doubles a+a, values nobody reads,
    several decrypts, random retained outputs): the executed plan's retained words and all bits equal the direct
    evaluation; no two live regions overlap; nothing that has two readers was placed or dissolved."""
    for seed in range(60):
        n, batch = ((130, 3), (128, 2), (64, 4))[seed % 3]
        d = random_circuit(lib, 1000 + seed, n, batch)
        try:
            plan = d.plan(flags)
            check_regions(plan)
            rng = np.random.default_rng(seed)
            inputs = {v: rng.integers(0, 2 ** 63, size=(batch, d.terms[v], d.dl), dtype=np.uint64) | np.uint64(1 << 63)
                      for v, node in enumerate(d.nodes) if node[0] == "in"}
            mask = np.zeros(d.dl, dtype=np.uint64)
            mask[0] = np.uint64((1 << 63) | (1 << 62))        # hit iff two bits set: products of random words hit 1 in 2**k
            want = evaluate(d, inputs)
            block, bits, read = execute(d, plan, inputs, mask)
            for bid, v in enumerate(d.decrypts):
                assert np.array_equal(bits[bid], decrypt_masked(want[v], mask)), (seed, bid)
            for v in d.outputs | {i for i, nd in enumerate(d.nodes) if nd[0] == "in"}:
                assert plan["values"][v]["addressable"], (seed, v)
                assert np.array_equal(read(v), want[v]), (seed, v)
            # readers per value among the kept nodes and the decrypt leaves
            readers = [0] * len(d.terms)
            for op in plan["ops"]:
                if op["elided"] or (op["kind"] == 2 and op["expr"] >= 0):
                    continue
                readers[op["a"]] += 1
                if op["kind"] in (0, 1):
                    readers[op["b"]] += 1
            for e in plan["exprs"]:
                if e["kind"] < 0:
                    readers[e["value"]] += 1
            for v, pv in enumerate(plan["values"]):
                if pv["parent"] >= 0:
                    assert readers[v] == 1 and v not in d.outputs and d.nodes[v][0] != "in", (seed, v)
                if not pv["region"] and pv["parent"] < 0:
                    assert readers[v] == 0, (seed, v)
            if not flags & PLACE:
                assert all(pv["parent"] < 0 for pv in plan["values"])
            if not flags & HOIST:
                assert not any(op["hoist_a"] or op["hoist_b"] for op in plan["ops"])
            if not flags & (FUSE | PUSHDOWN):
                assert not plan["exprs"]
        finally:
            d.close()


def test_tape_mode_keeps_every_value_in_a_region_of_its_own(lib):
    d = random_circuit(lib, 7, 130, 3)
    try:
        plan = d.plan(0)
        assert all(pv["region"] and pv["addressable"] and pv["parent"] < 0 for pv in plan["values"])
        assert not any(op["elided"] or op["placed_a"] or op["placed_b"] or op["hoist_a"] or op["hoist_b"] for op in plan["ops"])
        check_regions(plan)
        assert all(r["to"] == FOREVER or r["from"] == r["to"] for r in plan["regions"])
    finally:
        d.close()


def test_config5_plan_elides_the_last_product_and_every_copy_of_a_product(lib):
    """BASELINE config 5 (x <- x + e / x <- x * (e + e'), depth 16, 766 terms, then Dec): compiled, the last product is
    never written (Dec(x15 * r) = Dec(x15) & Dec(r)), every other product is written straight into the sum that
    consumes it, and the block holds the peak live set instead of all 41 values."""
    d, x = config5(lib, 4096, 8)
    try:
        tape = d.plan(0)
        comp = d.plan(ALL)
        check_regions(comp)
        muls = [op for op in comp["ops"] if op["kind"] == 1]
        assert len(muls) == 8 and [m["elided"] for m in muls] == [False] * 7 + [True]
        x_adds = [op for op in comp["ops"] if op["kind"] == 0 and d.nodes[op["a"]][0] == "mul"]
        assert len(x_adds) == 7 and all(op["placed_a"] and not op["placed_b"] and op["hoist_b"] for op in x_adds)
        # ... and every copy of an input (the other half of those adds, x0 + e, the eight sums e + e') is in the prologue:
        # no add launches a kernel of its own any more
        adds = [op for op in comp["ops"] if op["kind"] == 0 and not op["elided"]]
        assert all((op["placed_a"] or op["hoist_a"]) and (op["placed_b"] or op["hoist_b"]) for op in adds)
        assert sum(op["hoist_a"] + op["hoist_b"] for op in adds) == 25          # every one of the 25 inputs, once
        dec = [op for op in comp["ops"] if op["kind"] == 2][0]
        root = comp["exprs"][dec["expr"]]
        assert root["kind"] == 1 and comp["exprs"][root["l"]]["kind"] < 0 and comp["exprs"][root["r"]]["kind"] < 0
        assert not comp["values"][x]["region"] and tape["values"][x]["region"]
        # the tape holds every value (1 + 2 + 2 + 4 + ... + 766 terms and the inputs); the compiled block the inputs,
        # the two largest neighbouring sums and scratch
        assert comp["bytes"] * 2 < tape["bytes"]
        # kept as an output, the last product is computed after all
        d.output(x)
        kept = d.plan(ALL)
        assert kept["values"][x]["region"] and kept["values"][x]["addressable"]
        assert not any(op["elided"] for op in kept["ops"])
        # with PUSHDOWN the decrypt reaches the 25 inputs
        d2, x2 = config5(lib, 4096, 8)
        try:
            deep = d2.plan(ALL | PUSHDOWN)
            leaves = [e for e in deep["exprs"] if e["kind"] < 0]
            assert len(leaves) == 25 and all(d2.nodes[e["value"]][0] == "in" for e in leaves)
            assert all(op["elided"] for op in deep["ops"] if op["kind"] != 2)
        finally:
            d2.close()
    finally:
        d.close()


def test_optimize_and_output_argument_checks(lib):
    d = Described(lib, 130, 2)
    try:
        a = d.input(1)
        with pytest.raises(capi.CsgnError):
            check(lib.csgn_circuit_optimize(d.c, 64))                     # unknown flag
        with pytest.raises(capi.CsgnError):
            check(lib.csgn_circuit_output(d.c, 99))                       # no such value
        buf = C.create_string_buffer(64)
        with pytest.raises(capi.CsgnError):
            check(lib.csgn_circuit_plan_json(d.c, buf, len(buf)))         # no operations yet
        d.decrypt(d.add(a, a))
        with pytest.raises(capi.CsgnError):
            check(lib.csgn_circuit_plan_json(d.c, buf, len(buf)))         # buffer too small
        assert lib.csgn_circuit_block_bytes(d.c) == 0                     # not built
        stats = (C.c_uint64 * 8)()
        with pytest.raises(capi.CsgnError):
            check(lib.csgn_circuit_stats(d.c, stats))
    finally:
        d.close()
