"""Placed outputs (CSGN_CIRCUIT_PLACE, csgn_amd/csrc/csgn_circuit.hip): the circuits, shapes and knob settings that
tests/test_placed_outputs_cpu.py and tests/test_placed_outputs_gpu.py share, the plan facts every case must show
before it runs, and a restatement of the multiply launcher's predicates (mul_uniform_chunk, csgn_mul.hip) with a LITERAL
table of the kernel form each case is meant to reach.  Element e of a placed value goes to out + e * pitch, a slice of
the sum that consumes it; the kernels that take a pitch are k_mul_flat_blk<PITCH>, k_mul_flat<PITCH>, k_mul_tiled with
a.opitch, k_add_flat<PITCH> (two operands, or one: the strided copy) and k_copy_list (the HOIST prologue)."""
from tests.model import Described, evaluate, rand_terms

PLACE, HOIST = 2, 16
FLAGS = (PLACE, PLACE | HOIST)

# -- the circuits ------------------------------------------------------------------------------------------------------
# kind -> number of inputs
KINDS = {
    "right": 3,        # s = (a*b) + c          the product in the first slice of every element
    "left": 3,         # s = c + (a*b)          the product starts tc*dL words into the element
    "both": 4,         # s = (a*b) + (c*d)      two placed products; the add emits no kernel
    "nested": 4,       # s = ((a*b) + c) + d    the product's pitch is the OUTER sum's
    "sum_in_sum": 3,   # s = (a+b) + c          k_add_flat<PITCH> with both operands
}


class Circuit:
    """One circuit of KINDS over inputs of `terms` terms each, its final sum marked as an output."""

    def __init__(self, lib, kind, n, batch, terms):
        assert len(terms) == KINDS[kind], (kind, terms)
        self.kind, self.n, self.batch, self.in_terms = kind, n, batch, tuple(terms)
        self.d = d = Described(lib, n, batch)
        self.ins = ins = [d.input(t) for t in terms]
        self.products, self.inner = [], None
        if kind == "right":
            p = d.mul(ins[0], ins[1]); self.products = [p]
            self.s = d.add(p, ins[2])
        elif kind == "left":
            p = d.mul(ins[0], ins[1]); self.products = [p]
            self.s = d.add(ins[2], p)
        elif kind == "both":
            p, q = d.mul(ins[0], ins[1]), d.mul(ins[2], ins[3]); self.products = [p, q]
            self.s = d.add(p, q)
        elif kind == "nested":
            p = d.mul(ins[0], ins[1]); self.products = [p]
            self.inner = d.add(p, ins[2])
            self.s = d.add(self.inner, ins[3])
        else:
            self.inner = d.add(ins[0], ins[1])
            self.s = d.add(self.inner, ins[2])
        d.output(self.s)

    def close(self):
        self.d.close()

    # what the plan must say, and what csgn_circuit_stats must count, for the case to test a placed output at all
    def expected_counts(self, flags):
        """(placed operands, hoisted operands, kernels of the graph)"""
        hoist = bool(flags & HOIST)
        placed = {"right": 1, "left": 1, "both": 2, "nested": 2, "sum_in_sum": 1}[self.kind]
        hoisted = {"right": 1, "left": 1, "both": 0, "nested": 2, "sum_in_sum": 3}[self.kind] if hoist else 0
        products = len(self.products)
        if hoist:
            kernels = products + (1 if hoisted else 0)             # one prologue launch, then the products
        else:
            # without HOIST every input operand of an add is a copy launch of its own (sum_in_sum: a + b is ONE launch)
            kernels = products + {"right": 1, "left": 1, "both": 0, "nested": 2, "sum_in_sum": 2}[self.kind]
        return placed, hoisted, kernels

    def check_plan(self, plan, flags):
        d, dl, s = self.d, self.d.dl, self.s
        vals, ops = plan["values"], {op["out"]: op for op in plan["ops"]}
        ps = vals[s]
        pitch = d.terms[s] * dl
        assert ps["region"] and ps["addressable"] and ps["parent"] < 0 and ps["pitch"] == pitch, ps
        assert not any(op["elided"] for op in plan["ops"])
        hoist = bool(flags & HOIST)

        def placed_at(v, parent, words):
            pv = vals[v]
            assert pv["parent"] == parent, (v, pv)
            assert pv["offset"] == ps["offset"] + words * 8, (v, pv, words)
            assert pv["pitch"] == pitch and pitch > d.terms[v] * dl, (v, pv)      # a real pitch: not the dense form

        def add_flags(v, placed_a, placed_b):
            op = ops[v]
            assert (op["placed_a"], op["placed_b"]) == (placed_a, placed_b), op
            # whatever is not placed is an input here: hoisted with HOIST, copied by the add without
            assert (op["hoist_a"], op["hoist_b"]) == (hoist and not placed_a, hoist and not placed_b), op

        t = self.in_terms
        if self.kind == "right":
            placed_at(self.products[0], s, 0)
            add_flags(s, True, False)
        elif self.kind == "left":
            placed_at(self.products[0], s, t[2] * dl)
            add_flags(s, False, True)
        elif self.kind == "both":
            placed_at(self.products[0], s, 0)
            placed_at(self.products[1], s, t[0] * t[1] * dl)
            add_flags(s, True, True)
        elif self.kind == "nested":
            placed_at(self.inner, s, 0)
            placed_at(self.products[0], self.inner, 0)          # the parent is the inner sum, the pitch the outer one's
            add_flags(self.inner, True, False)
            add_flags(s, True, False)
        else:
            placed_at(self.inner, s, 0)
            add_flags(self.inner, False, False)
            add_flags(s, True, False)
        placed, hoisted, _ = self.expected_counts(flags)
        assert sum(op["placed_a"] + op["placed_b"] for op in plan["ops"]) == placed
        assert sum(op["hoist_a"] + op["hoist_b"] for op in plan["ops"]) == hoisted


_expected = {}


def expected(circ):
    """Inputs (every one from a seed of its own, so that no two slices hold equal words) and every value of the
    circuit in numpy, computed once per (kind, n, batch, terms) and never written again."""
    key = (circ.kind, circ.n, circ.batch, circ.in_terms)
    if key not in _expected:
        inputs = {v: rand_terms(circ.n, circ.batch, t, 7001 + 1000 * k + t)
                  for k, (v, t) in enumerate(zip(circ.ins, circ.in_terms))}
        vals = evaluate(circ.d, inputs)
        for a in vals:
            a.flags.writeable = False
        _expected[key] = (inputs, vals)
    return _expected[key]


# -- shapes of the placed product: (N, t1, t2, batch) ------------------------------------------------------------------
# U units per term: 10 sixteen-byte units at N = 1247, 32 at N = 4096, 21 EIGHT-byte units at N = 1300 (dL odd).
# CU = t2 * U units per row, PU = t1 * CU per product; B = 256 * units per lane is one workgroup's units.
SHAPES = {
    "BENCH_ROWS": (1247, 2, 128, 3),       # CU 1280, PU 2560: rows of 5 whole workgroups; no workgroup crosses a pair at MF 1, 2
    "ONE_BLOCK_ROWS": (4096, 3, 8, 4),     # CU 256, PU 768
    "CROSSING": (1247, 3, 26, 5),          # CU 260, PU 780: every workgroup crosses a row, most a pair; partial last one
    "TALL_1247": (1247, 191, 2, 3),        # CU 20, PU 3820: config 5's products
    "TALL_4096": (4096, 95, 2, 3),         # CU 64, PU 6080
    "PU_256": (4096, 4, 2, 5),             # PU 256, 512, 260: either side of PU >= B at MF 1 and 2
    "PU_512": (4096, 8, 2, 5),
    "PU_260": (1247, 13, 2, 7),
    "ODD_DL": (1300, 2, 13, 3),            # 8-byte units: CU 273, PU 546
    "LONG_520": (1247, 2, 52, 3),          # CU 520, PU 1040: long rows at MF 2 whose workgroups cross pairs
    "LONG_2080": (4096, 2, 65, 3),         # CU 2080, PU 4160: long rows at MF 8, pairs crossed
    "SHORT_PF": (1247, 8, 26, 3),          # CU 260, PU 2080: short rows WITH the prefetch at MF 4 and 8
    "ODD_SHORT": (1300, 4, 5, 3),          # 8-byte units: CU 105, PU 420: short rows at MF 1
    "ODD_LONG": (1300, 2, 25, 3),          # 8-byte units: CU 525, PU 1050: long rows at MF 2
    "ONE_1247": (1247, 1, 1, 5),           # 1 x 1 with a pitch: not the dense stream kernel
    "ONE_4096": (4096, 1, 1, 5),
    "ONE_1300": (1300, 1, 1, 5),
    "TWO_1247": (1247, 2, 2, 5),
    "SMALL_TILED_64": (1247, 5, 4, 3),     # default dispatch: the tiled kernel with 64 / 128 threads and 8 left terms
    "SMALL_TILED_128": (4096, 8, 4, 3),
}
# prefetch distance (KiB) of two rows, as in test_mul_flat_block_index: the first rows prefetch rows of the launch, the
# last two would reach past it
PF_KB = {"BENCH_ROWS": 32, "CROSSING": 8, "ODD_DL": 4, "LONG_520": 16, "LONG_2080": 64, "SHORT_PF": 8, "ODD_LONG": 8}
TC = (1, 3, 40)        # terms of the other operand: a skip of 10 to 400 units at N = 1247; odd: 8 bytes off at N = 1300


def knobs_of(shape, setting):
    """'f2' mul_flat 2 behind the touch pass; 'f2x0' the same with mul_xcd 0; 'f2t0' touch off (the prefetch at its
    default distance); 'f2pf' touch off and a prefetch distance of two rows; 'tiled' mul_flat -1; 'default' nothing."""
    if setting == "default":
        return {}
    if setting == "tiled":
        return {"mul_flat": -1}
    k = {"mul_flat": int(setting[1]), "mul_xcd": 1, "mul_touch": 3}
    tail = setting[2:]
    if tail == "x0":
        k["mul_xcd"] = 0
    elif tail == "t0":
        k["mul_touch"] = 0
    elif tail == "pf":
        k["mul_touch"] = 0
        k["mul_pf_kb"] = PF_KB[shape]
    else:
        assert tail == "", setting
    return k


def units(n):
    """(unit bytes, units per term) of a placed product: the circuit's offsets and pitches are multiples of dL words."""
    dl = (n + 63) // 64
    return (16, dl // 2) if dl % 2 == 0 else (8, dl)


def instantiation(shape, setting):
    """The launcher's predicates, restated: which kernel form the product of `shape` takes under `setting`."""
    n, t1, t2, batch = SHAPES[shape]
    w, U = units(n)
    CU, PU = t2 * U, t1 * t2 * U
    assert batch * (t1 + t2) * U * w < (4 << 20)                # far from a streaming call: mul_plan's small branch
    k = knobs_of(shape, setting)
    mf = k.get("mul_flat", 0)
    if mf == 0:                                                 # mul_plan with every knob at its default
        if w == 16 and CU <= 128 and ((t1 >= 4 and t2 >= 4 and 32 <= CU < 128) or (t1 >= 8 and CU == 128)):
            return "tiled%d bs%d" % (w, 64 if CU <= 64 else 128)
        if CU < (128 if w == 16 else 64):
            mf, touch = (2 if t1 >= 4 else 1), False
        else:
            return "tiled%d" % w
    elif mf < 0:
        return "tiled%d" % w
    else:
        touch = k["mul_touch"] > 0
    B = 256 * mf
    if PU < B:
        return "flat%d MF%d" % (w, mf)
    pf = (not touch) and CU >= 256 and k.get("mul_pf_kb", -1) != 0
    return "blk%d MF%d %s%s" % (w, mf, "long" if CU >= B else "short", " PF" if pf else "")


def crosses_a_pair(shape, setting):
    """Some workgroup of k_mul_flat_blk holds units of two products: the lanes past the pair's end take the skip."""
    n, t1, t2, batch = SHAPES[shape]
    inst = instantiation(shape, setting)
    if not inst.startswith("blk"):
        return False
    B = 256 * int(inst.split()[1][2:])
    return batch > 1 and (t1 * t2 * units(n)[1]) % B != 0


def host_kernel_name(shape, setting):
    """What csgn_mul_uniform_kernel answers under the setting's knobs (the 1 x 1 answer is the dense form's)."""
    n, t1, t2, _ = SHAPES[shape]
    inst = instantiation(shape, setting)
    if t1 == 1 and t2 == 1:
        return "k_and_stream"
    if inst.startswith("tiled"):
        return "k_mul_tiled"
    return "k_touch+k_mul_flat" if knobs_of(shape, setting).get("mul_touch", -1) > 0 else "k_mul_flat"


# The kernel form every case is MEANT to run: a literal table, asserted against instantiation() case by case.
_GRID = ("f1", "f1x0", "f2", "f2x0", "f4", "f4x0", "f8", "f8x0")
TABLE = {
    "CROSSING": {"f1": "blk16 MF1 long", "f1x0": "blk16 MF1 long", "f2": "blk16 MF2 short", "f2x0": "blk16 MF2 short",
                 "f4": "flat16 MF4", "f4x0": "flat16 MF4", "f8": "flat16 MF8", "f8x0": "flat16 MF8",
                 "f1t0": "blk16 MF1 long PF", "f2t0": "blk16 MF2 short PF", "f1pf": "blk16 MF1 long PF",
                 "f2pf": "blk16 MF2 short PF", "tiled": "tiled16", "default": "tiled16"},
    "ODD_DL": {"f1": "blk8 MF1 long", "f1x0": "blk8 MF1 long", "f2": "blk8 MF2 short", "f2x0": "blk8 MF2 short",
               "f4": "flat8 MF4", "f4x0": "flat8 MF4", "f8": "flat8 MF8", "f8x0": "flat8 MF8",
               "f1t0": "blk8 MF1 long PF", "f2t0": "blk8 MF2 short PF", "f1pf": "blk8 MF1 long PF",
               "f2pf": "blk8 MF2 short PF", "tiled": "tiled8", "default": "tiled8"},
    "TALL_1247": {"f1": "blk16 MF1 short", "f1x0": "blk16 MF1 short", "f2": "blk16 MF2 short", "f2x0": "blk16 MF2 short",
                  "f4": "blk16 MF4 short", "f4x0": "blk16 MF4 short", "f8": "blk16 MF8 short", "f8x0": "blk16 MF8 short",
                  "f1t0": "blk16 MF1 short", "tiled": "tiled16", "default": "blk16 MF2 short"},
    "BENCH_ROWS": {"f1": "blk16 MF1 long", "f2": "blk16 MF2 long", "f4": "blk16 MF4 long", "f8": "blk16 MF8 short",
                   "f1t0": "blk16 MF1 long PF", "f2t0": "blk16 MF2 long PF", "f4t0": "blk16 MF4 long PF",
                   "f8t0": "blk16 MF8 short PF", "f1pf": "blk16 MF1 long PF", "f2pf": "blk16 MF2 long PF",
                   "tiled": "tiled16", "default": "tiled16"},
    "ONE_BLOCK_ROWS": {"f1": "blk16 MF1 long", "f1t0": "blk16 MF1 long PF", "f2": "blk16 MF2 short",
                       "f2t0": "blk16 MF2 short PF", "f4": "flat16 MF4", "default": "tiled16"},
    "TALL_4096": {"f1": "blk16 MF1 short", "f2": "blk16 MF2 short", "f8": "blk16 MF8 short", "f1t0": "blk16 MF1 short",
                  "default": "blk16 MF2 short"},
    "PU_256": {"f1": "blk16 MF1 short", "f2": "flat16 MF2", "default": "flat16 MF2"},
    "PU_512": {"f1": "blk16 MF1 short", "f2": "blk16 MF2 short", "f4": "flat16 MF4", "default": "blk16 MF2 short"},
    "PU_260": {"f1": "blk16 MF1 short", "f2": "flat16 MF2", "default": "flat16 MF2"},
    "LONG_520": {"f1": "blk16 MF1 long", "f2": "blk16 MF2 long", "f2t0": "blk16 MF2 long PF", "f2pf": "blk16 MF2 long PF",
                 "f4": "blk16 MF4 short", "f4t0": "blk16 MF4 short PF"},
    "LONG_2080": {"f4": "blk16 MF4 long", "f4t0": "blk16 MF4 long PF", "f8": "blk16 MF8 long", "f8t0": "blk16 MF8 long PF",
                  "f8pf": "blk16 MF8 long PF", "tiled": "tiled16"},
    "SHORT_PF": {"f4": "blk16 MF4 short", "f4t0": "blk16 MF4 short PF", "f4pf": "blk16 MF4 short PF",
                 "f8": "blk16 MF8 short", "f8t0": "blk16 MF8 short PF", "f8pf": "blk16 MF8 short PF"},
    "ODD_SHORT": {"f1": "blk8 MF1 short", "f2": "flat8 MF2", "default": "tiled8"},
    "ODD_LONG": {"f1": "blk8 MF1 long", "f2": "blk8 MF2 long", "f2t0": "blk8 MF2 long PF", "f2pf": "blk8 MF2 long PF",
                 "f4": "blk8 MF4 short", "f4t0": "blk8 MF4 short PF"},
    "ONE_1247": {"f1": "flat16 MF1", "default": "flat16 MF1", "tiled": "tiled16"},
    "ONE_4096": {"f1": "flat16 MF1", "default": "flat16 MF1"},
    "ONE_1300": {"f1": "flat8 MF1", "default": "flat8 MF1", "tiled": "tiled8"},
    "TWO_1247": {"f1": "flat16 MF1", "default": "flat16 MF1", "tiled": "tiled16"},
    "SMALL_TILED_64": {"default": "tiled16 bs64"},
    "SMALL_TILED_128": {"default": "tiled16 bs128"},
}
PRODUCT_CASES = [(shape, setting) for shape, row in TABLE.items() for setting in row]
assert all(TABLE[s].keys() >= set(_GRID) for s in ("CROSSING", "ODD_DL", "TALL_1247"))


def product_terms(kind, shape, tc):
    """Input term counts of a product circuit.  `both`: the second product has the first one's shape (other words), so
    both run the case's kernel form and the second starts PU units into the element; `nested`: d has two terms."""
    _, t1, t2, _ = SHAPES[shape]
    return {"right": (t1, t2, tc), "left": (t1, t2, tc), "both": (t1, t2, t1, t2), "nested": (t1, t2, tc, 2)}[kind]


# (kind, flags, tc) run for every (shape, setting): `right` / `left` with every skip, with and without the prologue
PRODUCT_RUNS = ([(kind, flags, tc) for kind in ("right", "left") for flags in FLAGS for tc in TC] +
                [("both", flags, 0) for flags in FLAGS] + [("nested", flags, TC[1]) for flags in FLAGS])


def check_table_coverage():
    """Every kernel form the issue lists has a case.  16-byte units: all 15 reachable (LONG, PF, MF) of k_mul_flat_blk
    (short rows with the prefetch need 256 <= CU < 256 * MF: none at MF 1), each also by a case whose workgroups cross
    a pair; 8-byte units: {long, short} x MF {1, 2}; k_mul_flat on both sides of PU = B; the tiled kernel; 1 x 1; 2 x 2."""
    got = {}
    for shape, setting in PRODUCT_CASES:
        got.setdefault(TABLE[shape][setting], []).append((shape, setting))
    want16 = ["blk16 MF%d %s%s" % (mf, rows, pf) for mf in (1, 2, 4, 8) for rows in ("long", "short") for pf in ("", " PF")
              if not (mf == 1 and rows == "short" and pf)]
    assert len(want16) == 15
    want8 = ["blk8 MF%d %s" % (mf, rows) for mf in (1, 2) for rows in ("long", "short")]
    for inst in want16 + want8:
        assert inst in got, "no case runs " + inst
        assert any(crosses_a_pair(*c) for c in got[inst]), "no case of " + inst + " has a workgroup that crosses a pair"
    for inst in ("flat16 MF1", "flat16 MF2", "flat8 MF2", "tiled16", "tiled8", "tiled16 bs64", "tiled16 bs128"):
        assert inst in got, "no case runs " + inst
    # PU = B exactly and just above it take k_mul_flat_blk, PU < B k_mul_flat, at one and two units per lane
    assert TABLE["PU_256"]["f1"].startswith("blk") and TABLE["PU_260"]["f1"].startswith("blk")
    assert TABLE["PU_512"]["f2"].startswith("blk") and TABLE["PU_260"]["f2"].startswith("flat")
    assert TABLE["PU_256"]["f2"].startswith("flat") and TABLE["PU_512"]["f4"].startswith("flat")
    for one in ("ONE_1247", "ONE_4096", "ONE_1300"):
        assert SHAPES[one][1:3] == (1, 1) and {"f1", "default"} <= set(TABLE[one])
    assert SHAPES["TWO_1247"][1:3] == (2, 2) and {"f1", "default"} <= set(TABLE["TWO_1247"])
    return got


# -- sums and copies: (N, batch, T) ------------------------------------------------------------------------------------
# The launch under test moves batch * T * U units: a multiple of 256, and the nearest totals below and above that
# whole terms allow (16-byte units: 2 and 32 units off; 8-byte units at N = 1300: ONE unit off, 21 * 195 = 16 * 256 - 1
# and 21 * 573 = 47 * 256 + 1) -- the last workgroup of k_add_flat and of an entry of k_copy_list.
SUM_SHAPES = [(1247, 4, 32), (1247, 3, 17), (1247, 7, 11),
              (4096, 4, 4), (4096, 3, 5), (4096, 3, 3),
              (1300, 4, 64), (1300, 3, 65), (1300, 3, 191)]
SUM_EDGES = {(1247, 4, 32): 0, (1247, 3, 17): -2, (1247, 7, 11): 2, (4096, 4, 4): 0, (4096, 3, 5): -32, (4096, 3, 3): 32,
             (1300, 4, 64): 0, (1300, 3, 65): -1, (1300, 3, 191): 1}
SUM_KINDS = ("sum_in_sum", "nested", "right", "left")


def sum_terms(kind, T):
    """sum_in_sum: a + b has T terms (unequal halves) and so has c; the others: a 2 x 3 product and copies of T terms."""
    if kind == "sum_in_sum":
        ta = max(1, T // 3)
        return (ta, T - ta, T)
    return {"nested": (2, 3, T, T), "right": (2, 3, T), "left": (2, 3, T)}[kind]


def check_sum_edges():
    for (n, batch, T), edge in SUM_EDGES.items():
        total = batch * T * units(n)[1]
        assert (total - edge) % 256 == 0 and total > 256, (n, batch, T)


# HOIST: three inputs of different sizes in ONE prologue launch (several entries, the first[] search); at N = 1300 an
# entry is 16 bytes wide only if its words, pitches and addresses are all even: (2, 3, 5) mixes a wide entry with two
# narrow ones, (4, 2, 6) is all wide, (1, 2, 4) all narrow (an odd pitch)
HOIST_SHAPES = [(n, batch, sum_terms("sum_in_sum", T)) for n, batch, T in SUM_SHAPES] + \
               [(1300, 3, (2, 3, 5)), (1300, 5, (4, 2, 6)), (1300, 3, (1, 2, 4)), (1247, 3, (1, 40, 2)), (4096, 5, (3, 1, 9))]
