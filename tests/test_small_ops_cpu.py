"""The record of csgn_small_ops (include/csgn_hip.h) on a box without a GPU: the numpy layout the device tests build
record arrays with (tests/test_small_ops_gpu.py) is the C struct's, field for field."""
import os
import subprocess

from tests.model import SMALL_OP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_SRC = r"""
#include <cstddef>
#include <cstdio>
#include "csgn_hip.h"
#define F(f) std::printf(#f " %zu %zu\n", offsetof(csgn_small_op, f), sizeof(((csgn_small_op *)0)->f))
int main()
{
    std::printf("sizeof %zu %zu\n", sizeof(csgn_small_op), alignof(csgn_small_op));
    F(left); F(right); F(out); F(t1); F(t2); F(kind); F(reserved);
    return 0;
}
"""


def test_small_op_record_layout(tmp_path):
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text(LAYOUT_SRC)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    got = {ln.split()[0]: tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln}
    assert got.pop("sizeof") == (SMALL_OP.itemsize, 8) == (40, 8)            # size, alignment: arrays pack tightly
    assert got == {name: (SMALL_OP.fields[name][1], SMALL_OP.fields[name][0].itemsize) for name in SMALL_OP.names}
