"""CPU suite of arithmetic expressions: the model (tests/arith_model.py) against hand-worked cells, and the cell functions the
device kernel is built from (rivulus_amd/csrc/arith_cell.hpp, compiled here with g++) against the model, bit for bit, over a
million edge and random cells per run."""
import itertools
import math
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import arith_model as M
from rivulus_amd import capi
from rivulus_amd.capi import RV_BOOLEAN, RV_FLOAT64, RV_INT64, RV_NULL, RV_STRING

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "arith_cell_fuzz.cpp")
MIN, MAX = M.I64_MIN, M.I64_MAX
CELLS_PER_BLOCK = 65536  # x 16 blocks (4 type pairs x 4 operators) = 1 048 576 cells


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("arith") / "arith_cell_fuzz")
    # the contraction flag is the device unit's; on the host it keeps g++ from fusing anything it could see through
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-o", exe, SRC], check=True)
    return exe


# ---- the model against hand-worked cells -------------------------------------------------------------------------------
def test_int64_wraps_in_twos_complement():
    assert M.cell_op("+", RV_INT64, MAX, 1) == MIN
    assert M.cell_op("-", RV_INT64, MIN, 1) == MAX
    assert M.cell_op("*", RV_INT64, MIN, -1) == MIN
    assert M.cell_op("*", RV_INT64, 1 << 32, 1 << 32) == 0
    assert M.cell_op("*", RV_INT64, MAX, 2) == -2


def test_int64_division_truncates_and_nulls_on_zero():
    assert M.cell_op("/", RV_INT64, -7, 2) == -3
    assert M.cell_op("/", RV_INT64, 7, -2) == -3
    assert M.cell_op("/", RV_INT64, -7, -2) == 3
    assert M.cell_op("/", RV_INT64, 5, 0) is None
    assert M.cell_op("/", RV_INT64, 0, 0) is None
    assert M.cell_op("/", RV_INT64, MIN, -1) == MIN
    assert M.cell_op("/", RV_INT64, MIN, 1) == MIN


def test_int64_meets_float64_rounded_to_nearest_even():
    assert M.to_f64((1 << 53) + 1) == 9007199254740992.0
    assert M.to_f64((1 << 53) + 3) == 9007199254740996.0
    assert M.to_f64(MAX) == 2.0 ** 63
    dtype, cells = M.evaluate(("+", ("col", 0), ("col", 1)), [RV_INT64, RV_FLOAT64], [[(1 << 53) + 1], [0.0]])
    assert dtype == RV_FLOAT64 and cells == [9007199254740992.0]


def test_float64_specials():
    assert M.cell_op("/", RV_FLOAT64, 1.0, 0.0) == math.inf
    assert M.cell_op("/", RV_FLOAT64, -1.0, 0.0) == -math.inf
    assert M.cell_op("/", RV_FLOAT64, 1.0, -0.0) == -math.inf
    assert math.isnan(M.cell_op("/", RV_FLOAT64, 0.0, 0.0))
    assert math.isnan(M.cell_op("-", RV_FLOAT64, math.inf, math.inf))
    sub = M.cell_op("*", RV_FLOAT64, 1e-200, 1e-120)  # a subnormal result, kept
    assert 0.0 < sub < 2.2250738585072014e-308 and M.f64_bits(sub) == M.f64_bits(1e-200 * 1e-120)
    assert M.cell_op("/", RV_FLOAT64, 5e-324, 2.0) == 0.0 and M.cell_op("/", RV_FLOAT64, 1.5e-323, 2.0) == 1e-323  # ties to even


def test_contraction_witness():
    """(a * b) + c with a = 1 + 2^-30, b = 1 - 2^-30, c = -1: the product 1 - 2^-60 rounds to 1.0, so two roundings give exactly
    0.0; a fused multiply-add keeps the exact product and gives -2^-60."""
    a, b, c = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0
    tree = ("+", ("*", ("col", 0), ("col", 1)), ("col", 2))
    dtype, cells = M.evaluate(tree, [RV_FLOAT64] * 3, [[a], [b], [c]])
    assert dtype == RV_FLOAT64 and M.f64_bits(cells[0]) == M.f64_bits(0.0)
    exact = Fraction(a) * Fraction(b) + Fraction(c)  # what one rounding at the end would return
    assert exact == -Fraction(1, 2 ** 60)


def test_nulls_propagate():
    tree = ("*", ("+", ("col", 0), ("lit", 1)), ("col", 1))
    _, cells = M.evaluate(tree, [RV_INT64, RV_INT64], [[1, None, 3], [None, 2, 4]])
    assert cells == [None, None, 16]
    dtype, cells = M.evaluate(("+", ("col", 0), ("lit", None)), [RV_FLOAT64], [[1.0, 2.0]])
    assert dtype == RV_FLOAT64 and cells == [None, None]
    dtype, cells = M.evaluate(("+", ("col", 0), ("col", 1)), [RV_NULL, RV_NULL], [[None] * 2, [None] * 2])
    assert dtype == RV_NULL and cells == [None, None]


TYPE_TABLE = {
    (RV_FLOAT64, RV_FLOAT64): RV_FLOAT64, (RV_FLOAT64, RV_INT64): RV_FLOAT64, (RV_INT64, RV_FLOAT64): RV_FLOAT64,
    (RV_FLOAT64, RV_NULL): RV_FLOAT64, (RV_NULL, RV_FLOAT64): RV_FLOAT64,
    (RV_INT64, RV_INT64): RV_INT64, (RV_INT64, RV_NULL): RV_INT64, (RV_NULL, RV_INT64): RV_INT64,
    (RV_NULL, RV_NULL): RV_NULL,
}


def test_type_table_of_the_model():
    for left, right in itertools.product(range(5), repeat=2):
        if RV_BOOLEAN in (left, right) or RV_STRING in (left, right):
            with pytest.raises(M.TypeMismatch):
                M.result_dtype(left, right)
        else:
            assert M.result_dtype(left, right) == TYPE_TABLE[left, right]


def test_type_table_of_the_header(fuzz_exe):
    r = subprocess.run([fuzz_exe, "types"], capture_output=True, text=True, check=True)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == 25
    for left, right, got in rows:
        want = TYPE_TABLE.get((left, right), -1)  # -1: a Boolean / String operand
        assert got == want, (left, right, got)


def test_postfix_of_a_tree():
    tree = ("/", ("col", 0), ("-", ("col", 1), ("lit", 1.5)))
    assert capi.arith_postfix(tree) == [("col", 0), ("col", 1), ("lit", 1.5), "-", "/"]
    steps = capi.arith_steps(capi.arith_postfix(tree))
    assert [s.op for s in steps] == [capi.RV_ARITH_COL, capi.RV_ARITH_COL, capi.RV_ARITH_LIT, capi.RV_ARITH_SUB, capi.RV_ARITH_DIV]
    assert steps[2].lit_type == RV_FLOAT64 and steps[2].lit.f == 1.5 and steps[1].column == 1


# ---- the header's cell functions against the model ---------------------------------------------------------------------
def _signed(u):
    return u - (1 << 64) if u >> 63 else u


def test_cell_functions_match_the_model_bit_for_bit(fuzz_exe, tmp_path):
    out = str(tmp_path / "cells.bin")
    r = subprocess.run([fuzz_exe, "cells", str(CELLS_PER_BLOCK), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(16 * CELLS_PER_BLOCK)], r.stdout + r.stderr
    data = np.fromfile(out, dtype="<u8").reshape(4, 4, CELLS_PER_BLOCK, 4)
    assert 16 * CELLS_PER_BLOCK >= 10 ** 6
    unpack, pack = struct.Struct("<d").unpack, struct.Struct("<Q").pack
    seen_null = seen_nan = seen_subnormal = 0
    for pair, (a_float, b_float) in enumerate([(False, False), (True, True), (False, True), (True, False)]):
        dtype = RV_FLOAT64 if a_float or b_float else RV_INT64
        for k, op in enumerate("+-*/"):
            for a, b, got, ok in data[pair, k].tolist():
                x = unpack(pack(a))[0] if a_float else _signed(a)
                y = unpack(pack(b))[0] if b_float else _signed(b)
                if dtype == RV_FLOAT64:
                    x = x if a_float else M.to_f64(x)
                    y = y if b_float else M.to_f64(y)
                want = M.cell_op(op, dtype, x, y)
                if want is None:
                    seen_null += 1
                    assert ok == 0 and got == 0, (pair, op, a, b, got, ok)
                    continue
                assert ok == 1, (pair, op, a, b)
                if dtype == RV_FLOAT64 and want != want:
                    seen_nan += 1
                    assert (got & 0x7FF0000000000000) == 0x7FF0000000000000 and got & 0x000FFFFFFFFFFFFF, (pair, op, a, b, got)
                    continue
                assert got == M.cell_bits(dtype, want), (pair, op, a, b, got, M.cell_bits(dtype, want))
                if dtype == RV_FLOAT64 and 0 < (got & 0x7FFFFFFFFFFFFFFF) < (1 << 52):
                    seen_subnormal += 1
    assert seen_null and seen_nan and seen_subnormal  # the generator reaches every special the rules name
