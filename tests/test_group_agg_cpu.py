"""CPU suite of the grouped aggregation: the Python model (tests/group_agg_model.py) against hand-written tables whose expected outputs
were typed by hand (tests/golden/group_agg_cases.json), and the three bindings of the new entry points -- header, ctypes, Rust."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import group_agg_model as M
from rivulus_amd import capi
from rivulus_amd.capi import AGG_OPS, RvAggSpec  # absent without the feature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "group_agg_cases.json")))["cases"]


def test_there_are_a_dozen_hand_written_cases():
    assert len(CASES) >= 12 and len({c["name"] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_against_hand_written_tables(case):
    key = M.column_of("i64", case["key"])
    cols = [M.column_of(c["dtype"], c["cells"]) for c in case["columns"]]
    got = M.aggregate((key[1], key[2]), cols, [tuple(s) for s in case["specs"]])
    exp = case["expect"]
    assert got["groups"] == len(exp["first_row"])
    assert got["first_row"].tolist() == exp["first_row"]
    assert got["gids"].tolist() == exp["gids"]
    assert [int(v) if ok else None for v, ok in zip(got["key_values"], got["key_valid"])] == exp["key"]
    assert len(got["aggs"]) == len(exp["aggs"])
    for j, (agg, want) in enumerate(zip(got["aggs"], exp["aggs"])):
        assert agg[0] == want["dtype"], j
        assert M.agg_cells(agg) == M.expected_cells(want["dtype"], want["cells"]), (j, case["specs"][j])


def test_order_map_is_monotonic_and_round_trips():
    cells = [-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, np.inf]
    bits = np.array(cells, np.float64).view(np.uint64)
    for is_max in (False, True):
        keys = [int(k) for k in M.order_key(bits, True, is_max)]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        assert [M.order_value(k, True) for k in keys] == [int(b) for b in bits]
    nan = np.array([np.nan, -np.nan], np.float64).view(np.uint64)
    assert [int(k) for k in M.order_key(nan, True, False)] == [0, 0] and [int(k) for k in M.order_key(nan, True, True)] == [2 ** 64 - 1] * 2
    ints = np.array([-2 ** 63, -1, 0, 1, 2 ** 63 - 1], np.int64).view(np.uint64)
    keys = [int(k) for k in M.order_key(ints, False, False)]
    assert keys == sorted(keys) and [M.order_value(k, False) for k in keys] == [int(b) for b in ints]


def test_float_sum_and_gamma_bound():
    assert M.float_sum([]) == 0.0 and np.signbit(M.float_sum([-0.0])) == False  # noqa: E712
    assert M.float_sum([1e16, 1.0, -1e16]) == 1.0
    assert np.isnan(M.float_sum([np.inf, -np.inf])) and M.float_sum([np.inf, 1.0]) == np.inf
    assert M.gamma_bound([1.0]) == 0 and M.gamma_bound([1.0, 2.0]) == M.U / (1 - M.U) * 3


def test_bindings_exist():
    for name in ("rv_group_ids", "rv_hash_aggregate"):
        assert name in capi.PROTOTYPES
        assert getattr(ctypes.CDLL(capi.LIB_PATH), name) is not None
    assert ctypes.sizeof(RvAggSpec) == 8 and RvAggSpec.col.offset == 4
    assert AGG_OPS == {"count_rows": 0, "count": 1, "sum": 2, "min": 3, "max": 4}
    assert hasattr(capi.Context, "hash_aggregate") and hasattr(capi.Context, "group_ids")
    header = open(os.path.join(ROOT, "include", "rivulus_gpu.h")).read()
    assert "#define RV_ABI_VERSION 4" in header, "additive only"
    for k, v in AGG_OPS.items():
        assert f"RV_AGG_{k.upper()} = {v}" in header


def test_rust_declarations_are_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "rust_shim", "ffi.rs")).read()
    assert "pub fn rv_hash_aggregate(" in text and "pub fn rv_group_ids(" in text
    assert "pub struct RvAggSpec {" in text and "pub const RV_AGG_MAX: c_int = 4;" in text
