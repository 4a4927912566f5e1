"""CPU suite of grouping by several key columns: the Python model (tests/group_keys_model.py) against hand-written tables whose expected
outputs were typed by hand (tests/golden/group_keys_cases.json), and the bindings of the two new entry points -- header, ctypes, the
library's symbols, Rust."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import group_agg_model as M
import group_keys_model as K
from rivulus_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "group_keys_cases.json")))["cases"]
NEW = ("rv_group_ids_keys", "rv_hash_aggregate_keys")


def test_there_are_a_dozen_hand_written_cases():
    assert len(CASES) >= 12 and len({c["name"] for c in CASES}) == len(CASES)
    names = " ".join(c["name"] for c in CASES)
    for must in ("four_null_and_zero", "one_two_is_not_two_one", "nan", "minus_zero", "boolean_times_int64", "three_keys", "null_typed_key", "zero_rows"):
        assert must in names, must


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_against_hand_written_tables(case):
    n = case["rows"]
    keys = [K.key_column_of(k["dtype"], k.get("cells"), n) for k in case["keys"]]
    cols = [M.column_of(c["dtype"], c["cells"]) for c in case["columns"]]
    assert K.rows_of(keys) == n and all(len(c[1]) == n for c in cols)
    got = K.aggregate(keys, cols, [tuple(s) for s in case["specs"]])
    exp = case["expect"]
    assert got["groups"] == len(exp["first_row"])
    assert got["first_row"].tolist() == exp["first_row"]
    assert got["gids"].tolist() == exp["gids"]
    assert len(exp["keys"]) == len(keys)
    for k, (key, want) in enumerate(zip(keys, exp["keys"])):
        assert key[0] == want["dtype"]
        assert K.canonical_key_cells(key[0], got["key_cells"][k]) == K.expected_key_cells(want["dtype"], want["cells"]), f"key column {k}"
    assert len(got["aggs"]) == len(exp["aggs"])
    for j, (agg, want) in enumerate(zip(got["aggs"], exp["aggs"])):
        assert agg[0] == want["dtype"], j
        assert M.agg_cells(agg) == M.expected_cells(want["dtype"], want["cells"]), (j, case["specs"][j])


def test_cell_equality():
    f = lambda bits: np.array(bits, np.uint64).view(np.float64)  # noqa: E731
    nans = f([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FF800000000BEEF])
    assert {K.cell("f64", nans, None, i) for i in range(5)} == {K.CANONICAL_NAN}
    zeros = np.array([0.0, -0.0])
    assert K.cell("f64", zeros, None, 0) != K.cell("f64", zeros, None, 1)
    inf = f([0x7FF0000000000000, 0xFFF0000000000000])
    assert K.cell("f64", inf, None, 0) == 0x7FF0000000000000 and K.cell("f64", inf, None, 1) == 0xFFF0000000000000  # not NaNs
    ints = np.array([-1, 0], np.int64)
    assert K.cell("i64", ints, None, 0) == 2 ** 64 - 1
    assert K.cell("i64", ints, np.array([False, True]), 0) is None and K.cell("i64", ints, np.array([False, True]), 1) == 0
    assert K.cell("bool", np.array([True, False]), None, 0) == 1 and K.cell("bool", np.array([True, False]), None, 1) == 0
    assert K.cell("null", None, 5, 3) is None


def test_one_int64_key_is_the_single_key_model():
    rng = np.random.default_rng(1)
    n = 500
    key = rng.integers(-5, 5, n, dtype=np.int64)
    valid = rng.random(n) > 0.2
    cols = [("i64", rng.integers(-100, 100, n, dtype=np.int64), rng.random(n) > 0.3)]
    specs = [("sum", 0), ("min", 0), ("count_rows", None)]
    a = K.aggregate([("i64", key, valid)], cols, specs)
    b = M.aggregate((key, valid), cols, specs)
    assert a["gids"].tolist() == b["gids"].tolist() and a["first_row"].tolist() == b["first_row"].tolist()
    assert [M.agg_cells(x) for x in a["aggs"]] == [M.agg_cells(x) for x in b["aggs"]]


def test_bindings_exist():
    header = open(os.path.join(ROOT, "include", "rivulus_gpu.h")).read()
    assert "#define RV_ABI_VERSION 4" in header, "additive only"
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert f"rv_status {name}(rv_ctx *ctx, const rv_dcolumn *const *keys, uint32_t nkeys," in header
        assert name in capi.PROTOTYPES
        assert getattr(lib, name) is not None
    assert capi.load().rv_abi_version() == 4
    assert len(capi.PROTOTYPES["rv_group_ids_keys"][1]) == 6 and len(capi.PROTOTYPES["rv_hash_aggregate_keys"][1]) == 10
    assert hasattr(capi.Context, "hash_aggregate_keys") and hasattr(capi.Context, "group_ids_keys")
    # the single-key entry points keep their prototypes
    assert len(capi.PROTOTYPES["rv_group_ids"][1]) == 5 and len(capi.PROTOTYPES["rv_hash_aggregate"][1]) == 9
    # the normative text states the Float64 and the null rules
    at = header.index("(K9a)")
    text = " ".join(header[at:header.index("rv_status rv_group_ids_keys(")].split())
    for phrase in ("every other NaN", "-0.0 and +0.0 are DIFFERENT keys", "never read as a value", "no special null group", "group_ids<keys>"):
        assert phrase in text, phrase


def _tests_c_digest():
    d = os.path.join(ROOT, "tests", "c")
    return {f: hashlib.sha256(open(os.path.join(d, f), "rb").read()).hexdigest() for f in sorted(os.listdir(d))}


def test_rust_declarations_are_current_and_the_layouts_stay(tmp_path):
    before = _tests_c_digest()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert _tests_c_digest() == before, "the generator leaves the C layout files as they are"
    text = open(os.path.join(ROOT, "rust_shim", "ffi.rs")).read()
    assert "pub fn rv_hash_aggregate_keys(ctx: *mut RvCtx, keys: *const *const RvDcolumn, nkeys: u32," in text
    assert "pub fn rv_group_ids_keys(ctx: *mut RvCtx, keys: *const *const RvDcolumn, nkeys: u32," in text
    assert "pub const RV_ABI_VERSION: u32 = 4;" in text
    # no new struct: the layouts tests/c/abi_check.c pins still compile against the header
    src = os.path.join(ROOT, "tests", "c", "abi_check.c")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-DRV_ABI_LAYOUT_ONLY", "-c", src, "-o", str(tmp_path / "abi_check.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
