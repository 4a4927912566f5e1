"""CPU suite of the sort: the numpy model (tests/sort_model.py) against tables whose expected permutations were typed by hand
(tests/golden/sort_cases.json), the three bindings of the new entry points -- header, ctypes, Rust -- and the shared order map
(rivulus_amd/csrc/order_key.hpp) under the sanitizers as a stand-alone program."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import sort_model as M
from rivulus_amd import capi
from rivulus_amd.capi import RV_SORT_DESCENDING, RV_SORT_NULLS_LAST  # absent without the feature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = json.load(open(os.path.join(ROOT, "tests", "golden", "sort_cases.json")))
CASES, FRAMES = DOC["cases"], DOC["frames"]


def test_there_are_a_dozen_hand_written_cases():
    names = [c["name"] for c in CASES + FRAMES]
    assert len(CASES) >= 12 and len(set(names)) == len(names) and all(c["why"] for c in CASES + FRAMES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_against_hand_written_tables(case):
    col = M.column_of(case["dtype"], case["cells"])
    got = M.sort_indices(col, case["flags"], case.get("prior"))
    assert got.dtype == np.int64 and got.tolist() == case["expect"], case["why"]


@pytest.mark.parametrize("case", FRAMES, ids=[c["name"] for c in FRAMES])
def test_model_chains_the_keys(case):
    cols = [M.column_of(c["dtype"], c["cells"]) for c in case["columns"]]
    keys = [tuple(k) for k in case["keys"]]
    assert M.sort_frame(cols, keys).tolist() == case["expect"], case["why"]
    assert M.lexsort_frame(cols, keys).tolist() == case["expect"], "np.lexsort over (class, key) says the same"


def test_model_order_map():
    cells = np.array([-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, np.inf])
    keys = [int(k) for k in M.order_key(cells.view(np.uint64), True)]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF], np.uint64)
    assert [int(k) for k in M.order_key(nans, True)] == [2 ** 64 - 1] * 4 and keys[-1] < 2 ** 64 - 1
    ints = np.array([-2 ** 63, -1, 0, 1, 2 ** 63 - 1], np.int64).view(np.uint64)
    ikeys = [int(k) for k in M.order_key(ints, False)]
    assert ikeys == sorted(ikeys) and len(set(ikeys)) == 5


def test_model_ignores_what_lies_under_nulls():
    rng = np.random.default_rng(5)
    valid = rng.random(200) >= 0.3
    a = rng.integers(-5, 5, 200)
    b = np.where(valid, a, rng.integers(-2 ** 62, 2 ** 62, 200))
    for flags in range(4):
        assert np.array_equal(M.sort_indices(("i64", a, valid), flags), M.sort_indices(("i64", b, valid), flags))


def test_bindings_exist():
    for name in ("rv_sort_indices", "rv_sort"):
        assert name in capi.PROTOTYPES
        assert getattr(ctypes.CDLL(capi.LIB_PATH), name) is not None
    assert (RV_SORT_DESCENDING, RV_SORT_NULLS_LAST) == (M.DESCENDING, M.NULLS_LAST) == (1, 2)
    assert hasattr(capi.Context, "sort_indices") and hasattr(capi.Context, "sort")
    header = open(os.path.join(ROOT, "include", "rivulus_gpu.h")).read()
    assert "#define RV_ABI_VERSION 4" in header, "additive only"
    assert "#define RV_SORT_DESCENDING 1u" in header and "#define RV_SORT_NULLS_LAST 2u" in header
    res, args = capi.PROTOTYPES["rv_sort_indices"]
    assert res is ctypes.c_int and args[2] is ctypes.c_uint32 and len(args) == 5
    res, args = capi.PROTOTYPES["rv_sort"]
    assert len(args) == 7 and args[2] is ctypes.c_uint32 and args[5] is ctypes.c_uint32


def test_rust_declarations_are_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "rust_shim", "ffi.rs")).read()
    assert "pub fn rv_sort_indices(" in text and "pub fn rv_sort(" in text
    assert "pub const RV_SORT_DESCENDING: u32 = 1;" in text and "pub const RV_SORT_NULLS_LAST: u32 = 2;" in text


def test_the_order_map_is_shared_not_restated():
    """group_agg_kernel.hpp and sort_kernel.hpp both go through order_key.hpp"""
    csrc = os.path.join(ROOT, "rivulus_amd", "csrc")
    for name in ("group_agg_kernel.hpp", "sort_kernel.hpp"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "order_key.hpp"' in text and "rvorder::" in text, name


def test_order_key_under_the_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "sort_key_tests.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sort_key_tests")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, src], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 100000, r.stdout[-500:]
