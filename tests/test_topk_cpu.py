"""CPU suite of top-k: the numpy model (tests/topk_model.py) against tables typed by hand (tests/golden/topk_cases.json), the select
model's candidate set on random inputs (closed downward in the sort order, and holding the answer), the three bindings of the new entry
points -- header, ctypes, Rust -- and the select's decisions (rivulus_amd/csrc/topk_rule.hpp) under the sanitizers as a stand-alone program."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import sort_model as M
import topk_model as T
from rivulus_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = json.load(open(os.path.join(ROOT, "tests", "golden", "topk_cases.json")))
CASES, FRAMES = DOC["cases"], DOC["frames"]


def test_there_are_a_dozen_hand_written_cases():
    names = [c["name"] for c in CASES + FRAMES]
    assert len(CASES) >= 12 and len(FRAMES) >= 1 and len(set(names)) == len(names) and all(c["why"] for c in CASES + FRAMES)
    assert {c["selected"] for c in CASES} == {True, False} and max(c["passes"] for c in CASES) == 8


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_against_hand_written_tables(case):
    col = M.column_of(case["dtype"], case["cells"])
    got = T.top_k_indices(col, case["flags"], case["k"])
    assert got.dtype == np.int64 and got.tolist() == case["expect"], case["why"]
    s = T.select(col, case["flags"], case["k"], 1, case["divisor"])
    assert (s.selected, s.passes, s.candidates.tolist()) == (case["selected"], case["passes"], case["candidates"]), case["why"]
    assert s.count == len(case["candidates"])


@pytest.mark.parametrize("case", FRAMES, ids=[c["name"] for c in FRAMES])
def test_model_of_a_frame(case):
    cols = [M.column_of(c["dtype"], c["cells"]) for c in case["columns"]]
    keys = [tuple(k) for k in case["keys"]]
    assert T.top_k_frame(cols, keys, case["k"]).tolist() == case["expect"], case["why"]
    s = T.select(cols[keys[0][0]], keys[0][1], case["k"], 1, case["divisor"])
    assert (s.selected, s.passes, s.candidates.tolist()) == (case["selected"], case["passes"], case["candidates"])
    # the candidates' rows, sorted by every key among themselves, give the same answer: nothing outside them can matter
    sub = [(c[0], c[1][s.candidates], None if c[2] is None else c[2][s.candidates]) for c in cols]
    assert s.candidates[M.sort_frame(sub, keys)][:case["k"]].tolist() == case["expect"]


def random_column(rng):
    n = int(rng.integers(0, 400))
    card = int(rng.integers(1, max(2, n + 1)))
    pool = rng.integers(-(1 << 63), (1 << 63) - 1, card, dtype=np.int64) if rng.random() < 0.5 else rng.integers(-3, max(1, card), card)
    v = pool[rng.integers(0, card, n)] if n else np.zeros(0, np.int64)
    share = float(rng.choice([0.0, 0.0, 0.05, 0.5, 1.0]))
    valid = rng.random(n) >= share if share > 0 else None
    if rng.random() < 0.5:
        return ("f64", v.astype(np.int64).view(np.float64) if rng.random() < 0.5 else v.astype(np.float64), valid)
    return ("i64", v.astype(np.int64), valid)


def test_candidates_are_closed_downward_and_hold_the_answer():
    rng = np.random.default_rng(20)
    selected = 0
    for case in range(200):
        col = random_column(rng)
        n = len(col[1])
        flags = int(rng.integers(0, 4))
        k = int(rng.choice([0, 1, 2, 5, max(0, n // 2 - 1), n // 2, n, n + 1, int(rng.integers(0, n + 2))]))
        divisor = int(rng.choice([1, 2, 32, 1 << 40]))
        s = T.select(col, flags, k, 1, divisor)
        order = M.sort_indices(col, flags)
        want = order[:k]
        assert np.array_equal(T.top_k_indices(col, flags, k), want)
        assert np.all(np.diff(s.candidates) > 0), "ascending row ids"
        assert np.isin(want, s.candidates).all(), (case, "the answer lies inside the candidates")
        # closed downward: the candidates are a PREFIX of the sort, as a set ...
        assert np.array_equal(np.sort(order[:s.count]), s.candidates), case
        # ... that ends at a boundary between two different keys: no tie of the last candidate is left outside
        if s.selected and 0 < s.count < n:
            cls, keys = M.working_keys(col, flags)
            a, b = order[s.count - 1], order[s.count]
            assert (cls[a], keys[a]) != (cls[b], keys[b]), case
        # sorting the candidates alone gives the answer
        sub = (col[0], col[1][s.candidates], None if col[2] is None else col[2][s.candidates])
        assert np.array_equal(s.candidates[M.sort_indices(sub, flags)][:k], want), case
        assert s.passes == 0 or 1 <= s.passes <= 8
        selected += s.selected and s.passes > 0
    assert selected >= 40, "the random cases exercise the select, not only the fallback"


def test_stop_rule_in_the_model():
    rng = np.random.default_rng(21)
    col = ("i64", rng.integers(-(1 << 63), (1 << 63) - 1, 5000, dtype=np.int64), None)
    once = T.select(col, 0, 10, 1, 1)
    full = T.select(col, 0, 10, 1, 1 << 40)
    assert once.passes == 1 and full.passes == 8 and full.count == 10 and once.count >= full.count
    assert np.isin(full.candidates, once.candidates).all()


def test_bindings_exist():
    for name in ("rv_top_k_indices", "rv_top_k"):
        assert name in capi.PROTOTYPES
        assert getattr(ctypes.CDLL(capi.LIB_PATH), name) is not None
    assert hasattr(capi.Context, "top_k_indices") and hasattr(capi.Context, "top_k")
    header = open(os.path.join(ROOT, "include", "rivulus_gpu.h")).read()
    assert "#define RV_ABI_VERSION 4" in header, "additive only"
    assert "rv_status rv_top_k_indices(rv_ctx *ctx, const rv_dcolumn *key, uint32_t flags, uint64_t k, rv_dcolumn **out_indices);" in header
    assert "rv_status rv_top_k(" in header
    for option in ("top_k_select_from_rows", "top_k_refine_divisor", "top_k_last_passes", "top_k_last_candidates"):
        assert f'"{option}"' in header, option
    res, args = capi.PROTOTYPES["rv_top_k_indices"]
    assert res is ctypes.c_int and args[2] is ctypes.c_uint32 and args[3] is ctypes.c_uint64 and len(args) == 5
    res, args = capi.PROTOTYPES["rv_top_k"]
    assert len(args) == 8 and args[5] is ctypes.c_uint32 and args[6] is ctypes.c_uint64


def test_rust_declarations_are_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "rust_shim", "ffi.rs")).read()
    assert "pub fn rv_top_k_indices(" in text and "pub fn rv_top_k(" in text


def test_the_sort_s_pieces_are_shared_not_restated():
    csrc = os.path.join(ROOT, "rivulus_amd", "csrc")
    kernels = open(os.path.join(csrc, "topk_kernel.hpp")).read()
    assert '#include "sort_kernel.hpp"' in kernels and '#include "topk_rule.hpp"' in kernels
    assert "sort_cell_is_null(" in kernels and "sort_peers(" in kernels and "rvorder::sort_key(" in kernels
    unit = open(os.path.join(csrc, "topk.hip")).read()
    assert unit.count('check_sort_key(') >= 2 and "void check_sort_key" not in unit, "one check, the sort's"
    assert "rvt::kTopKRefineDivisor" in unit and "rvt::kTopKSelectFromRows" in unit
    assert " topk" in open(os.path.join(csrc, "Makefile")).read().split("UNITS =")[1].splitlines()[0]


def test_topk_rule_under_the_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "topk_rule_tests.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "topk_rule_tests")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, src], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 10000, r.stdout[-500:]
