"""CPU suite of the window frames (K12a): tests/window_frame_model.py against the hand-written tables of
tests/golden/window_frame_cases.json, against tests/window_model.py on the ops they share and against its own fast path; the three
bindings of rv_window_frames against each other; csrc/window_frame_rule.hpp under the sanitizers as a stand-alone program."""
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import window_frame_model as F
import window_model as M
from rivulus_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "window_frame_cases.json")) as f:
    CASES = json.load(f)["cases"]


def expr_of(e):
    if e["op"] in F.FRAME_OPS:
        return e["op"], e["col"], e["preceding"], e["following"]
    if e["op"] == "ntile":
        return "ntile", e["col"], e["buckets"]
    return e["op"], e["col"], e.get("offset", 0)


def frames_of(case):
    return [(e["preceding"], e["following"]) for e in case["exprs"] if e["op"] in F.FRAME_OPS]


def test_there_are_twenty_hand_written_cases_and_they_cover_the_ground():
    names = [c["name"] for c in CASES]
    assert len(CASES) >= 20 and len(set(names)) == len(names)
    ops = {e["op"] for c in CASES for e in c["exprs"]}
    assert ops >= set(capi.WINDOW_FRAME_OPS)
    frames = [fr for c in CASES for fr in frames_of(c)]
    assert any(p is None and f is not None for p, f in frames) and any(f is None and p is not None for p, f in frames) and (None, None) in frames
    assert any(p is not None and p < 0 for p, f in frames) and any(f is not None and f < 0 for p, f in frames)
    assert any(abs(v) == 1 << 62 for fr in frames for v in fr if v is not None)
    assert any(None in e["expected"] for c in CASES for e in c["exprs"])
    assert any(None in col["cells"] for c in CASES for col in c["columns"])
    assert any(cell in ("nan", "-0.0") for c in CASES for col in c["columns"] for cell in col["cells"])
    assert {col["dtype"] for c in CASES for col in c["columns"]} >= {"i64", "f64", "bool", "str"}
    ntiles = [(e["buckets"], len(e["expected"])) for c in CASES if not c["partition_by"] for e in c["exprs"] if e["op"] == "ntile"]
    assert any(n % b == 0 and 1 < b < n for b, n in ntiles) and any(n % b and b < n for b, n in ntiles)
    assert any(e["op"] == "ntile" and e["buckets"] > len(e["expected"]) for c in CASES for e in c["exprs"])
    assert any(c["partition_by"] and len(set(c["columns"][c["partition_by"][0]]["cells"])) == len(c["columns"][0]["cells"]) for c in CASES)  # partitions of length 1


def sums_only_integer_valued_floats(case):
    """what the model's fast path takes: every Float64 cell under a SUM / AVG is an integer"""
    return not any(c["dtype"] == "f64" and e["op"] in ("sum", "avg") and any(isinstance(x, str) or (x is not None and x != int(x)) for x in c["cells"])
                   for e in case["exprs"] for c in [case["columns"][e["col"]]])


TABLES = [(c, False) for c in CASES] + [(c, True) for c in CASES if sums_only_integer_valued_floats(c)]


@pytest.mark.parametrize("case,fast", TABLES, ids=[c["name"] + ("-fast" if f else "") for c, f in TABLES])
def test_model_against_hand_written_tables(case, fast):
    cols = [M.column_of(c["dtype"], c["cells"]) for c in case["columns"]]
    got = F.window_frames(cols, case["partition_by"], [tuple(k) for k in case["order_by"]], [expr_of(e) for e in case["exprs"]], exact_float=fast, fast=fast)
    for e, g in zip(case["exprs"], got):
        assert g[0] == e["dtype"], (e, g[0])
        assert M.same_cells(M.cells_of(g), M.expected_cells(e["dtype"], e["expected"])), f"{e['op']}: model {M.cells_of(g)}, table {e['expected']}"


def same_results(a, b):
    return a[0] == b[0] and np.array_equal(a[2], b[2]) and (a[1] is None and b[1] is None or np.array_equal(np.asarray(a[1]), np.asarray(b[1])))


def random_frame(rng, case):
    n = int(rng.integers(1, 40))
    mask = lambda: (rng.random(n) >= 0.3) if rng.random() < 0.7 else None
    cols = [("i64", rng.integers(0, 3, n), mask()), ("i64", rng.integers(-2, 3, n), mask()), ("i64", rng.integers(-9, 9, n), mask()),
            ("i64", rng.integers(0, 2, n), None), ("f64", rng.integers(-9, 9, n).astype(np.float64), mask()), ("bool", rng.random(n) < 0.5, mask()),
            ("str", [f"s{i % 4}" for i in range(n)], mask())]
    partition_by = [[], [0], [0, 3]][case % 3]
    order_by = [[], [(1, case % 4)], [(1, case % 4), (3, 1)]][(case // 3) % 3]
    return n, cols, partition_by, order_by


def test_the_ops_of_rv_window_read_as_frames_equal_window_model_on_60_random_frames():
    rng = np.random.default_rng(12)
    exprs = [("row_number", 0), ("rank", 0), ("dense_rank", 0), ("cum_count", 2), ("cum_sum", 2), ("cum_sum", 4), ("cum_min", 2), ("cum_max", 4), ("cum_min", 4),
             ("lag", 2, 1), ("lead", 4, 2), ("lag", 5, 0), ("lead", 6, 1), ("lag", 6, 50)]
    for case in range(60):
        n, cols, partition_by, order_by = random_frame(rng, case)
        for fast in (False, True):
            got = F.window_frames(cols, partition_by, order_by, exprs, exact_float=True, fast=fast)
            for e, g, w in zip(exprs, got, M.window(cols, partition_by, order_by, exprs)):
                assert same_results(g, w), (case, fast, e, M.cells_of(g), M.cells_of(w))


def test_the_fast_path_equals_the_loop():
    rng = np.random.default_rng(13)
    for case in range(60):
        n, cols, partition_by, order_by = random_frame(rng, case)
        frames = [(int(rng.integers(-6, 7)), int(rng.integers(-6, 7))) for _ in range(4)] + [(None, 0), (0, None), (None, None), (None, -2), (-1, None), (1 << 62, 3), (n, -n)]
        frames = [fr for fr in frames if F.frame_ok(F.edge(fr[0]), F.edge(fr[1]))]
        exprs = [(op, c, p, f) for p, f in frames for op, c in (("count", 5), ("count", 6), ("sum", 2), ("sum", 4), ("min", 4), ("max", 2), ("avg", 2), ("avg", 4),
                                                                ("first_value", 5), ("last_value", 4), ("first_value", 6), ("last_value", 2))]
        exprs += [("ntile", 0, b) for b in (1, 2, 3, 7, n, n + 1)]
        loop = F.window_frames(cols, partition_by, order_by, exprs)
        fast = F.window_frames(cols, partition_by, order_by, exprs, exact_float=True, fast=True)
        for e, a, b in zip(exprs, loop, fast):
            assert same_results(a, b), (case, e, M.cells_of(a), M.cells_of(b))


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------
def test_bindings_agree_and_the_abi_is_still_4():
    header = open(os.path.join(ROOT, "include", "rivulus_gpu.h")).read()
    assert re.search(r"#define RV_ABI_VERSION 4\b", header)
    assert re.search(r"#define RV_FRAME_UNBOUNDED INT64_MAX\b", header) and capi.RV_FRAME_UNBOUNDED == F.UNBOUNDED == (1 << 63) - 1
    assert "rv_window_frames" in capi.PROTOTYPES and getattr(ctypes.CDLL(capi.LIB_PATH), "rv_window_frames") is not None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi
    enums, structs, protos = gen_rust_ffi.parse_header()
    assert dict(enums["rv_window_frame_op"]) == {"RV_WINF_" + k.upper(): v for k, v in capi.WINDOW_FRAME_OPS.items()}
    assert sorted(capi.WINDOW_FRAME_OPS.values()) == list(range(9, 17)) and sorted(capi.WINDOW_OPS.values()) == list(range(9))
    fields = gen_rust_ffi.struct_fields(structs["rv_window_frame_spec"])
    assert [(t, n) for t, n in fields] == [("uint32_t", "op"), ("uint32_t", "col"), ("uint64_t", "offset"), ("int64_t", "preceding"), ("int64_t", "following")]
    assert [(n, getattr(capi.RvWindowFrameSpec, n).offset) for n, _ in capi.RvWindowFrameSpec._fields_] == \
        [("op", 0), ("col", 4), ("offset", 8), ("preceding", 16), ("following", 24)]
    assert ctypes.sizeof(capi.RvWindowFrameSpec) == 32
    args = [a for n, _, a in gen_rust_ffi.prototypes() if n == "rv_window_frames"][0]
    assert len(args) == len(capi.PROTOTYPES["rv_window_frames"][1]) == 11
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "rust_shim", "ffi.rs")).read()
    assert "pub fn rv_window_frames(" in text and "pub struct RvWindowFrameSpec" in text and "pub const RV_WINF_NTILE: c_int = 16;" in text


def test_the_rule_is_one_header_shared_with_the_kernels_and_nothing_is_copied():
    csrc = os.path.join(ROOT, "rivulus_amd", "csrc")
    kernels = open(os.path.join(csrc, "window_frame_kernel.hpp")).read()
    assert '#include "window_frame_rule.hpp"' in kernels and '#include "window_kernel.hpp"' in kernels
    assert "rvframe::frame_pick(" in kernels and "rvframe::ntile_bucket(" in kernels and "rvframe::block_head(" in kernels
    assert "win_block_scan<OP>" in kernels and "win_block_scan(const" not in kernels  # K12's workgroup scan, used and not redefined
    host = open(os.path.join(csrc, "window_frame.hip")).read()
    assert "rvk::window_carry_scan<OP>" in host
    assert "atomicAdd" not in kernels.replace("striped_add", "")  # no floating-point atomic: no atomic add at all next to the scans


def test_window_frame_rule_under_the_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "window_frame_rule_tests.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "window_frame_rule_tests")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, src], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 4000000, r.stdout[-500:]
