"""CPU suite of the window operator (K12): tests/window_model.py against the hand-written tables of tests/golden/window_cases.json, the
three bindings of rv_window against each other, and csrc/window_combine.hpp under the sanitizers as a stand-alone program."""
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import sort_model as S
import window_model as M
from rivulus_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "window_cases.json")) as f:
    CASES = json.load(f)["cases"]


def test_there_are_sixteen_hand_written_cases_and_they_cover_the_ground():
    names = [c["name"] for c in CASES]
    assert len(CASES) >= 16 and len(set(names)) == len(names)
    ops = {e["op"] for c in CASES for e in c["exprs"]}
    assert ops == set(capi.WINDOW_OPS)
    assert any(not c["partition_by"] and c["order_by"] for c in CASES) and any(c["partition_by"] and not c["order_by"] for c in CASES)
    assert any(not c["partition_by"] and not c["order_by"] for c in CASES)
    assert {f for c in CASES for _, f in c["order_by"]} >= {0, 1, 3}
    assert any(None in e["expected"] for c in CASES for e in c["exprs"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_against_hand_written_tables(case):
    cols = [M.column_of(c["dtype"], c["cells"]) for c in case["columns"]]
    exprs = [(e["op"], e["col"], e.get("offset", 0)) for e in case["exprs"]]
    got = M.window(cols, case["partition_by"], [tuple(k) for k in case["order_by"]], exprs)
    for e, g in zip(case["exprs"], got):
        assert g[0] == e["dtype"], (e, g[0])
        assert M.same_cells(M.cells_of(g), M.expected_cells(e["dtype"], e["expected"])), f"{e['op']}: model {M.cells_of(g)}, table {e['expected']}"


def brute_force(cols, partition_by, order_by, op, ci, k=0):
    """the header's sentences read row by row, quadratic: a second statement next to the model's cumulative sums (Int64 columns only)"""
    n = M.rows_of(cols)
    codes = M.partition_codes(cols, partition_by)
    perm = list(S.sort_frame(M.cols_for_sort(cols), order_by)) if order_by else list(range(n))
    keys = [S.working_keys(M.cols_for_sort(cols)[c], f) for c, f in order_by]
    values, valid = cols[ci][1], M.valid_of(cols[ci])
    out = []
    for r in range(n):
        mine = [q for q in perm if codes[q] == codes[r]]
        pos = mine.index(r)
        peers = lambda a, b: all(cls[a] == cls[b] and key[a] == key[b] for cls, key in keys)
        frame = [q for q in mine[:pos + 1] if valid[q]]
        if op == "row_number":
            out.append(pos + 1)
        elif op == "rank":
            out.append(1 + min(i for i, q in enumerate(mine) if peers(q, r)))
        elif op == "dense_rank":
            out.append(1 + sum(1 for i in range(1, pos + 1) if not peers(mine[i], mine[i - 1])))
        elif op == "cum_count":
            out.append(len(frame))
        elif op == "cum_sum":
            s = sum(int(values[q]) for q in frame) % (1 << 64)
            out.append(s - (1 << 64) if s >> 63 else s)
        elif op in ("cum_min", "cum_max"):
            out.append((min if op == "cum_min" else max)(int(values[q]) for q in frame) if frame else None)
        else:
            s = pos - k if op == "lag" else pos + k
            out.append(int(values[mine[s]]) if 0 <= s < len(mine) and valid[mine[s]] else None)
    return out


def test_model_against_the_sentences_read_row_by_row():
    rng = np.random.default_rng(12)
    for case in range(60):
        n = int(rng.integers(1, 40))
        mask = lambda: (rng.random(n) >= 0.3) if rng.random() < 0.7 else None
        cols = [("i64", rng.integers(0, 3, n), mask()), ("i64", rng.integers(-2, 3, n), mask()), ("i64", rng.integers(-9, 9, n), mask()),
                ("i64", rng.integers(0, 2, n), None)]
        partition_by = [[], [0], [0, 3]][case % 3]
        order_by = [[], [(1, case % 4)], [(1, case % 4), (3, 1)]][(case // 3) % 3]
        exprs = [("row_number", 0), ("rank", 0), ("dense_rank", 0), ("cum_count", 2), ("cum_sum", 2), ("cum_min", 2), ("cum_max", 2), ("lag", 2, 1),
                 ("lead", 2, 2), ("lag", 2, 0)]
        got = M.window(cols, partition_by, order_by, exprs)
        for e, g in zip(exprs, got):
            assert M.cells_of(g) == brute_force(cols, partition_by, order_by, *e), (case, e)


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------
def test_bindings_agree_and_the_abi_is_still_4():
    header = open(os.path.join(ROOT, "include", "rivulus_gpu.h")).read()
    assert re.search(r"#define RV_ABI_VERSION 4\b", header)
    assert "rv_window" in capi.PROTOTYPES and getattr(ctypes.CDLL(capi.LIB_PATH), "rv_window") is not None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi
    enums, structs, protos = gen_rust_ffi.parse_header()
    assert dict(enums["rv_window_op"]) == {"RV_WIN_" + k.upper(): v for k, v in capi.WINDOW_OPS.items()}
    fields = gen_rust_ffi.struct_fields(structs["rv_window_spec"])
    assert [(t, n) for t, n in fields] == [("uint32_t", "op"), ("uint32_t", "col"), ("uint64_t", "offset")]
    assert [(n, getattr(capi.RvWindowSpec, n).offset) for n, _ in capi.RvWindowSpec._fields_] == [("op", 0), ("col", 4), ("offset", 8)]
    assert ctypes.sizeof(capi.RvWindowSpec) == 16
    args = [a for n, _, a in gen_rust_ffi.prototypes() if n == "rv_window"][0]
    assert len(args) == len(capi.PROTOTYPES["rv_window"][1]) == 11
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "rust_shim", "ffi.rs")).read()
    assert "pub fn rv_window(" in text and "pub struct RvWindowSpec" in text and "pub const RV_WIN_LEAD: c_int = 8;" in text


def test_the_combine_is_one_header_shared_with_the_kernels():
    csrc = os.path.join(ROOT, "rivulus_amd", "csrc")
    kernels = open(os.path.join(csrc, "window_kernel.hpp")).read()
    assert '#include "window_combine.hpp"' in kernels and '#include "order_key.hpp"' in kernels
    assert "atomicAdd" not in kernels.replace("striped_add", "")  # no floating-point atomic: no atomic add at all next to the scan


def test_window_combine_under_the_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "window_combine_tests.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "window_combine_tests")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, src], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 10000, r.stdout[-500:]
