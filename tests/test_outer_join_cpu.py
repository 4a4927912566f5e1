"""CPU suite: the model of the outer, semi and anti hash joins (tests/outer_join_model.py) against the hand-written cases of
tests/golden/outer_join_cases.json and against its own invariants, and the join kinds' additions to the C ABI.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from join_model import comparable, inner_join_pairs, materialize
from outer_join_model import (FULL_OUTER, INNER, KIND_NAMES, KINDS, PROBE_ANTI, PROBE_OUTER, PROBE_SEMI, join_pairs, load_golden_cases,
                              materialize_kind, output_names)
from rivulus_amd import capi
from rivulus_amd.capi import RV_BOOLEAN, RV_FLOAT64, RV_INT64, RV_NULL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load_golden_cases()
NAN = float("nan")


def key_of(frame, name):
    return next((d, c) for n, d, c in frame if n == name)


def same_frame(got, want):
    return [(n, d, comparable(d, c)) for n, d, c in got] == [(n, d, comparable(d, c)) for n, d, c in want]


# ---- the golden cases ---------------------------------------------------------------------------------------------------------------
def test_the_golden_file_covers_what_it_must():
    names = {c["name"] for c in CASES}
    assert len(CASES) >= 12 and len(names) == len(CASES)
    for c in CASES:
        assert all(len(col[2]) <= 8 for col in c["build"] + c["probe"]), c["name"]
        assert set(c["pairs"]) == set(KINDS)
    key_cells = lambda c, side: key_of(c[side], c[f"{side}_key"])
    has_null = lambda c, side: any(x is None for x in key_cells(c, side)[1]) and key_cells(c, side)[0] != RV_NULL
    has_nan = lambda c, side: any(isinstance(x, float) and x != x for x in key_cells(c, side)[1])
    assert any(has_null(c, "build") and not has_null(c, "probe") for c in CASES)
    assert any(has_null(c, "probe") and not has_null(c, "build") for c in CASES)
    assert any(has_null(c, "probe") and has_null(c, "build") for c in CASES)
    assert any(not has_null(c, "probe") and not has_null(c, "build") for c in CASES)
    assert any(has_nan(c, "build") for c in CASES) and any(has_nan(c, "probe") for c in CASES)
    assert any(len(key_cells(c, "build")[1]) == 0 for c in CASES) and any(len(key_cells(c, "probe")[1]) == 0 for c in CASES)
    assert any(key_cells(c, "build")[0] == RV_INT64 and key_cells(c, "probe")[0] == RV_FLOAT64 for c in CASES)
    assert any(({n for n, _, _ in c["build"]} - {c["build_key"]}) & {n for n, _, _ in c["probe"]} for c in CASES)  # a name clash
    zeros = [c for c in CASES if key_cells(c, "build")[0] == RV_FLOAT64 and 0.0 in key_cells(c, "build")[1]]
    assert any({str(x) for x in key_cells(c, "build")[1] + key_cells(c, "probe")[1]} >= {"0.0", "-0.0"} for c in zeros)
    assert any(len(set(x for x in key_cells(c, "build")[1] if x is not None)) < len([x for x in key_cells(c, "build")[1] if x is not None])
               for c in CASES if key_cells(c, "build")[0] == RV_INT64)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_the_golden_cases(case):
    bd, bk = key_of(case["build"], case["build_key"])
    pd, pk = key_of(case["probe"], case["probe_key"])
    for kind in KINDS:
        pairs = join_pairs(kind, bd, bk, pd, pk)
        assert pairs == case["pairs"][kind], KIND_NAMES[kind]
        if kind in case["frames"]:
            got = materialize_kind(kind, case["probe"], case["build"], case["build_key"], pairs)
            assert same_frame(got, case["frames"][kind]), KIND_NAMES[kind]


def test_golden_inner_frames_are_the_inner_model_s():
    """The literal INNER frames of the golden file against join_model.materialize: the two models agree on today's join."""
    for case in CASES:
        if INNER in case["frames"]:
            got = materialize(case["probe"], case["build"], case["build_key"], case["pairs"][INNER])
            assert same_frame(got, case["frames"][INNER]), case["name"]


# ---- invariants on random inputs ----------------------------------------------------------------------------------------------------
def random_keys(rng, dtype, n):
    if dtype == RV_NULL:
        return [None] * n
    if dtype == RV_INT64:
        base = rng.integers(-6, 6, n).tolist()
    elif dtype == RV_FLOAT64:
        pool = [0.0, -0.0, NAN, 1.5, -2.0, float("inf")]
        base = [pool[i] for i in rng.integers(0, len(pool), n)]
    else:
        base = (rng.integers(0, 2, n) == 1).tolist()
    return [None if rng.random() < 0.15 else v for v in base]


def random_sides():
    rng = np.random.default_rng(99)
    dtypes = [RV_INT64, RV_FLOAT64, RV_BOOLEAN, RV_NULL]
    for trial in range(200):
        bd, pd = dtypes[int(rng.integers(0, 4))], dtypes[int(rng.integers(0, 4))]
        if trial % 3:
            pd = bd
        yield bd, random_keys(rng, bd, int(rng.integers(0, 40))), pd, random_keys(rng, pd, int(rng.integers(0, 40)))


def test_inner_kind_is_the_inner_join_model():
    for bd, bk, pd, pk in random_sides():
        assert join_pairs(INNER, bd, bk, pd, pk) == inner_join_pairs(bd, bk, pd, pk)


def test_semi_and_anti_partition_the_probe_rows():
    for bd, bk, pd, pk in random_sides():
        semi = [p for p, _ in join_pairs(PROBE_SEMI, bd, bk, pd, pk)]
        anti = [p for p, _ in join_pairs(PROBE_ANTI, bd, bk, pd, pk)]
        assert semi == sorted(semi) and anti == sorted(anti)
        assert sorted(semi + anti) == list(range(len(pk)))
        assert set(semi) == {p for p, _ in inner_join_pairs(bd, bk, pd, pk)}


def test_outer_row_count_is_inner_plus_anti():
    for bd, bk, pd, pk in random_sides():
        outer = join_pairs(PROBE_OUTER, bd, bk, pd, pk)
        inner = inner_join_pairs(bd, bk, pd, pk)
        anti = join_pairs(PROBE_ANTI, bd, bk, pd, pk)
        assert len(outer) == len(inner) + len(anti)
        assert [x for x in outer if x[1] is not None] == inner
        assert [p for p, b in outer if b is None] == [p for p, _ in anti]
        assert [p for p, _ in outer] == sorted(p for p, _ in outer)


def test_full_outer_tail_is_ascending_and_disjoint_from_the_inner_build_rows():
    for bd, bk, pd, pk in random_sides():
        full = join_pairs(FULL_OUTER, bd, bk, pd, pk)
        outer = join_pairs(PROBE_OUTER, bd, bk, pd, pk)
        assert full[:len(outer)] == outer
        tail = full[len(outer):]
        assert all(p is None for p, _ in tail)
        rows = [b for _, b in tail]
        assert rows == sorted(set(rows))
        met = {b for _, b in inner_join_pairs(bd, bk, pd, pk)}
        assert not met & set(rows) and met | set(rows) == set(range(len(bk)))


def test_output_names():
    probe = [("a", RV_INT64, []), ("k", RV_INT64, [])]
    build = [("k", RV_INT64, []), ("a", RV_INT64, []), ("b", RV_INT64, [])]
    assert output_names(INNER, probe, build, "k") == ["a", "k", "a_right", "b"]
    assert output_names(PROBE_OUTER, probe, build, "k") == ["a", "k", "a_right", "b"]
    assert output_names(FULL_OUTER, probe, build, "k") == ["a", "k", "k_right", "a_right", "b"]
    assert output_names(PROBE_SEMI, probe, build, "k") == output_names(PROBE_ANTI, probe, build, "k") == ["a", "k"]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_join_kinds_within_abi_4():
    text = open(os.path.join(ROOT, "include", "rivulus_gpu.h")).read()
    assert "#define RV_ABI_VERSION 4" in text
    for name in ("rv_join_probe_kind", "rv_take_device_nullable", "rv_hash_join_kind", "rv_hash_join_chunked_kind"):
        assert re.search(r"rv_status %s\(" % name, text), name
        assert name in capi.PROTOTYPES, name
    m = re.search(r"typedef enum rv_join_kind \{(.*?)\} rv_join_kind;", text, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    items = dict((k.strip(), int(v)) for k, v in (it.split("=") for it in body.split(",") if it.strip()))
    assert items == {"RV_JOIN_INNER": 0, "RV_JOIN_PROBE_OUTER": 1, "RV_JOIN_FULL_OUTER": 2, "RV_JOIN_PROBE_SEMI": 3, "RV_JOIN_PROBE_ANTI": 4}
    assert (capi.RV_JOIN_INNER, capi.RV_JOIN_PROBE_OUTER, capi.RV_JOIN_FULL_OUTER, capi.RV_JOIN_PROBE_SEMI, capi.RV_JOIN_PROBE_ANTI) == KINDS
    # the inner entry points are still there, unchanged in shape
    for name in ("rv_join_probe", "rv_hash_join", "rv_hash_join_chunked", "rv_take_device"):
        assert re.search(r"rv_status %s\(" % name, text), name
    # the kernel names the tests check are the documented ones
    for s in ("join_probe_emit<0,outer>", "join_probe_emit<1,outer>", "join_probe_emit<2,outer>", "join_probe_emit<0,full>",
              "join_probe_emit<1,full>", "join_probe_emit<2,full>", "join_probe_emit<0,semi>", "join_probe_emit<0,anti>"):
        assert s in text, s


def test_join_output_columns():
    assert [capi.join_output_columns(k, 3, 4) for k in KINDS] == [6, 6, 7, 3, 3]


def test_rust_ffi_is_in_step_with_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ffi = open(os.path.join(ROOT, "rust_shim", "ffi.rs")).read()
    assert "pub fn rv_hash_join_kind(" in ffi and "pub const RV_JOIN_PROBE_ANTI: c_int = 4;" in ffi
