"""GPU suite: rv_window against tests/window_model.py.  Every comparison is exact (Float64 by bit pattern, every NaN one NaN) except the one
Float64 CUM_SUM test over data whose partial sums round, which holds the device to the bound the header states.  Row counts sit round one
lane, one wave and one tile of the scan (kWinTileRows sorted positions), one past the kWinTileRows tile aggregates a round of the carry scan
takes, and 2^24 rows."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import group_agg_model as A
import window_model as M
from rivulus_amd import capi
from rivulus_amd.capi import RV_BOOLEAN, RV_FLOAT64, RV_INT64, RV_NULL, RV_STRING, Column, RvError

pytestmark = pytest.mark.gpu

RV_ERR_INVALID_ARG, RV_ERR_LENGTH_MISMATCH, RV_ERR_TYPE_MISMATCH, RV_ERR_OUT_OF_BOUNDS, RV_ERR_UNSUPPORTED = 1, 2, 3, 4, 5
with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rivulus_amd", "csrc", "window_kernel.hpp")) as _f:
    _src = _f.read()
THREADS = int(re.search(r"kWinThreads = (\d+)", _src).group(1))
ITEMS = int(re.search(r"kWinItems = (\d+)", _src).group(1))
TILE = THREADS * ITEMS
WAVE = 64 * ITEMS  # sorted positions one wave of the scan holds
ROW_COUNTS = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
I64_MIN = -(1 << 63)
ALL_FLAGS = [0, 1, 2, 3]
DTYPES = {"i64": RV_INT64, "f64": RV_FLOAT64, "bool": RV_BOOLEAN, "str": RV_STRING, "null": RV_NULL}
NUMBERING = [("row_number", 0), ("rank", 0), ("dense_rank", 0)]
EVERY_OP = NUMBERING + [("cum_count", 0), ("cum_sum", 0), ("cum_min", 0), ("cum_max", 0), ("lag", 0, 1), ("lead", 0, 2)]


@pytest.fixture(scope="module")
def ctx():
    with capi.Context(0) as c:
        yield c


# ---- building inputs ----------------------------------------------------------------------------------------------------------------
def upload(ctx, col, offset=0):
    """The device column of a model column; offset > 0: a slice at that element (and validity bit) offset of a longer upload."""
    dtype, values, valid = col
    n = len(values)
    if dtype == "null":
        return ctx.upload(Column.nulls(n))
    ok = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    if dtype == "str":
        cells = ["pad"] * offset + [v if o else None for v, o in zip(values, ok)] + ["pad"] * min(3, offset)
        host = Column.from_strings(cells)
    else:
        fill = np.full(offset, 1 if dtype == "bool" else 77, np.asarray(values).dtype)
        full = np.concatenate([fill, np.asarray(values), fill[:3]])
        mask = np.concatenate([np.ones(offset, bool), ok, np.ones(min(3, offset), bool)])
        host = Column.from_numpy(full, None if valid is None and not offset else mask)
    dev = ctx.upload(host)
    return dev.slice(offset, n) if offset else dev


def compare(dev, want, what):
    """one output column against the model's (dtype, values, valid): dtype, length, bitmap iff a null, null count, cells, 0 under nulls"""
    dtype, values, valid = want
    n = len(valid)
    info = dev.info()
    assert info.dtype == DTYPES[dtype] and info.length == n, f"{what}: dtype {info.dtype} length {info.length}"
    if dtype == "null":
        return
    nulls = int((~valid).sum())
    assert info.null_count == nulls and bool(info.has_validity) == (nulls > 0), f"{what}: null_count {info.null_count} (model {nulls}), bitmap {info.has_validity}"
    host = dev.download()
    if nulls:
        assert np.array_equal(host.logical_valid(), valid), f"{what}: validity differs first at {np.flatnonzero(host.logical_valid() != valid)[:5]}"
    if dtype == "str":
        got = host.to_strings()
        assert got == [v if o else None for v, o in zip(values, valid)], f"{what}: strings differ"
        return
    got = host.logical_values()
    if dtype == "f64":
        got = M.canonical_bits(got)
    bad = np.flatnonzero(got != np.asarray(values))
    assert len(bad) == 0, f"{what}: cells differ first at rows {bad[:5]}: got {got[bad[:5]]}, model {np.asarray(values)[bad[:5]]}"


def check(ctx, cols, partition_by, order_by, exprs, offsets=None, exact_float=False, what=""):
    want = M.window(cols, partition_by, order_by, exprs, exact_float=exact_float)
    devs = [upload(ctx, c, offsets[i] if offsets else 0) for i, c in enumerate(cols)]
    got = ctx.window(devs, partition_by, order_by, exprs)
    for e, g, w in zip(exprs, got, want):
        compare(g, w, f"{what} {e} partition {partition_by} order {order_by}")
    return got


def i64(values, valid=None):
    return "i64", np.asarray(values, np.int64), valid


def f64(values, valid=None):
    return "f64", np.asarray(values, np.float64), valid


def garbage_under_nulls(col):
    """the same column with NaN / INT64_MIN under its null cells"""
    dtype, values, valid = col
    if valid is None:
        return col
    values = values.copy()
    values[~valid] = np.nan if dtype == "f64" else I64_MIN
    return dtype, values, valid


def frame(rng, n, parts, nulls=0.2):
    """partition key, order key with ties, an Int64 and an integer-valued Float64 value column, all but the partition key nullable"""
    mask = lambda: (rng.random(n) >= nulls) if n and nulls else None
    return [i64(rng.integers(0, max(1, parts), n)), i64(rng.integers(-5, 5, n), mask()),
            garbage_under_nulls(i64(rng.integers(-1000, 1000, n), mask())),
            garbage_under_nulls(f64(rng.integers(-(1 << 19), 1 << 19, n).astype(np.float64), mask()))]


# ---- row counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts(ctx, n):
    rng = np.random.default_rng(n)
    cols = frame(rng, n, 5)
    exprs = NUMBERING + [("cum_count", 2), ("cum_sum", 2), ("cum_sum", 3), ("cum_min", 3), ("cum_max", 2), ("lag", 2, 1), ("lead", 3, 1)]
    check(ctx, cols, [0], [(1, 0)], exprs, exact_float=True)
    check(ctx, cols, [], [], exprs, exact_float=True, what="in place")
    if n:
        assert ctx.last_kernel() == "window_scan"


def test_zero_rows_have_the_right_dtypes(ctx):
    cols = [i64([]), f64([]), ("bool", np.zeros(0, bool), None), ("str", [], None)]
    got = check(ctx, cols, [0], [(1, 0)], [("row_number", 0), ("cum_sum", 1), ("cum_min", 0), ("lag", 2, 1), ("lead", 3, 1), ("cum_count", 3)])
    assert [g.info().dtype for g in got] == [RV_INT64, RV_FLOAT64, RV_INT64, RV_BOOLEAN, RV_STRING, RV_INT64]


def test_one_past_a_round_of_the_carry_scan(ctx):
    n = TILE * TILE + 1  # kWinTileRows tile aggregates and one more: the carry scan's second round
    rng = np.random.default_rng(7)
    part = np.sort(rng.integers(0, 40, n))
    cols = [i64(part), i64(rng.integers(-1000, 1000, n))]
    check(ctx, cols, [0], [], [("row_number", 0), ("cum_sum", 1)])
    check(ctx, cols, [], [], [("row_number", 0), ("cum_sum", 1)], what="in place")


def test_2_24_rows(ctx):
    """The model's sorts over 2^24 rows would take many seconds, so this one frame is built for its answer to have a closed form: partition
    p = row % 1000, ordered by a key that falls with the row index, value = the row index.  A partition's rows are p, p + 1000, ..., in window
    order from the largest down; with t = row // 1000 and T the partition's largest t, row_number = T - t + 1, the running sum is the sum of
    p + 1000 s for s = t .. T, and LAG(1) is the row 1000 further on, null for the partition's largest row."""
    n, parts = 1 << 24, 1000
    row = np.arange(n, dtype=np.int64)
    p, t = row % parts, row // parts
    top = (n - 1 - p) // parts
    devs = [ctx.upload(Column.from_numpy(c)) for c in (p, n - row, row)]
    got = ctx.window(devs, [0], [(1, 0)], [("row_number", 0), ("cum_sum", 2), ("lag", 2, 1)])
    none = np.ones(n, bool)
    compare(got[0], ("i64", top - t + 1, none), "row_number")
    compare(got[1], ("i64", (top - t + 1) * p + parts * (top * (top + 1) // 2 - (t - 1) * t // 2), none), "cum_sum")
    compare(got[2], ("i64", np.where(row + parts < n, row + parts, 0), row + parts < n), "lag")
    assert ctx.last_kernel() == "window_scan"


# ---- shapes where a segmented scan goes wrong -------------------------------------------------------------------------------------------
def value_columns(rng, n):
    return [garbage_under_nulls(i64(rng.integers(-1000, 1000, n), rng.random(n) >= 0.3)),
            garbage_under_nulls(f64(rng.integers(-1000, 1000, n).astype(np.float64), rng.random(n) >= 0.3))]


SCAN_EXPRS = NUMBERING + [("cum_count", 1), ("cum_sum", 1), ("cum_sum", 2), ("cum_min", 1), ("cum_max", 2), ("cum_min", 2), ("cum_max", 1)]


def test_one_partition_over_many_tiles_passes_the_carry_on(ctx):
    n = 4 * TILE + 13  # heads at 0 and at 3 * TILE + 500: tiles 1 and 2 hold no head
    rng = np.random.default_rng(1)
    part = (np.arange(n) >= 3 * TILE + 500).astype(np.int64)
    check(ctx, [i64(part)] + value_columns(rng, n), [0], [], SCAN_EXPRS, exact_float=True)


def test_every_row_its_own_partition(ctx):
    n = 2 * TILE + 3
    rng = np.random.default_rng(2)
    check(ctx, [i64(rng.permutation(n))] + value_columns(rng, n), [0], [], SCAN_EXPRS + [("lag", 1, 1), ("lead", 1, 1)], exact_float=True)


@pytest.mark.parametrize("head", [TILE - 1, TILE, TILE + 1, WAVE - 1, WAVE, WAVE + ITEMS - 1, WAVE + ITEMS, 2 * TILE - 1, 2 * TILE + 1])
def test_heads_at_the_edges_of_tiles_waves_and_threads(ctx, head):
    n = 2 * TILE + 2  # two partitions: [0, head) and [head, n); the second ends at the last row
    rng = np.random.default_rng(head)
    part = (np.arange(n) >= head).astype(np.int64)
    check(ctx, [i64(part)] + value_columns(rng, n), [0], [], SCAN_EXPRS + [("lag", 1, 2), ("lead", 2, 2)], exact_float=True)


def test_all_null_value_columns(ctx):
    n = TILE + 70
    rng = np.random.default_rng(3)
    none = np.zeros(n, bool)
    cols = [i64(rng.integers(0, 9, n)), ("i64", np.full(n, I64_MIN), none), ("f64", np.full(n, np.nan), none), ("null", np.zeros(n, np.int64), None)]
    exprs = [("cum_count", 1), ("cum_sum", 1), ("cum_sum", 2), ("cum_min", 1), ("cum_max", 2), ("lag", 1, 1), ("lead", 2, 1), ("cum_count", 3), ("lag", 3, 1)]
    got = check(ctx, cols, [0], [], exprs)
    assert got[1].info().has_validity == 0 and got[3].info().null_count == n


@pytest.mark.parametrize("offset", [1, 63, 65])
def test_slices(ctx, offset):
    n = TILE + 9
    rng = np.random.default_rng(offset)
    cols = frame(rng, n, 7) + [("bool", rng.random(n) < 0.5, rng.random(n) >= 0.2), ("str", [f"s{i % 11}" for i in range(n)], rng.random(n) >= 0.2)]
    exprs = EVERY_OP + [("cum_sum", 3), ("cum_min", 3), ("cum_max", 2), ("cum_count", 5), ("lag", 4, 1), ("lead", 5, 1), ("cum_count", 4)]
    check(ctx, cols, [0], [(1, 0)], exprs, offsets=[offset, offset + 1, offset, 0, offset, offset], exact_float=True)


# ---- every op x dtype x flags x nulls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("nulls", [0.0, 0.3, 1.0])
def test_every_op_over_both_dtypes(ctx, flags, nulls):
    n = TILE + 300
    rng = np.random.default_rng(flags * 10 + int(nulls * 10))
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -2.5, 1e300, 5e-324])
    cols = frame(rng, n, 6, nulls=0.0)
    cols[1] = i64(rng.integers(-3, 3, n), rng.random(n) >= nulls if nulls else None)            # Int64 order key
    cols.append(garbage_under_nulls(f64(rng.choice(specials, n), rng.random(n) >= nulls if nulls else None)))  # Float64 order key / MIN / MAX value
    for v in (2, 3):
        cols[v] = garbage_under_nulls((cols[v][0], cols[v][1], rng.random(n) >= nulls if nulls else None))
    exprs = NUMBERING + [(op, c) for op in ("cum_count", "cum_sum", "cum_min", "cum_max") for c in (2, 3)] + \
        [("cum_min", 4), ("cum_max", 4), ("cum_count", 4), ("lag", 2, 1), ("lead", 3, 1), ("lag", 4, 2)]
    check(ctx, cols, [0], [(1, flags)], exprs, exact_float=True, what="Int64 order key")
    check(ctx, cols, [0], [(4, flags), (1, flags ^ 1)], exprs, exact_float=True, what="Float64 + Int64 order keys")


def test_two_partition_keys_boolean_and_float_specials(ctx):
    n = TILE + 131
    rng = np.random.default_rng(5)
    nan2 = np.array([0x7FF8000000000001], np.uint64).view(np.float64)[0]
    fkey = rng.choice(np.array([0.0, -0.0, np.nan, -np.nan, nan2, 1.0, np.inf]), n)
    cols = [("bool", rng.random(n) < 0.5, rng.random(n) >= 0.2), garbage_under_nulls(f64(fkey, rng.random(n) >= 0.2)), i64(rng.integers(-9, 9, n), rng.random(n) >= 0.2),
            i64(rng.integers(-1000, 1000, n))]
    check(ctx, cols, [0, 1], [(2, 2)], NUMBERING + [("cum_sum", 3), ("cum_max", 3), ("lag", 3, 1), ("lead", 0, 1), ("cum_count", 0)])
    assert ctx.last_kernel() == "window_scan"


# ---- LAG / LEAD -------------------------------------------------------------------------------------------------------------------------
def test_lag_lead_offsets_and_dtypes(ctx):
    n, plen = 6 * 97, 97
    rng = np.random.default_rng(6)
    cols = [i64(np.arange(n) // plen), i64(rng.integers(-50, 50, n)), garbage_under_nulls(i64(rng.integers(-9, 9, n), rng.random(n) >= 0.2)),
            garbage_under_nulls(f64(rng.standard_normal(n), rng.random(n) >= 0.2)), ("bool", rng.random(n) < 0.5, rng.random(n) >= 0.2),
            ("str", [f"v{i * 7 % 23}" * (i % 3) for i in range(n)], rng.random(n) >= 0.2), ("bool", rng.random(n) < 0.5, None), ("str", [f"w{i}" for i in range(n)], None)]
    exprs = [(op, c, k) for op in ("lag", "lead") for c in (2, 3, 4, 5, 6, 7) for k in (0, 1, 2, plen, n + 1)]
    check(ctx, cols, [0], [(1, 0)], exprs)
    assert ctx.last_kernel() == "window_shift"
    check(ctx, cols, [], [], exprs[::3], what="in place")
    assert ctx.last_kernel() == "window_shift"
    got = check(ctx, cols, [0], [(1, 1)], [("lag", 7, 0), ("lead", 6, 0), ("lag", 2, 1 << 62), ("lead", 2, 1 << 62)])
    assert got[0].info().has_validity == 0 and got[1].info().has_validity == 0  # k == 0 copies the column


def test_in_place_path(ctx):
    n = 3 * TILE + 5
    rng = np.random.default_rng(8)
    cols = [i64(np.zeros(n))] + value_columns(rng, n)
    check(ctx, cols, [], [], SCAN_EXPRS + [("lag", 1, 3), ("lead", 2, TILE)], exact_float=True)
    assert ctx.last_kernel() == "window_scan"


# ---- Float64 CUM_SUM --------------------------------------------------------------------------------------------------------------------
def test_float_sum_of_integer_valued_cells_is_bit_exact(ctx):
    n = 5 * TILE + 77  # |x| < 2^20: every partial sum of any bracketing is an integer below 2^44
    rng = np.random.default_rng(9)
    x = rng.integers(-(1 << 20) + 1, 1 << 20, n).astype(np.float64)
    x[rng.random(n) < 0.05] = -0.0
    cols = [i64(rng.integers(0, 3, n)), i64(rng.integers(0, 1 << 30, n)), garbage_under_nulls(f64(x, rng.random(n) >= 0.1))]
    check(ctx, cols, [0], [(1, 0)], [("cum_sum", 2)], exact_float=True)
    check(ctx, cols, [], [], [("cum_sum", 2)], exact_float=True, what="in place")


def test_float_sum_within_the_stated_bound_and_the_same_bits_twice(ctx):
    """mixed-sign uniform data: |got - fsum(frame)| <= gamma_{m-1} x sum|x| over the frame, m its non-null cells (the header's bound: that
    of any summation order, tests/group_agg_model.gamma_bound), against math.fsum over the frame.  A frame of one or two cells has one
    correctly rounded sum and the bound leaves no room for another."""
    n = 3 * TILE + 11
    rng = np.random.default_rng(10)
    x = rng.uniform(-1.0, 1.0, n)
    valid = rng.random(n) >= 0.1
    cols = [i64((np.arange(n) >= TILE + 5).astype(np.int64)), garbage_under_nulls(f64(x, valid))]
    devs = [upload(ctx, c) for c in cols]
    a = ctx.window(devs, [0], [], [("cum_sum", 1)])[0].download().logical_values()
    b = ctx.window(devs, [0], [], [("cum_sum", 1)])[0].download().logical_values()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "two calls over the same buffers differ"
    seq, part_head, _ = M.sequence(cols, [0], [])
    worst = Fraction(0)
    cells = []
    for j, row in enumerate(seq):
        if part_head[j]:
            cells = []
        if valid[row]:
            cells.append(float(x[row]))
        last = j + 1 == n or part_head[j + 1]
        if j % 97 and not part_head[j] and not last:
            continue  # every 97th position, every partition's first and last
        exact = math.fsum(cells)
        bound = A.gamma_bound(cells)
        err = abs(Fraction(float(a[row])) - Fraction(exact))
        assert err <= bound, f"row {row} (position {j}, {len(cells)} cells): |{a[row]!r} - {exact!r}| = {float(err):.3e} > {float(bound):.3e}"
        worst = max(worst, err / bound if bound else Fraction(0))
    print(f"worst error / bound: {float(worst):.3e}")


# ---- random cases -------------------------------------------------------------------------------------------------------------------------
def test_100_random_cases(ctx):
    rng = np.random.default_rng(100)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0, -7.0, 0.5])
    for case in range(100):
        n = int(rng.choice([1, 2, 5, 64, 65, 200, 700, TILE + 3]))
        mask = lambda p=0.25: (rng.random(n) >= p) if rng.random() < 0.7 else None
        cols = [i64(rng.integers(0, int(rng.choice([1, 2, 5, 50])), n), mask()), ("bool", rng.random(n) < 0.5, mask()),
                f64(rng.choice(specials, n), mask()), i64(rng.integers(-4, 4, n), mask()),
                garbage_under_nulls(i64(rng.integers(I64_MIN, (1 << 63) - 1, n, endpoint=True), mask())),
                garbage_under_nulls(f64(rng.integers(-99, 99, n).astype(np.float64), mask())), ("str", [f"x{i % 5}" for i in range(n)], mask()),
                ("null", np.zeros(n, np.int64), None)]
        partition_by = [int(c) for c in rng.choice([0, 1, 2, 7], int(rng.integers(0, 3)), replace=False)]
        order_by = [(int(c), int(rng.integers(0, 4))) for c in rng.choice([2, 3, 5, 7], int(rng.integers(0, 3)), replace=False)]
        ops = [("row_number", 0), ("rank", 1), ("dense_rank", 6), ("cum_count", int(rng.integers(0, 8))), ("cum_sum", 4), ("cum_sum", 5), ("cum_min", 2),
               ("cum_max", 2), ("cum_min", 4), ("cum_max", 5), ("lag", int(rng.integers(0, 8)), int(rng.integers(0, 4))),
               ("lead", int(rng.integers(0, 8)), int(rng.integers(0, 4)))]
        exprs = [ops[i] for i in rng.choice(len(ops), int(rng.integers(1, 6)), replace=False)]
        check(ctx, cols, partition_by, order_by, exprs, exact_float=True, what=f"case {case}")


# ---- errors: each leaves the context usable and creates nothing ---------------------------------------------------------------------------
def test_errors_are_followed_by_a_good_call(ctx):
    n = 100
    rng = np.random.default_rng(11)
    model = frame(rng, n, 4) + [("bool", rng.random(n) < 0.5, None), ("str", [f"s{i % 3}" for i in range(n)], None)]
    cols = [upload(ctx, c) for c in model]
    short = upload(ctx, i64(np.arange(n - 1)))

    def good():
        got = ctx.window(cols, [0], [(1, 0)], [("row_number", 0), ("cum_sum", 2)])
        for g, w in zip(got, M.window(model, [0], [(1, 0)], [("row_number", 0), ("cum_sum", 2)])):
            compare(g, w, "the call after an error")

    def refused(status, text, *args):
        with pytest.raises(RvError) as e:
            ctx.window(*args)
        assert e.value.status == status and text in e.value.message, e.value
        good()

    refused(RV_ERR_INVALID_ARG, "no window expressions", cols, [0], [], [])
    refused(RV_ERR_INVALID_ARG, "unknown op", cols, [0], [], [(9, 0)])
    refused(RV_ERR_INVALID_ARG, "reads column 6 of 6", cols, [0], [], [("cum_sum", 6)])
    refused(RV_ERR_INVALID_ARG, "partition key 0 is column 7", cols, [7], [], [("row_number", 0)])
    refused(RV_ERR_INVALID_ARG, "order key 0 is column 6", cols, [], [(6, 0)], [("row_number", 0)])
    refused(RV_ERR_INVALID_ARG, "unknown flag bits", cols, [], [(1, 4)], [("row_number", 0)])
    refused(RV_ERR_INVALID_ARG, "key columns", cols, [0] * 9, [], [("row_number", 0)])
    refused(RV_ERR_INVALID_ARG, "order keys", cols, [], [(1, 0)] * 9, [("row_number", 0)])
    refused(RV_ERR_LENGTH_MISMATCH, "length", cols + [short], [0], [], [("row_number", 0)])
    refused(RV_ERR_UNSUPPORTED, "String keys go through rv_string_dict_build", cols, [5], [], [("row_number", 0)])
    refused(RV_ERR_UNSUPPORTED, "Boolean and String sort keys are not built", cols, [], [(4, 0)], [("row_number", 0)])
    refused(RV_ERR_UNSUPPORTED, "Boolean and String sort keys are not built", cols, [], [(5, 0)], [("row_number", 0)])
    for op in ("cum_sum", "cum_min", "cum_max"):
        refused(RV_ERR_TYPE_MISMATCH, "take an Int64 or Float64 column", cols, [0], [], [(op, 4)])
        refused(RV_ERR_TYPE_MISMATCH, "take an Int64 or Float64 column", cols, [0], [], [(op, 5)])
    ctx.set_option("agg_max_groups", 3)
    try:  # four partitions
        with pytest.raises(RvError) as e:
            ctx.window(cols, [0], [], [("row_number", 0)])
        assert e.value.status == RV_ERR_UNSUPPORTED and "agg_max_groups" in e.value.message, e.value
    finally:
        ctx.set_option("agg_max_groups", 0)
    good()
    lib = capi.load()
    out = (capi.C.c_void_p * 1)()
    spec = (capi.RvWindowSpec * 1)()
    assert lib.rv_window(ctx.handle, None, 1, None, 0, None, None, 0, spec, 1, out) == RV_ERR_INVALID_ARG
    assert lib.rv_window(ctx.handle, capi._handles(cols), len(cols), None, 1, None, None, 0, spec, 1, out) == RV_ERR_INVALID_ARG
    assert lib.rv_window(ctx.handle, capi._handles(cols), len(cols), None, 0, None, None, 0, None, 1, out) == RV_ERR_INVALID_ARG
    assert lib.rv_window(ctx.handle, capi._handles(cols), len(cols), None, 0, None, None, 0, spec, 1, None) == RV_ERR_INVALID_ARG
    good()
