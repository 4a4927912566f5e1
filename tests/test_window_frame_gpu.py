"""GPU suite: rv_window_frames against tests/window_frame_model.py.  Every comparison is exact (Float64 by bit pattern, every NaN one NaN)
except the one Float64 SUM / AVG test over data whose partial sums round, which holds the device to the bound the header states.  Row
counts and widths sit round one lane, one wave and one tile of the scans (kWinTileRows positions), one past the kWinTileRows tile
aggregates a round of the carry scan takes (forward and mirrored), and 2^24 rows.  The model runs with fast=True (cumulative sums and
slices); tests/test_window_frame_cpu.py holds that against the model's sequential loop."""
import math
from fractions import Fraction

import numpy as np
import pytest

import group_agg_model as A
import window_frame_model as F
import window_model as M
from rivulus_amd import capi
from rivulus_amd.capi import RV_BOOLEAN, RV_FLOAT64, RV_INT64, RV_STRING, Column, RvError
from test_window_gpu import ITEMS, TILE, WAVE, I64_MIN, compare, f64, frame, garbage_under_nulls, i64, upload

pytestmark = pytest.mark.gpu

RV_ERR_INVALID_ARG, RV_ERR_LENGTH_MISMATCH, RV_ERR_TYPE_MISMATCH, RV_ERR_OUT_OF_BOUNDS, RV_ERR_UNSUPPORTED = 1, 2, 3, 4, 5
ROW_COUNTS = [0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
WIDTHS = [1, 2, 3, 7, 8, 9, 63, 64, 65, 511, 512, 513, TILE - 1, TILE, TILE + 1]
U, BIG = None, 1 << 62  # an unbounded side; the largest finite offset
ALL_FLAGS = [0, 1, 2, 3]
AGGS = ("count", "sum", "min", "max", "avg")
OLD_OPS = [("row_number", 0), ("rank", 0), ("dense_rank", 0), ("cum_count", 2), ("cum_sum", 2), ("cum_sum", 3), ("cum_min", 3), ("cum_max", 2),
           ("lag", 2, 1), ("lead", 3, 2)]


@pytest.fixture(scope="module")
def ctx():
    with capi.Context(0) as c:
        yield c


def shapes(w):
    """the frames of width w (and w + 1 for the two that leave the row itself out)"""
    return [(w - 1, 0), (0, w - 1), (w // 2, w - 1 - w // 2), (w, -1), (-1, w)]


def check(ctx, cols, partition_by, order_by, exprs, offsets=None, fast=True, what=""):
    """fast: every Float64 cell that is summed is integer-valued and every partial sum representable (the model's cumulative sums);
    otherwise the model's loop, whose left fold the caller knows to be the one possible result"""
    want = F.window_frames(cols, partition_by, order_by, exprs, exact_float=fast, fast=fast)
    devs = [upload(ctx, c, offsets[i] if offsets else 0) for i, c in enumerate(cols)]
    got = ctx.window_frames(devs, partition_by, order_by, exprs)
    for e, g, w in zip(exprs, got, want):
        compare(g, w, f"{what} {e} partition {partition_by} order {order_by}")
    return got


def same_columns(a, b, what):
    """two device columns equal array for array: dtype, length, null count, bitmap, validity, cells"""
    ia, ib = a.info(), b.info()
    assert (ia.dtype, ia.length, ia.null_count, bool(ia.has_validity)) == (ib.dtype, ib.length, ib.null_count, bool(ib.has_validity)), what
    ha, hb = a.download(), b.download()
    assert (ha.validity is None) == (hb.validity is None) and (ha.validity is None or np.array_equal(ha.logical_valid(), hb.logical_valid())), what
    if ia.dtype == RV_STRING:
        assert ha.to_strings() == hb.to_strings(), what
    else:
        va, vb = ha.logical_values(), hb.logical_values()
        if ia.dtype == RV_FLOAT64:
            va, vb = va.view(np.uint64), vb.view(np.uint64)
        assert np.array_equal(va, vb), what


def aggregates(frames, int_col=2, float_col=3):
    return [(op, c, p, f) for p, f in frames for op in AGGS for c in (int_col, float_col)]


def partition_runs(lengths):
    return np.repeat(np.arange(len(lengths)), lengths).astype(np.int64)


# ---- row counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts(ctx, n):
    rng = np.random.default_rng(n)
    cols = frame(rng, n, 5)
    exprs = aggregates([(3, 0), (1, 1), (U, U)]) + [("sum", 2, 0, 2), ("min", 3, 2, -1), ("max", 2, -1, 2), ("first_value", 2, 2, 0), ("last_value", 3, 0, 2),
                                                    ("ntile", 0, 3), ("row_number", 0), ("cum_sum", 2)]
    check(ctx, cols, [0], [(1, 0)], exprs)
    check(ctx, cols, [], [], exprs, what="in place")
    if n:
        assert ctx.last_kernel() == "window_frame"


def test_zero_rows_have_the_right_dtypes(ctx):
    cols = [i64([]), f64([]), ("bool", np.zeros(0, bool), None), ("str", [], None)]
    got = check(ctx, cols, [0], [(1, 0)], [("count", 3, 1, 1), ("sum", 1, 1, 1), ("min", 0, 1, 1), ("avg", 0, 1, 1), ("first_value", 2, 1, 1),
                                          ("last_value", 3, 1, 1), ("ntile", 0, 4), ("max", 1, U, U)])
    assert [g.info().dtype for g in got] == [RV_INT64, RV_FLOAT64, RV_INT64, RV_FLOAT64, RV_BOOLEAN, RV_STRING, RV_INT64, RV_FLOAT64]


def clipped_series_sum(n, preceding, following):
    """SUM over [j - preceding, j + following] cut to [0, n) of x = row, in place"""
    j = np.arange(n, dtype=np.int64)
    lo, hi = np.maximum(0, j - preceding), np.minimum(n - 1, j + following)
    return (lo + hi) * (hi - lo + 1) // 2


def test_one_past_a_round_of_the_carry_scan(ctx):
    n = TILE * TILE + 1  # kWinTileRows tile aggregates and one more: the second round of the carry scan, forward and mirrored
    dev = ctx.upload(Column.from_numpy(np.arange(n, dtype=np.int64)))
    got = ctx.window_frames([dev], [], [], [("sum", 0, 5, 5)])
    compare(got[0], ("i64", clipped_series_sum(n, 5, 5), np.ones(n, bool)), "sum (5, 5)")


def test_2_24_rows(ctx):
    n = 1 << 24
    dev = ctx.upload(Column.from_numpy(np.arange(n, dtype=np.int64)))
    got = ctx.window_frames([dev], [], [], [("sum", 0, 1000, 1000), ("sum", 0, U, U)])
    compare(got[0], ("i64", clipped_series_sum(n, 1000, 1000), np.ones(n, bool)), "sum (1000, 1000)")
    compare(got[1], ("i64", np.full(n, n * (n - 1) // 2, np.int64), np.ones(n, bool)), "sum over everything")
    assert ctx.last_kernel() == "window_frame"


# ---- widths and partition lengths -------------------------------------------------------------------------------------------------------
def value_columns(rng, n):
    return [garbage_under_nulls(i64(rng.integers(-1000, 1000, n), rng.random(n) >= 0.3)),
            garbage_under_nulls(f64(rng.integers(-1000, 1000, n).astype(np.float64), rng.random(n) >= 0.3))]


def width_exprs(w):
    """every frame shape of width w as Int64 SUM and COUNT, three of them as Float64 MIN / SUM / AVG too, and FIRST / LAST"""
    out = []
    for k, (p, f) in enumerate(shapes(w)):
        out += [("sum", 1, p, f), ("count", 2, p, f)]
        if k in (0, 2, 4):
            out += [("min", 2, p, f), ("max", 1, p, f), ("sum", 2, p, f), ("avg", 2, p, f)]
        if k in (1, 3):
            out += [("first_value", 1, p, f), ("last_value", 2, p, f)]
    return out


@pytest.mark.parametrize("w", WIDTHS)
def test_widths_against_partition_lengths(ctx, w):
    """partitions of w - 1, w, w + 1, 2 w and 2 w + 1 rows (and one of 5), the last ending at the last row"""
    lengths = [x for x in (w - 1, w, w + 1, 2 * w, 5, 2 * w + 1) if x > 0]
    part = partition_runs(lengths)
    n = len(part)
    rng = np.random.default_rng(w)
    check(ctx, [i64(part)] + value_columns(rng, n), [0], [], width_exprs(w), what=f"w {w}")


@pytest.mark.parametrize("extra", [0, 1])
def test_widths_of_the_row_count_and_one_more(ctx, extra):
    n = TILE + 1
    rng = np.random.default_rng(extra)
    cols = [i64(np.zeros(n))] + value_columns(rng, n)
    check(ctx, cols, [0], [], width_exprs(n + extra), what=f"w rows + {extra}")
    check(ctx, cols, [], [], width_exprs(n + extra), what=f"in place, w rows + {extra}")


def test_unbounded_ends_and_offsets_of_2_62(ctx):
    n = TILE + 77
    rng = np.random.default_rng(21)
    part = partition_runs([1, 700, 1, n - 702])
    frames = [(U, 0), (0, U), (U, U), (U, -3), (-3, U), (U, 5), (5, U), (BIG, 0), (0, BIG), (BIG, BIG), (BIG, -BIG), (-BIG, BIG), (5, BIG), (BIG, -2), (U, BIG),
              (BIG, U), (U, -BIG), (-BIG, U)]
    exprs = [(op, c, p, f) for p, f in frames for op, c in (("sum", 1), ("count", 2), ("max", 2), ("avg", 1), ("first_value", 1), ("last_value", 2))]
    check(ctx, [i64(part)] + value_columns(rng, n), [0], [], exprs)
    check(ctx, [i64(part)] + value_columns(rng, n), [], [], exprs, what="in place")


# ---- shapes where a segmented scan goes wrong, forward or mirrored ----------------------------------------------------------------------
FRAME_EXPRS = [e for w in (3, 64, 700) for e in width_exprs(w)] + [("sum", 1, U, U), ("min", 2, U, 0), ("max", 2, 0, U), ("ntile", 0, 7)]


def test_one_partition_over_four_tiles(ctx):
    n = 4 * TILE + 13  # heads at 0 and at 3 * TILE + 500: tiles 1 and 2 hold no partition head
    rng = np.random.default_rng(1)
    part = (np.arange(n) >= 3 * TILE + 500).astype(np.int64)
    check(ctx, [i64(part)] + value_columns(rng, n), [0], [], FRAME_EXPRS + width_exprs(3 * TILE))


def test_every_row_its_own_partition(ctx):
    n = 2 * TILE + 3
    rng = np.random.default_rng(2)
    check(ctx, [i64(rng.permutation(n))] + value_columns(rng, n), [0], [], FRAME_EXPRS)


EDGES = [TILE - 1, TILE, TILE + 1, WAVE - 1, WAVE, WAVE + ITEMS - 1, WAVE + ITEMS, 2 * TILE - 1, 2 * TILE + 1]


@pytest.mark.parametrize("edge", EDGES)
def test_partition_heads_and_block_boundaries_at_the_edges_of_tiles_waves_and_threads(ctx, edge):
    n = 2 * TILE + 2
    rng = np.random.default_rng(edge)
    values = value_columns(rng, n)
    part = (np.arange(n) >= edge).astype(np.int64)  # two partitions: [0, edge) and [edge, n); the second ends at the last row
    check(ctx, [i64(part)] + values, [0], [], FRAME_EXPRS, what=f"head at {edge}")
    # one partition, width `edge`: a block boundary at position `edge`; width edge - 1 puts one at edge - 1
    check(ctx, [i64(np.zeros(n))] + values, [0], [], width_exprs(edge) + [("sum", 1, edge - 2, 0), ("min", 2, 0, edge - 2)], what=f"block boundary at {edge}")


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
    exprs = aggregates([(4, 0), (2, 3), (U, U)]) + [(op, 4, p, f) for op in ("count", "min", "max", "first_value", "last_value") for p, f in ((4, 0), (3, -1))] + \
        [("first_value", 2, 2, 2), ("last_value", 3, 2, 2), ("first_value", 3, U, U), ("last_value", 2, -1, 5), ("ntile", 0, 4), ("ntile", 0, 1000)]
    check(ctx, cols, [0], [(1, flags)], exprs, what="Int64 order key")
    check(ctx, cols, [0], [(4, flags), (1, flags ^ 1)], exprs, what="Float64 + Int64 order keys")


def test_inf_and_nan_reach_only_the_frames_that_hold_them(ctx):
    n = 3 * WAVE + 50  # integer-valued cells, one +inf and one NaN: a frame's sum is exact, +inf or NaN whatever the bracketing
    x = np.arange(n, dtype=np.float64)
    x[WAVE - 1], x[2 * WAVE] = np.inf, np.nan
    valid = np.ones(n, bool)
    valid[[5, WAVE, 2 * WAVE - 1]] = False
    cols = [i64(np.zeros(n)), garbage_under_nulls(f64(x, valid))]
    exprs = [(op, 1, p, f) for op in ("sum", "avg", "min", "max") for p, f in ((3, 0), (0, 3), (10, 10), (40, -1), (63, 0))]
    got = check(ctx, cols, [0], [], exprs, fast=False)
    s = got[0].download().logical_values()  # SUM over (3, 0)
    hit_inf, hit_nan = np.r_[WAVE - 1:WAVE + 3], np.r_[2 * WAVE:2 * WAVE + 4]
    assert np.isinf(s[hit_inf]).all() and np.isnan(s[hit_nan]).all() and np.isfinite(np.delete(s, np.r_[hit_inf, hit_nan])).all()


def test_int64_sum_wraps(ctx):
    n = 3 * WAVE + 5
    rng = np.random.default_rng(22)
    cols = [i64(rng.integers(0, 3, n)), i64(rng.integers(I64_MIN, (1 << 63) - 1, n, endpoint=True), rng.random(n) >= 0.1)]
    check(ctx, cols, [0], [], [("sum", 1, 7, 0), ("sum", 1, 64, 64), ("sum", 1, U, U), ("avg", 1, 3, 3), ("min", 1, 2, 2), ("max", 1, 2, 2)])


def test_count_first_and_last_over_boolean_and_string_columns(ctx):
    n, plen = 6 * 97, 97
    rng = np.random.default_rng(6)
    cols = [i64(np.arange(n) // plen), i64(rng.integers(-50, 50, n)), ("bool", rng.random(n) < 0.5, rng.random(n) >= 0.2),
            ("str", [f"v{i * 7 % 23}" * (i % 3) for i in range(n)], rng.random(n) >= 0.2), ("bool", rng.random(n) < 0.5, None), ("str", [f"w{i}" for i in range(n)], None),
            ("null", np.zeros(n, np.int64), None)]
    exprs = [(op, c, p, f) for op in ("count", "first_value", "last_value") for c in (2, 3, 4, 5, 6) for p, f in ((2, 0), (0, 2), (3, -2), (-1, plen), (U, U), (n + 1, n + 1))]
    check(ctx, cols, [0], [(1, 0)], exprs)
    check(ctx, cols, [], [], exprs[::2], what="in place")


@pytest.mark.parametrize("offset", [1, 63, 65])
def test_slices(ctx, offset):
    n = TILE + 9
    rng = np.random.default_rng(offset)
    cols = frame(rng, n, 7) + [("bool", rng.random(n) < 0.5, rng.random(n) >= 0.2), ("str", [f"s{i % 11}" for i in range(n)], rng.random(n) >= 0.2)]
    exprs = aggregates([(5, 1), (U, 0)]) + [("count", 4, 2, 2), ("count", 5, 2, 2), ("first_value", 4, 1, 1), ("last_value", 5, 1, 1), ("ntile", 0, 5), ("lag", 4, 1)]
    check(ctx, cols, [0], [(1, 0)], exprs, offsets=[offset, offset + 1, offset, 0, offset, offset])
    check(ctx, cols, [], [], exprs, offsets=[offset, offset + 1, offset, 0, offset, offset], what="in place")


def test_two_partition_keys_boolean_and_float_specials(ctx):
    n = TILE + 131
    rng = np.random.default_rng(5)
    nan2 = np.array([0x7FF8000000000001], np.uint64).view(np.float64)[0]
    fkey = rng.choice(np.array([0.0, -0.0, np.nan, -np.nan, nan2, 1.0, np.inf]), n)
    cols = [("bool", rng.random(n) < 0.5, rng.random(n) >= 0.2), garbage_under_nulls(f64(fkey, rng.random(n) >= 0.2)), i64(rng.integers(-9, 9, n), rng.random(n) >= 0.2),
            i64(rng.integers(-1000, 1000, n))]
    check(ctx, cols, [0, 1], [(2, 2)], [("sum", 3, 7, 0), ("max", 3, 2, 2), ("avg", 3, U, U), ("first_value", 0, 1, 0), ("count", 0, 3, 3), ("ntile", 0, 3), ("min", 1, 4, 4)])
    assert ctx.last_kernel() == "window_frame"


# ---- equivalences -----------------------------------------------------------------------------------------------------------------------
def test_the_old_ops_through_the_new_entry_point_equal_rv_window(ctx):
    n = TILE + 300
    rng = np.random.default_rng(30)
    model = frame(rng, n, 6)
    model[3] = garbage_under_nulls(f64(rng.uniform(-1, 1, n), rng.random(n) >= 0.2))  # a CUM_SUM whose partial sums round: the same kernels, the same bits
    cols = [upload(ctx, c) for c in model]
    for part, order in (([0], [(1, 0)]), ([], [])):
        old = ctx.window(cols, part, order, OLD_OPS)
        assert ctx.last_kernel() == "window_scan"
        new = ctx.window_frames(cols, part, order, OLD_OPS)
        assert ctx.last_kernel() == "window_scan"
        for e, a, b in zip(OLD_OPS, old, new):
            same_columns(a, b, f"{e} through both entry points")
        # the frame ops that say the same thing
        pairs = [(("count", 2, U, 0), ("cum_count", 2)), (("sum", 2, U, 0), ("cum_sum", 2)), (("min", 3, U, 0), ("cum_min", 3)), (("max", 2, U, 0), ("cum_max", 2)),
                 (("min", 2, U, 0), ("cum_min", 2)), (("max", 3, U, 0), ("cum_max", 3))]
        for k in (0, 1, 3, 700):
            pairs += [(("first_value", 3, k, -k), ("lag", 3, k)), (("first_value", 2, -k, k), ("lead", 2, k))]
        framed = ctx.window_frames(cols, part, order, [p[0] for p in pairs])
        classic = ctx.window(cols, part, order, [p[1] for p in pairs])
        for p, a, b in zip(pairs, framed, classic):
            same_columns(a, b, f"{p[0]} against {p[1]}")


def test_a_mixed_call_equals_one_call_per_expression(ctx):
    n = 2 * TILE + 77
    rng = np.random.default_rng(31)
    model = frame(rng, n, 9)
    cols = [upload(ctx, c) for c in model]
    exprs = OLD_OPS + aggregates([(6, 0), (100, 100), (TILE, -1)]) + [("first_value", 2, 6, 0), ("last_value", 3, 100, 100), ("ntile", 0, 4), ("sum", 2, U, U), ("min", 3, 0, U)]
    together = ctx.window_frames(cols, [0], [(1, 2)], exprs)
    for e, g, w in zip(exprs, together, F.window_frames(model, [0], [(1, 2)], exprs, exact_float=True, fast=True)):
        compare(g, w, f"mixed call {e}")
    for e, g in zip(exprs, together):
        same_columns(g, ctx.window_frames(cols, [0], [(1, 2)], [e])[0], f"{e} alone")


# ---- Float64 SUM / AVG ------------------------------------------------------------------------------------------------------------------
def test_float_sum_of_integer_valued_cells_is_bit_exact(ctx):
    n = 5 * TILE + 77  # |x| < 2^53 / rows: every partial sum of any bracketing is an integer below 2^53
    rng = np.random.default_rng(9)
    most = (1 << 53) // n
    x = rng.integers(-most + 1, most, n).astype(np.float64)
    x[rng.random(n) < 0.05] = -0.0
    cols = [i64(rng.integers(0, 3, n)), i64(rng.integers(0, 1 << 30, n)), garbage_under_nulls(f64(x, rng.random(n) >= 0.1))]
    exprs = [(op, 2, p, f) for op in ("sum", "avg") for p, f in ((6, 0), (1000, 1000), (U, U), (0, TILE), (U, -1))]
    check(ctx, cols, [0], [(1, 0)], exprs)
    check(ctx, cols, [], [], exprs, what="in place")


def test_float_sum_and_avg_within_the_stated_bound_and_the_same_bits_twice(ctx):
    """mixed-sign uniform data: |got - fsum(frame)| <= gamma_{m-1} x sum|x| over the frame, m its non-null cells (the header's bound: that
    of any summation order, tests/group_agg_model.gamma_bound), against math.fsum over the frame.  AVG is SUM / m by one division, so it is
    held to the correctly rounded quotient of the device's own SUM.  A frame of one or two cells has one correctly rounded sum and the bound
    leaves no room for another."""
    n = 3 * TILE + 11
    rng = np.random.default_rng(10)
    x = rng.uniform(-1.0, 1.0, n)
    valid = rng.random(n) >= 0.1
    cols = [i64((np.arange(n) >= TILE + 5).astype(np.int64)), garbage_under_nulls(f64(x, valid))]
    devs = [upload(ctx, c) for c in cols]
    frames = [(6, 0), (40, 40), (U, U), (1, 0), (0, 700)]
    exprs = [(op, 1, p, f) for p, f in frames for op in ("sum", "avg")]
    a = [g.download() for g in ctx.window_frames(devs, [0], [], exprs)]
    b = [g.download() for g in ctx.window_frames(devs, [0], [], exprs)]
    for e, u, v in zip(exprs, a, b):
        assert np.array_equal(u.logical_values().view(np.uint64), v.logical_values().view(np.uint64)), f"{e}: two calls over the same buffers differ"
    worst = Fraction(0)
    for k, (p, f) in enumerate(frames):
        s, avg = a[2 * k].logical_values(), a[2 * k + 1]
        avg_values, avg_valid = avg.logical_values(), avg.logical_valid() if avg.validity is not None else np.ones(n, bool)
        cells = F.frame_cells(cols, [0], [], 1, p, f)
        for row in range(0, n, 53 if p is not U else 997):
            c = cells[row]
            exact, bound = math.fsum(c), A.gamma_bound(c)
            err = abs(Fraction(float(s[row])) - Fraction(exact))
            assert err <= bound, f"SUM ({p}, {f}) row {row} ({len(c)} cells): |{s[row]!r} - {exact!r}| = {float(err):.3e} > {float(bound):.3e}"
            worst = max(worst, err / bound if bound else Fraction(0))
            assert bool(avg_valid[row]) == (len(c) > 0)
            if c:
                assert avg_values[row] == s[row] / len(c), f"AVG ({p}, {f}) row {row}"
    print(f"worst error / bound: {float(worst):.3e}")


# ---- random cases -----------------------------------------------------------------------------------------------------------------------
def test_150_random_cases(ctx):
    rng = np.random.default_rng(150)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0, -7.0, 0.5])
    for case in range(150):
        n = int(rng.choice([1, 2, 5, 64, 65, 200, 700, TILE + 3, 5000], p=[.1, .1, .15, .1, .1, .15, .15, .1, .05]))
        mask = lambda p=0.25: (rng.random(n) >= p) if rng.random() < 0.7 else None
        cols = [i64(rng.integers(0, int(rng.choice([1, 2, 5, 50])), n), mask()), ("bool", rng.random(n) < 0.5, mask()),
                f64(rng.choice(specials, n), mask()), i64(rng.integers(-4, 4, n), mask()),
                garbage_under_nulls(i64(rng.integers(I64_MIN, (1 << 63) - 1, n, endpoint=True), mask())),
                garbage_under_nulls(f64(rng.integers(-99, 99, n).astype(np.float64), mask())), ("str", [f"x{i % 5}" for i in range(n)], mask()),
                ("null", np.zeros(n, np.int64), None)]
        partition_by = [int(c) for c in rng.choice([0, 1, 2, 7], int(rng.integers(0, 3)), replace=False)]
        order_by = [(int(c), int(rng.integers(0, 4))) for c in rng.choice([2, 3, 5, 7], int(rng.integers(0, 3)), replace=False)]

        def a_frame():
            w = int(rng.choice(WIDTHS + [n, n + 1]))
            return (shapes(w) + [(U, 0), (0, U), (U, U), (U, w), (w, U), (BIG, w), (-w, BIG)])[int(rng.integers(0, 12))]

        ops = [("row_number", 0), ("rank", 1), ("dense_rank", 6), ("cum_sum", 5), ("cum_max", 2), ("lag", int(rng.integers(0, 8)), int(rng.integers(0, 4))),
               ("ntile", 0, int(rng.choice([1, 2, 3, 7, 64, n + 1]))), ("count", int(rng.integers(0, 8)), *a_frame()), ("sum", 4, *a_frame()), ("sum", 5, *a_frame()),
               ("min", 2, *a_frame()), ("max", 2, *a_frame()), ("min", 4, *a_frame()), ("max", 5, *a_frame()), ("avg", 4, *a_frame()), ("avg", 5, *a_frame()),
               ("first_value", int(rng.integers(0, 8)), *a_frame()), ("last_value", int(rng.integers(0, 8)), *a_frame())]
        exprs = [ops[i] for i in rng.choice(len(ops), int(rng.integers(1, 7)), replace=False)]
        check(ctx, cols, partition_by, order_by, exprs, what=f"case {case}")


def test_last_kernel(ctx):
    cols = [upload(ctx, i64(np.arange(100) % 3)), upload(ctx, i64(np.arange(100)))]
    for exprs, name in (([("sum", 1, 1, 1)], "window_frame"), ([("ntile", 0, 3)], "window_frame"), ([("first_value", 1, 1, 1)], "window_frame"),
                        ([("lag", 1, 1), ("count", 1, U, U)], "window_frame"), ([("cum_sum", 1)], "window_scan"), ([("lag", 1, 1)], "window_shift")):
        ctx.window_frames(cols, [0], [], exprs)
        assert ctx.last_kernel() == name, exprs


# ---- errors: each leaves the context usable and creates nothing ---------------------------------------------------------------------------
def test_errors_are_followed_by_a_good_call(ctx):
    n = 100
    rng = np.random.default_rng(11)
    model = frame(rng, n, 4) + [("bool", rng.random(n) < 0.5, None), ("str", [f"s{i % 3}" for i in range(n)], None)]
    cols = [upload(ctx, c) for c in model]
    short = upload(ctx, i64(np.arange(n - 1)))
    good_exprs = [("row_number", 0), ("sum", 2, 3, 0), ("avg", 3, 1, 1)]

    want = F.window_frames(model, [0], [(1, 0)], good_exprs, exact_float=True)

    def good():
        for g, w in zip(ctx.window_frames(cols, [0], [(1, 0)], good_exprs), want):
            compare(g, w, "the call after an error")

    def refused(status, text, *args):
        with pytest.raises(RvError) as e:
            ctx.window_frames(*args)
        assert e.value.status == status and text in e.value.message, e.value
        assert "rv_window_frames" in e.value.message or status == RV_ERR_LENGTH_MISMATCH, e.value  # the batch check names no caller
        good()

    refused(RV_ERR_INVALID_ARG, "no window expressions", cols, [0], [], [])
    refused(RV_ERR_INVALID_ARG, "expression 1 has the unknown op 17", cols, [0], [], [("sum", 2, 1, 1), (17, 0, 0, 0, 0)])
    for p, f in ((1, -2), (-1, 0), (0, -1), (-BIG, BIG - 1), (BIG + 1, 0), (0, BIG + 1), (-BIG - 1, F.UNBOUNDED), (F.UNBOUNDED, -BIG - 1), (0, -(1 << 63))):
        for op in ("count", "sum", "min", "max", "avg", "first_value", "last_value"):
            refused(RV_ERR_INVALID_ARG, "expression 1: a frame's finite offsets", cols, [0], [], [("row_number", 0), (op, 2, p, f)])
    refused(RV_ERR_INVALID_ARG, "expression 0: NTILE of 0 buckets", cols, [0], [], [("ntile", 0, 0)])
    refused(RV_ERR_INVALID_ARG, "reads column 6 of 6", cols, [0], [], [("sum", 6, 1, 1)])
    refused(RV_ERR_INVALID_ARG, "partition key 0 is column 7", cols, [7], [], [("ntile", 0, 2)])
    refused(RV_ERR_INVALID_ARG, "order key 0 is column 6", cols, [], [(6, 0)], [("ntile", 0, 2)])
    refused(RV_ERR_INVALID_ARG, "unknown flag bits", cols, [], [(1, 4)], [("ntile", 0, 2)])
    refused(RV_ERR_INVALID_ARG, "key columns", cols, [0] * 9, [], [("ntile", 0, 2)])
    refused(RV_ERR_INVALID_ARG, "order keys", cols, [], [(1, 0)] * 9, [("ntile", 0, 2)])
    refused(RV_ERR_LENGTH_MISMATCH, "length", cols + [short], [0], [], [("ntile", 0, 2)])
    refused(RV_ERR_UNSUPPORTED, "String keys go through rv_string_dict_build", cols, [5], [], [("ntile", 0, 2)])
    refused(RV_ERR_UNSUPPORTED, "Boolean and String sort keys are not built", cols, [], [(4, 0)], [("ntile", 0, 2)])
    refused(RV_ERR_UNSUPPORTED, "Boolean and String sort keys are not built", cols, [], [(5, 0)], [("ntile", 0, 2)])
    for op in ("sum", "min", "max", "avg"):
        refused(RV_ERR_TYPE_MISMATCH, "SUM / MIN / MAX / AVG take an Int64 or Float64 column", cols, [0], [], [(op, 4, 1, 1)])
        refused(RV_ERR_TYPE_MISMATCH, "SUM / MIN / MAX / AVG take an Int64 or Float64 column", cols, [0], [], [(op, 5, 1, 1)])
    for op in ("cum_sum", "cum_min", "cum_max"):
        refused(RV_ERR_TYPE_MISMATCH, "CUM_SUM / CUM_MIN / CUM_MAX take an Int64 or Float64 column", cols, [0], [], [(op, 4)])
    ctx.set_option("agg_max_groups", 3)
    try:  # four partitions
        with pytest.raises(RvError) as e:
            ctx.window_frames(cols, [0], [], [("ntile", 0, 2)])
        assert e.value.status == RV_ERR_UNSUPPORTED and "agg_max_groups" in e.value.message, e.value
    finally:
        ctx.set_option("agg_max_groups", 0)
    good()
    lib = capi.load()
    out = (capi.C.c_void_p * 1)()
    spec = (capi.RvWindowFrameSpec * 1)()
    assert lib.rv_window_frames(ctx.handle, None, 1, None, 0, None, None, 0, spec, 1, out) == RV_ERR_INVALID_ARG
    assert lib.rv_window_frames(ctx.handle, capi._handles(cols), len(cols), None, 1, None, None, 0, spec, 1, out) == RV_ERR_INVALID_ARG
    assert lib.rv_window_frames(ctx.handle, capi._handles(cols), len(cols), None, 0, None, None, 0, None, 1, out) == RV_ERR_INVALID_ARG
    assert lib.rv_window_frames(ctx.handle, capi._handles(cols), len(cols), None, 0, None, None, 0, spec, 1, None) == RV_ERR_INVALID_ARG
    good()
