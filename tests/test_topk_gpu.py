"""GPU suite: rv_top_k_indices / rv_top_k against tests/topk_model.py.  The result is the sort's cut at k and the sort is stable, so EVERY
comparison here is exact equality with the model's -- no tolerance anywhere.  The path a call takes is asserted too: rv_ctx_last_kernel and
the read-only options "top_k_last_passes" / "top_k_last_candidates" against the model's restatement of the select.  The select is forced at
small row counts by option "top_k_select_from_rows" = 1; row counts sit round one lane, one wave, one tile of the collect
(rvk::kTopKTileRows), and one past a single sweep of the grid-strided histogram kernel (8 workgroups of 256 rows per CU)."""
import numpy as np
import pytest

import sort_model as M
import topk_model as T
from helpers import const
from rivulus_amd import capi
from rivulus_amd.capi import RV_INT64, Column, RvError

pytestmark = pytest.mark.gpu

RV_ERR_INVALID_ARG, RV_ERR_LENGTH_MISMATCH, RV_ERR_UNSUPPORTED = 1, 2, 5
TILE = 256 * const("kTopKCollectRowsPerLane")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ALL_FLAGS = [0, 1, 2, 3]
HUGE = 1 << 40  # a divisor no candidate count stays under: refine to the last differing position


@pytest.fixture(scope="module")
def ctx():
    with capi.Context(0) as c:
        yield c


@pytest.fixture(autouse=True)
def forced_select(ctx):
    """every test starts with the select forced at any row count and the built-in divisor, and leaves the built-in values behind"""
    ctx.set_option("top_k_select_from_rows", 1)
    ctx.set_option("top_k_refine_divisor", 0)
    yield
    ctx.set_option("top_k_select_from_rows", 0)
    ctx.set_option("top_k_refine_divisor", 0)


# ---- building inputs ----------------------------------------------------------------------------------------------------------------
def upload(ctx, col, offset=0):
    """The device column of a model column (dtype, values, valid); offset > 0: a slice at that element (and validity bit) offset of a longer
    upload whose other cells are valid and hold 77."""
    dtype, values, valid = col
    n = len(values)
    if dtype == "null":
        return ctx.upload(Column.nulls(n))
    if offset:
        fill = np.full(offset, 77, values.dtype)
        values = np.concatenate([fill, values, fill[:3]])
        valid = np.concatenate([np.ones(offset, bool), np.ones(n, bool) if valid is None else valid, np.ones(min(3, offset), bool)])
    dev = ctx.upload(Column.from_numpy(values, valid))
    return dev.slice(offset, n) if offset else dev


def indices_of(dev, rows):
    info = dev.info()
    assert info.dtype == RV_INT64 and info.length == rows and info.offset == 0 and info.null_count == 0 and info.has_validity == 0
    return dev.download().logical_values()


def settings(ctx):
    return (ctx.get_option("top_k_select_from_rows") or const("kTopKSelectFromRows"), ctx.get_option("top_k_refine_divisor") or const("kTopKRefineDivisor"))


def assert_path(ctx, s, n, what=""):
    """the context's account of the last call against the model's Select"""
    assert ctx.get_option("top_k_last_passes") == s.passes, (what, "passes", s.passes)
    assert ctx.get_option("top_k_last_candidates") == s.count, (what, "candidates", s.count)
    if s.passes:
        assert ctx.last_kernel() == "topk_collect", what
    elif s.count:
        assert ctx.last_kernel().startswith("sort_") or ctx.last_kernel().startswith("rocprim"), (what, ctx.last_kernel())


def check(ctx, col, k, flags=0, offset=0, what=""):
    """One rv_top_k_indices call against the model -- result and path; returns (indices, the model's Select)."""
    n = len(col[1])
    want = T.top_k_indices(col, flags, min(k, n))
    s = T.select(col, flags, k, *settings(ctx))
    got = indices_of(ctx.top_k_indices(upload(ctx, col, offset), k, flags=flags), min(k, n))
    assert np.array_equal(got, want), f"{what} n {n} k {k} flags {flags} offset {offset}: first difference at {np.flatnonzero(got != want)[:5]}"
    assert_path(ctx, s, n, f"{what} n {n} k {k} flags {flags}")
    return got, s


def i64(values, valid=None):
    return "i64", np.asarray(values, np.int64), valid


def f64_bits(bits, valid=None):
    return "f64", np.asarray(bits, np.uint64).view(np.float64), valid


def random_i64(rng, n):
    return rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)


# ---- row counts and k ---------------------------------------------------------------------------------------------------------------
def row_counts(ctx):
    sweep = ctx.device_info()["compute_units"] * 8 * 256
    return [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, sweep + 1]


def test_row_counts(ctx):
    for n in row_counts(ctx):
        rng = np.random.default_rng(n)
        wide, few = i64(random_i64(rng, n)), i64(rng.integers(0, 50, n), rng.random(n) >= 0.3 if n else None)
        for k in sorted({0, 1, 2, max(0, n // 3), n}):
            check(ctx, wide, k, what="random 64-bit")
            check(ctx, few, k, flags=3, what="few values, nulls")


def test_the_select_runs_at_every_row_count_it_can(ctx):
    """2k < n with distinct keys: the model says select, so the counts above are not all the fallback's"""
    for n in [3, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]:
        rng = np.random.default_rng(n)
        _, s = check(ctx, i64(rng.permutation(n) - n // 2), 1)
        assert s.selected and s.passes >= 1 and s.count >= 1


@pytest.mark.parametrize("n", [1, 2, 5, 300, TILE + 7])
def test_every_k(ctx, n):
    rng = np.random.default_rng(n)
    col = i64(rng.integers(-40, 40, n), rng.random(n) >= 0.2)
    for k in sorted({0, 1, 2, max(0, n // 2 - 1), n // 2, n - 1, n, n + 1, 1 << 63}):
        for flags in ALL_FLAGS:
            got, _ = check(ctx, col, k, flags)
            assert len(got) == min(k, n)


def test_k_at_a_bin_edge_and_one_past_it(ctx):
    """values 0..9, 30 rows each, in the lowest byte: k = 60 ends exactly with the last row of bin 1, k = 61 takes the first row of bin 2"""
    rng = np.random.default_rng(1)
    v = np.repeat(np.arange(10), 30)
    rng.shuffle(v)
    for flags in (0, 1):
        _, s = check(ctx, i64(v), 60, flags)
        assert s.selected and s.count == 60
        _, s = check(ctx, i64(v), 61, flags)
        assert s.selected and s.count == 90
        _, s = check(ctx, i64(v), 59, flags)
        assert s.selected and s.count == 60


# ---- keys ---------------------------------------------------------------------------------------------------------------------------
def test_all_equal_keeps_row_order_and_refines_nothing(ctx):
    n = 2 * TILE + 5
    for flags in ALL_FLAGS:
        got, s = check(ctx, i64(np.full(n, -12345)), 7, flags)
        assert np.array_equal(got, np.arange(7)) and not s.selected, "every row ties with the cut: the whole (pass-free) sort"
    # all equal but for nulls in front: the nulls alone are candidates, one pass, no refinement
    valid = np.ones(n, bool)
    valid[[5, 900, 4000]] = False
    got, s = check(ctx, i64(np.full(n, 3), valid), 2)
    assert got.tolist() == [5, 900] and s.selected and s.passes == 1 and s.count == 3
    # ... and the equal values behind a few nulls: every value ties, more than half the rows
    got, s = check(ctx, i64(np.full(n, 3), valid), 6)
    assert got.tolist() == [5, 900, 4000, 0, 1, 2] and not s.selected


def test_two_distinct_values(ctx):
    rng = np.random.default_rng(2)
    n = 3 * TILE + 7
    v = np.where(rng.random(n) < 0.2, -(1 << 40), 1 << 50)
    for flags in ALL_FLAGS:
        check(ctx, i64(v), 100, flags)
        check(ctx, i64(v), int((v == -(1 << 40)).sum()), flags)
        check(ctx, i64(v), int((v == -(1 << 40)).sum()) + 1, flags)


@pytest.mark.parametrize("shift", [0, 56])
def test_one_differing_byte(ctx, shift):
    """shift 56: negative and positive Int64 that differ in nothing but the top byte -- the position with nothing above it"""
    rng = np.random.default_rng(shift)
    base = np.uint64(0x0123456789ABCDEF & ~(0xFF << shift))
    v = (base | (rng.integers(0, 256, 2 * TILE + 3, dtype=np.uint64) << np.uint64(shift))).view(np.int64)
    if shift == 56:
        assert (v < 0).any() and (v > 0).any()
    for flags in (0, 1):
        _, s = check(ctx, i64(v), 40, flags)
        assert s.selected and s.passes == 1


def test_signs_in_the_top_byte_then_refined(ctx):
    rng = np.random.default_rng(3)
    v = random_i64(rng, 3 * TILE + 1)
    ctx.set_option("top_k_refine_divisor", HUGE)
    for flags in (0, 1):
        _, s = check(ctx, i64(v), 5, flags)
        assert s.selected and s.passes == 8 and s.count == 5


def test_int_extremes(ctx):
    rng = np.random.default_rng(4)
    n = 2 * TILE + 9
    v = rng.choice(np.array([I64_MIN, I64_MAX, -1, 0, 1, I64_MIN + 1, I64_MAX - 1], np.int64), n, p=[0.02, 0.02, 0.2, 0.2, 0.2, 0.18, 0.18])
    for flags in ALL_FLAGS:
        for k in (1, int((v == I64_MIN).sum()), int((v == I64_MIN).sum()) + 1, int((v == I64_MAX).sum()) + 1, 300):
            check(ctx, i64(v, rng.random(n) >= 0.05), k, flags)


def test_refine_to_the_last_position_and_stop_after_the_first(ctx):
    rng = np.random.default_rng(5)
    col = i64(random_i64(rng, 4 * TILE + 1))
    ctx.set_option("top_k_refine_divisor", HUGE)
    _, deep = check(ctx, col, 10)
    ctx.set_option("top_k_refine_divisor", 1)
    _, shallow = check(ctx, col, 10)
    assert deep.passes == 8 and deep.count == 10 and shallow.passes == 1 and shallow.count > 10
    ctx.set_option("top_k_refine_divisor", 0)
    _, built_in = check(ctx, col, 10)
    assert 1 <= built_in.passes <= 8 and built_in.count <= max(10, len(col[1]) // const("kTopKRefineDivisor"))


def test_sorted_and_reverse_sorted(ctx):
    n = 3 * TILE + 17
    asc = np.arange(n, dtype=np.int64) * 1000003 - 10 ** 9
    for v in (asc, asc[::-1].copy()):
        for flags in (0, 1):
            check(ctx, i64(v), 33, flags)


# ---- Float64 ------------------------------------------------------------------------------------------------------------------------
NANS = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF,
                 0x7FF8000000001234], np.uint64)


def test_zeros_on_either_side_of_the_cut(ctx):
    rng = np.random.default_rng(6)
    n = 2 * TILE + 3
    v = np.abs(rng.standard_normal(n)) + 1.0
    minus, plus = [7, 500, 3000], [2, 600, 2999, 4000]
    v[minus], v[plus] = -0.0, 0.0
    got, _ = check(ctx, ("f64", v, None), 3)
    assert got.tolist() == minus, "every -0.0 before any +0.0"
    got, _ = check(ctx, ("f64", v, None), 4)
    assert got.tolist() == minus + plus[:1]
    got, _ = check(ctx, ("f64", v, None), 2)
    assert got.tolist() == minus[:2]
    # negated and descending: +0.0 (where -0.0 was) is the largest cell, -0.0 (where +0.0 was) the next
    got, _ = check(ctx, ("f64", -v, None), 4, flags=1)
    assert got.tolist() == minus + plus[:1]


def test_infinities(ctx):
    rng = np.random.default_rng(7)
    n = 2 * TILE + 11
    v = rng.standard_normal(n)
    v[[3, 700]] = -np.inf
    v[[4, 800, 900]] = np.inf
    got, _ = check(ctx, ("f64", v, None), 3)
    assert got[:2].tolist() == [3, 700]
    got, _ = check(ctx, ("f64", v, None), 2, flags=1)
    assert got.tolist() == [4, 800]
    check(ctx, ("f64", v, rng.random(n) >= 0.1), 50, flags=3)


def test_the_cut_inside_the_nan_class(ctx):
    rng = np.random.default_rng(8)
    n = 2 * TILE + 31
    bits = rng.standard_normal(n).view(np.uint64).copy()
    where = np.flatnonzero(rng.random(n) < 0.1)
    bits[where] = NANS[np.arange(len(where)) % len(NANS)]
    k = len(where) // 2
    got, s = check(ctx, f64_bits(bits), k, flags=1)
    assert np.array_equal(got, where[:k]) and s.selected and s.count == len(where), "descending: the NaNs first, of both signs and every payload, in row order"
    got, _ = check(ctx, f64_bits(bits), n - k, flags=0)  # ascending, the cut inside the NaNs at the far end: the whole sort
    assert np.array_equal(got[n - len(where):], where[:len(where) - k])


def test_float_descending(ctx):
    rng = np.random.default_rng(9)
    n = 3 * TILE + 1
    v = rng.standard_normal(n) * 1e-300
    for flags in ALL_FLAGS:
        check(ctx, ("f64", v, rng.random(n) >= 0.2), 77, flags)


# ---- nulls --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_null_counts_round_k(ctx, flags):
    """m < k, m == k, m > k under every flag combination; nulls last with v < k is the whole sort"""
    rng = np.random.default_rng(10 + flags)
    n = 2 * TILE + 77
    m = 40
    valid = np.ones(n, bool)
    valid[rng.choice(n, m, replace=False)] = False
    for col in (i64(rng.integers(-5000, 5000, n), valid), ("f64", rng.standard_normal(n), valid)):
        for k in (m - 1, m, m + 1, 3 * m):
            _, s = check(ctx, col, k, flags)
            assert s.selected
            if not flags & M.NULLS_LAST:
                assert (s.count == m) == (k <= m), "the nulls alone while they suffice"
    few_values = ~valid  # v = 40, m = n - 40
    for k in (39, 40, 41):
        _, s = check(ctx, i64(rng.integers(-5000, 5000, n), few_values), k, flags)
        if flags & M.NULLS_LAST:
            assert s.selected == (k <= 40), "nulls last: fewer values than k is the whole sort"


def test_garbage_under_nulls_changes_nothing(ctx):
    rng = np.random.default_rng(14)
    n = 3 * TILE + 5
    valid = rng.random(n) >= 0.1
    v = rng.integers(-1000, 1000, n)
    for flags in ALL_FLAGS:
        runs = []
        for _ in range(2):
            got, s = check(ctx, i64(np.where(valid, v, random_i64(rng, n)), valid), 500, flags)
            runs.append((got, s.passes, s.count))
        assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1:] == runs[1][1:]
    fv = rng.standard_normal(n)
    runs = [check(ctx, ("f64", np.where(valid, fv, fill), valid), 500, 2)[0] for fill in (np.nan, -np.inf)]
    assert np.array_equal(runs[0], runs[1])


def test_null_column(ctx):
    for flags in ALL_FLAGS:
        got, s = check(ctx, ("null", np.zeros(TILE + 3, np.int64), None), 9, flags)
        assert np.array_equal(got, np.arange(9)) and not s.selected


@pytest.mark.parametrize("offset", [1, 63, 65])
def test_slices_of_key_and_validity(ctx, offset):
    rng = np.random.default_rng(offset)
    n = 2 * TILE + 13
    for flags in ALL_FLAGS:
        _, s = check(ctx, i64(rng.integers(-30000, 30000, n), rng.random(n) >= 0.05), 300, flags, offset=offset)
        assert s.selected
    check(ctx, ("f64", rng.standard_normal(n), rng.random(n) >= 0.25), 200, 1, offset=offset)


# ---- rv_top_k -----------------------------------------------------------------------------------------------------------------------
def check_frame(ctx, cols, extra_host, keys, k):
    """rv_top_k against the model's rows gathered by rv_take; returns the model's Select of the first key"""
    n = len(cols[0][1])
    host = [Column.from_numpy(c[1], c[2]) if c[0] != "null" else Column.nulls(n) for c in cols] + extra_host
    devs = [ctx.upload(h) for h in host]
    perm = T.top_k_frame(cols, keys, min(k, n))
    s = T.select(cols[keys[0][0]], keys[0][1], k, *settings(ctx))
    outs = ctx.top_k(devs, keys, k)
    assert_path(ctx, s, n, f"frame keys {keys} k {k}")
    expect = ctx.take(devs, perm)
    for j, (o, e) in enumerate(zip(outs, expect)):
        assert o.info().length == len(perm)
        assert o.download().same_as(e.download()) is None, (j, keys, k)
    return s, outs, perm


def test_second_key_decides_ties_that_straddle_the_cut(ctx):
    """k0 ties over rows 0..199 at the cut; k1 DESCENDS with the row, so cutting the ties by row order before k1 is applied answers wrongly"""
    n = 1000
    k0 = np.where(np.arange(n) < 200, 5, 9 + np.arange(n) % 7)
    k0[[300, 301]] = 1
    k1 = -np.arange(n)
    s, outs, perm = check_frame(ctx, [i64(k0), i64(k1)], [], [(0, 0), (1, 0)], 12)
    assert s.selected and s.count == 202
    assert perm.tolist() == [301, 300] + list(range(199, 189, -1))
    assert outs[1].download().logical_values().tolist() == [-301, -300] + [-row for row in range(199, 189, -1)]
    # in row order where the second key says so
    s, _, perm = check_frame(ctx, [i64(k0), i64(np.zeros(n, np.int64))], [], [(0, 0), (1, 1)], 12)
    assert perm.tolist() == [300, 301] + list(range(10))


def test_three_keys_and_columns_riding_along(ctx):
    rng = np.random.default_rng(15)
    n = TILE + 99
    cols = [i64(rng.integers(0, 40, n), rng.random(n) >= 0.02), ("f64", rng.integers(0, 5, n).astype(np.float64) - 2.0, rng.random(n) >= 0.1),
            i64(rng.integers(-3, 3, n))]
    strings = [None if i % 7 == 3 else f"s{i % 13}" * (i % 3) for i in range(n)]
    extra = [Column.from_numpy(rng.random(n) < 0.5, rng.random(n) >= 0.2), Column.from_strings(strings), Column.nulls(n)]
    for keys in ([(0, 0), (1, 1), (2, 3)], [(0, 1), (2, 2), (1, 0)], [(1, 2)]):
        for k in (0, 1, 50, n // 2 - 1, n, n + 5):
            s, outs, perm = check_frame(ctx, cols, extra, keys, k)
            assert outs[4].download().to_strings() == [strings[i] for i in perm]
    s, _, _ = check_frame(ctx, cols, extra, [(0, 0), (1, 1), (2, 3)], 50)
    assert s.selected
    one = ctx.top_k([ctx.upload(Column.from_numpy(cols[2][1]))], [0], 5)  # a key by index alone: flags 0
    assert one[0].download().logical_values().tolist() == np.sort(cols[2][1], kind="stable")[:5].tolist()


def test_k_zero_gives_zero_row_columns_of_the_right_dtypes(ctx):
    host = [Column.from_numpy(np.arange(10, dtype=np.int64)), Column.from_numpy(np.arange(10) * 0.5), Column.from_numpy(np.arange(10) % 2 == 0),
            Column.from_strings([str(i) for i in range(10)]), Column.nulls(10)]
    devs = [ctx.upload(h) for h in host]
    outs = ctx.top_k(devs, [(1, 1)], 0)
    assert [o.info().dtype for o in outs] == [h.dtype for h in host] and all(o.info().length == 0 for o in outs)
    idx = ctx.top_k_indices(devs[0], 0)
    assert idx.info().dtype == RV_INT64 and idx.info().length == 0
    empty = ctx.top_k_indices(ctx.upload(Column.from_numpy(np.zeros(0, np.int64))), 5)
    assert empty.info().dtype == RV_INT64 and empty.info().length == 0


# ---- both sides of each switch ------------------------------------------------------------------------------------------------------
def test_select_from_rows_switch(ctx):
    ctx.set_option("top_k_select_from_rows", 0)
    edge = const("kTopKSelectFromRows")
    rng = np.random.default_rng(16)
    for n, selected in ((edge - 1, False), (edge, True), (edge + 1, True)):
        _, s = check(ctx, i64(random_i64(rng, n)), 100)
        assert s.selected == selected, n


def test_k_just_below_and_at_half_the_rows(ctx):
    rng = np.random.default_rng(17)
    n = 2 * TILE
    col = i64(rng.permutation(n) * 3 - n)
    _, s = check(ctx, col, n // 2 - 1)
    assert s.selected and s.count == n // 2 - 1
    _, s = check(ctx, col, n // 2)
    assert not s.selected
    _, s = check(ctx, i64(col[1][:n - 1]), n // 2 - 1)  # odd n: 2k = n - 1 < n
    assert s.selected


def test_low_cardinality_key_falls_back_after_the_last_pass(ctx):
    rng = np.random.default_rng(18)
    n = 3 * TILE + 3
    v = np.where(rng.random(n) < 0.7, 256, 513)  # two positions differ; the cut's bin holds 70 % of the rows whatever is refined
    _, s = check(ctx, i64(v), 10)
    assert not s.selected and ctx.last_kernel().startswith("sort_")
    _, s = check(ctx, i64(v), 10, flags=1)  # descending: the 30 % come first
    assert s.selected and s.count == int((v == 513).sum())


def test_candidate_count_against_the_divisor(ctx):
    rng = np.random.default_rng(19)
    n = 32 * 300
    col = i64(rng.integers(0, 1 << 16, n))
    for divisor in (8, const("kTopKRefineDivisor"), 128):
        ctx.set_option("top_k_refine_divisor", divisor)
        _, s = check(ctx, col, 20)
        assert s.selected and (s.count <= n // divisor or s.passes == 2), "two differing positions: at most two passes"


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def good_call(ctx):
    got, _ = check(ctx, i64([3, 1, 2, 1, 9, 8, 7]), 2)
    assert got.tolist() == [1, 3]


def sort_error(call):
    with pytest.raises(RvError) as e:
        call()
    return e.value.status, e.value.message


def test_indices_errors_are_the_sort_s(ctx):
    for col in (Column.from_numpy(np.array([True, False])), Column.from_strings(["b", "a"])):
        dev = ctx.upload(col)
        status, text = sort_error(lambda: ctx.top_k_indices(dev, 1))
        want_status, want_text = sort_error(lambda: ctx.sort_indices(dev))
        assert status == want_status == RV_ERR_UNSUPPORTED and text == want_text.replace("rv_sort_indices", "rv_top_k_indices")
        good_call(ctx)
    dev = upload(ctx, i64([1, 2]))
    status, text = sort_error(lambda: ctx.top_k_indices(dev, 1, flags=4))
    want_status, want_text = sort_error(lambda: ctx.sort_indices(dev, flags=4))
    assert status == want_status == RV_ERR_INVALID_ARG and text == want_text.replace("rv_sort_indices", "rv_top_k_indices")
    good_call(ctx)


def test_frame_errors_are_the_sort_s(ctx):
    a, b = upload(ctx, i64([2, 1, 3])), upload(ctx, i64([1, 2, 3, 4]))
    s, t = ctx.upload(Column.from_strings(["x", "y", "z"])), ctx.upload(Column.from_numpy(np.array([True, False, True])))
    for cols, keys, want in [([a], [], RV_ERR_INVALID_ARG), ([a], [1], RV_ERR_INVALID_ARG), ([a], [(0, 4)], RV_ERR_INVALID_ARG),
                             ([a, b], [0], RV_ERR_LENGTH_MISMATCH), ([a, s], [1], RV_ERR_UNSUPPORTED), ([a, t], [(1, 1)], RV_ERR_UNSUPPORTED)]:
        status, text = sort_error(lambda: ctx.top_k(cols, keys, 2))
        sort_status, sort_text = sort_error(lambda: ctx.sort(cols, keys))
        assert status == sort_status == want, (keys, text)
        assert text == sort_text.replace("rv_sort", "rv_top_k"), "the same text under this function's name"
        out = ctx.top_k([a, s], [0], 2)
        assert out[0].download().logical_values().tolist() == [1, 2] and out[1].download().to_strings() == ["y", "x"]
    good_call(ctx)


def test_read_only_options(ctx):
    for name in ("top_k_last_passes", "top_k_last_candidates"):
        with pytest.raises(RvError):
            ctx.set_option(name, 1)
    with pytest.raises(RvError):
        ctx.set_option("top_k_refine_divisor", -1)
    good_call(ctx)


# ---- random cases, determinism, timer ---------------------------------------------------------------------------------------------------
def random_case(rng):
    n = int(rng.integers(0, 20001))
    card = int(rng.integers(1, max(2, n + 1)))
    is_float = rng.random() < 0.5
    pool = random_i64(rng, card) if rng.random() < 0.5 else rng.integers(0, max(1, card), card)
    v = pool[rng.integers(0, card, n)] if n else np.zeros(0, np.int64)
    share = float(rng.choice([0.0, 0.0, 0.05, 0.5, 1.0]))
    valid = rng.random(n) >= share if share > 0 else None
    col = ("f64", v.astype(np.int64).view(np.float64) if rng.random() < 0.5 else v.astype(np.float64), valid) if is_float else i64(v, valid)
    k = int(rng.choice([0, 1, 10, 100, int(rng.integers(0, n + 2)), int(rng.integers(0, n // 2 + 1))]))
    return col, k, int(rng.integers(0, 4)), int(rng.choice([0, 0, 1, 63, 65]))


def test_random_cases_with_the_select_forced(ctx):
    rng = np.random.default_rng(22)
    selected = 0
    for case in range(100):
        col, k, flags, offset = random_case(rng)
        ctx.set_option("top_k_refine_divisor", int(rng.choice([0, 0, 1, 4, HUGE])))
        _, s = check(ctx, col, k, flags, offset, what=f"case {case} {col[0]}")
        selected += s.selected and s.passes > 0
    assert selected >= 30


def test_large_case_twice(ctx):
    ctx.set_option("top_k_select_from_rows", 0)
    rng = np.random.default_rng(23)
    n = 1 << 24
    col = i64(random_i64(rng, n), rng.random(n) >= 0.01)
    dev = upload(ctx, col)
    want = T.top_k_indices(col, 1, 1000)
    s = T.select(col, 1, 1000, *settings(ctx))
    runs = [indices_of(ctx.top_k_indices(dev, 1000, flags=1), 1000) for _ in range(2)]
    assert_path(ctx, s, n)
    assert s.selected and np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], want)


def test_kernel_name_and_timer(ctx):
    rng = np.random.default_rng(24)
    dev = upload(ctx, i64(random_i64(rng, 4 * TILE)))
    ctx.set_option("profile_kernels", 1)
    try:
        ctx.kernel_stats(reset=True)
        ctx.top_k_indices(dev, 10)
        assert ctx.last_kernel() == "topk_collect" and ctx.get_option("top_k_last_passes") >= 1
        ms, launches = ctx.kernel_stats(reset=True)
        assert ms > 0 and launches >= 7
    finally:
        ctx.set_option("profile_kernels", 0)
