"""GPU suite: rv_sort_indices / rv_sort against tests/sort_model.py.  The sort is stable, so the permutation is unique and EVERY comparison
here is exact equality with the model's -- no tolerance anywhere.  Row counts sit round one lane, one wave, one tile of the radix passes
(rvk::kSortTileRows), one past the 2048 tile counts a workgroup of the scan takes (eight tiles: the scan's second workgroup), and one past a
single sweep of the grid-strided map kernel (8 workgroups of 256 rows per CU: 2^19 rows on 256 CUs).  The scan's second ROUND of block sums
starts past 2^27 rows: that is the scan's own ground (strings, CSV), not re-tested here."""
import numpy as np
import pytest

import sort_model as M
from helpers import const
from rivulus_amd import capi
from rivulus_amd.capi import RV_INT64, Column, RvError

pytestmark = pytest.mark.gpu

RV_ERR_INVALID_ARG, RV_ERR_LENGTH_MISMATCH, RV_ERR_TYPE_MISMATCH, RV_ERR_OUT_OF_BOUNDS, RV_ERR_UNSUPPORTED = 1, 2, 3, 4, 5
TILE = 256 * const("kSortRowsPerLane")
ROW_COUNTS = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 8 * TILE + 1, (1 << 19) + 77]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ALL_FLAGS = [0, 1, 2, 3]


@pytest.fixture(scope="module")
def ctx():
    with capi.Context(0) as c:
        yield c


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


def indices_of(dev, n):
    """the Int64 values of a permutation column: n rows, no nulls, no bitmap"""
    info = dev.info()
    assert info.dtype == RV_INT64 and info.length == n and info.offset == 0 and info.null_count == 0 and info.has_validity == 0
    return dev.download().logical_values()


def check(ctx, col, flags=0, prior=None, offset=0, what=""):
    """One rv_sort_indices call against the model; returns the permutation."""
    n = len(col[1])
    want = M.sort_indices(col, flags, prior)
    pdev = None if prior is None else ctx.upload(Column.from_numpy(np.asarray(prior, np.int64)))
    got = indices_of(ctx.sort_indices(upload(ctx, col, offset), flags=flags, prior=pdev), n)
    assert np.array_equal(got, want), f"{what} flags {flags} offset {offset}: first difference at {np.flatnonzero(got != want)[:5]}"
    return got


def i64(values, valid=None):
    return "i64", np.asarray(values, np.int64), valid


def f64_bits(bits, valid=None):
    return "f64", np.asarray(bits, np.uint64).view(np.float64), valid


def random_i64(rng, n):
    return rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)


# ---- row counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts(ctx, n):
    rng = np.random.default_rng(n)
    check(ctx, i64(random_i64(rng, n)), what="random 64-bit")
    check(ctx, i64(rng.integers(0, 7, n), rng.random(n) >= 0.3 if n else None), flags=3, what="few values, nulls")
    got = ctx.sort_indices(upload(ctx, i64(rng.integers(0, 7, n))))
    assert got.info().length == n


# ---- keys ---------------------------------------------------------------------------------------------------------------------------
def test_all_equal_is_the_identity_and_runs_no_pass(ctx):
    n = 2 * TILE + 5
    for flags in ALL_FLAGS:
        got = check(ctx, i64(np.full(n, -12345)), flags)
        assert np.array_equal(got, np.arange(n)) and ctx.get_option("sort_last_passes") == 0
        assert ctx.last_kernel() == "sort_widen"


def test_two_distinct_values(ctx):
    rng = np.random.default_rng(2)
    v = np.where(rng.random(3 * TILE + 7) < 0.5, -(1 << 40), 1 << 50)
    for flags in ALL_FLAGS:
        check(ctx, i64(v), flags)


@pytest.mark.parametrize("shift", [0, 56])
def test_one_differing_byte_is_one_pass(ctx, shift):
    rng = np.random.default_rng(shift)
    base = np.uint64(0x0123456789ABCDEF & ~(0xFF << shift))
    v = (base | (rng.integers(0, 256, 2 * TILE + 3, dtype=np.uint64) << np.uint64(shift))).view(np.int64)
    check(ctx, i64(v))
    assert ctx.get_option("sort_last_passes") == 1
    check(ctx, i64(v), flags=1)
    assert ctx.get_option("sort_last_passes") == 1


def test_values_below_2_16_take_two_passes(ctx):
    rng = np.random.default_rng(16)
    check(ctx, i64(rng.integers(0, 1 << 16, 5 * TILE + 11)))
    assert ctx.get_option("sort_last_passes") <= 2
    assert ctx.last_kernel() == "sort_scatter"


def test_random_64_bit_takes_eight(ctx):
    rng = np.random.default_rng(64)
    check(ctx, i64(random_i64(rng, 4 * TILE + 1)))
    assert ctx.get_option("sort_last_passes") == 8


def test_int_extremes(ctx):
    rng = np.random.default_rng(3)
    v = rng.choice(np.array([I64_MIN, I64_MAX, -1, 0, 1, I64_MIN + 1, I64_MAX - 1], np.int64), 2 * TILE + 9)
    for flags in ALL_FLAGS:
        check(ctx, i64(v, rng.random(len(v)) >= 0.1), flags)


def test_sorted_and_reverse_sorted(ctx):
    n = 3 * TILE + 17
    asc = np.arange(n, dtype=np.int64) * 1000003 - 10 ** 9
    for v in (asc, asc[::-1].copy()):
        for flags in (0, 1):
            check(ctx, i64(v), flags)


# ---- Float64 ------------------------------------------------------------------------------------------------------------------------
FLOAT_SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072009e-308, 1.0, -1.0,
                           1.7976931348623157e308, -1.7976931348623157e308]).view(np.uint64)
NANS = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF,
                 0x7FF8000000001234], np.uint64)


def test_float_specials(ctx):
    rng = np.random.default_rng(4)
    bits = rng.choice(FLOAT_SPECIALS, 2 * TILE + 3)
    for flags in ALL_FLAGS:
        check(ctx, f64_bits(bits, rng.random(len(bits)) >= 0.2), flags)


def test_nans_end_up_last_in_row_order(ctx):
    rng = np.random.default_rng(5)
    n = 2 * TILE + 31
    bits = rng.standard_normal(n).view(np.uint64).copy()
    where = np.flatnonzero(rng.random(n) < 0.3)
    bits[where] = NANS[np.arange(len(where)) % len(NANS)]
    got = check(ctx, f64_bits(bits))
    assert np.array_equal(got[n - len(where):], where), "the NaNs, of both signs and every payload, last and in row order"
    got = check(ctx, f64_bits(bits), flags=1)
    assert np.array_equal(got[:len(where)], where), "descending: first, still in row order"


def test_float_order_agrees_on_bits_through_a_take(ctx):
    rng = np.random.default_rng(6)
    n = 3 * TILE + 1
    bits = np.concatenate([rng.choice(FLOAT_SPECIALS, n // 2), (rng.standard_normal(n - n // 2) * 1e-300).view(np.uint64)])
    rng.shuffle(bits)
    col = f64_bits(bits)
    dev = upload(ctx, col)
    taken = ctx.take_device([dev], ctx.sort_indices(dev))[0].download().logical_values().view(np.uint64)
    assert np.array_equal(taken, bits[M.sort_indices(col)])
    keys = M.order_key(taken, True)
    assert np.all(keys[:-1] <= keys[1:])


# ---- nulls --------------------------------------------------------------------------------------------------------------------------
def null_patterns(rng, n):
    head, tail = np.ones(n, bool), np.ones(n, bool)
    head[:n // 3] = False
    tail[n - n // 3:] = False
    return {"absent": None, "first rows": head, "last rows": tail, "every row": np.zeros(n, bool), "scattered": rng.random(n) >= 0.4}


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_nulls_under_every_flag_combination(ctx, flags):
    rng = np.random.default_rng(7)
    n = 2 * TILE + 77
    v = rng.integers(-50, 50, n)
    for name, valid in null_patterns(rng, n).items():
        check(ctx, i64(v, valid), flags, what=name)
        check(ctx, ("f64", v.astype(np.float64) / 7, valid), flags, what=name)


def test_garbage_under_nulls_changes_nothing(ctx):
    rng = np.random.default_rng(8)
    n = 3 * TILE + 5
    valid = rng.random(n) >= 0.35
    v = rng.integers(-1000, 1000, n)
    for flags in ALL_FLAGS:
        perms = []
        for _ in range(2):
            garbage = np.where(valid, v, random_i64(rng, n))
            perms.append(check(ctx, i64(garbage, valid), flags))
        assert np.array_equal(perms[0], perms[1])
    fv = rng.standard_normal(n)
    perms = []
    for fill in (np.nan, -np.inf):
        perms.append(check(ctx, ("f64", np.where(valid, fv, fill), valid), 2))
    assert np.array_equal(perms[0], perms[1])


def test_null_column(ctx):
    assert np.array_equal(check(ctx, ("null", np.zeros(TILE + 3, np.int64), None), 3), np.arange(TILE + 3))
    prior = np.random.default_rng(9).permutation(TILE + 3)
    assert np.array_equal(check(ctx, ("null", np.zeros(TILE + 3, np.int64), None), 1, prior=prior), prior)


# ---- slices -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [1, 63, 65])
def test_slices_of_key_and_validity(ctx, offset):
    rng = np.random.default_rng(offset)
    n = 2 * TILE + 13
    for flags in ALL_FLAGS:
        check(ctx, i64(rng.integers(-300, 300, n), rng.random(n) >= 0.25), flags, offset=offset)
    check(ctx, ("f64", rng.standard_normal(n), rng.random(n) >= 0.25), 1, offset=offset)
    prior = rng.permutation(n)
    pdev = ctx.upload(Column.from_numpy(np.concatenate([np.full(offset, -5, np.int64), prior]))).slice(offset, n)
    col = i64(rng.integers(0, 9, n))
    got = indices_of(ctx.sort_indices(upload(ctx, col, offset), prior=pdev), n)
    assert np.array_equal(got, M.sort_indices(col, 0, prior)), "a sliced prior"


# ---- chaining -----------------------------------------------------------------------------------------------------------------------
def frame_columns(rng, n):
    return [i64(rng.integers(0, 4, n), rng.random(n) >= 0.1), ("f64", rng.integers(0, 5, n).astype(np.float64) - 2.0, rng.random(n) >= 0.1),
            i64(rng.integers(-3, 3, n))]


@pytest.mark.parametrize("keys", [[(0, 0), (1, 1)], [(2, 3), (0, 2), (1, 0)]], ids=["two keys", "three keys"])
def test_chained_keys_against_lexsort(ctx, keys):
    rng = np.random.default_rng(len(keys))
    n = 2 * TILE + 41
    cols = frame_columns(rng, n)
    devs = [upload(ctx, c) for c in cols]
    perm = None
    for c, flags in reversed(keys):
        perm = ctx.sort_indices(devs[c], flags=flags, prior=perm)
    got = indices_of(perm, n)
    assert np.array_equal(got, M.lexsort_frame(cols, keys)) and np.array_equal(got, M.sort_frame(cols, keys))


def test_prior_that_is_not_the_identity(ctx):
    rng = np.random.default_rng(10)
    n = 2 * TILE + 3
    for flags in ALL_FLAGS:
        check(ctx, i64(rng.integers(0, 20, n), rng.random(n) >= 0.2), flags, prior=rng.permutation(n))


def good_call(ctx):
    check(ctx, i64([3, 1, 2, 1]), 0)


def test_prior_errors_leave_the_context_usable(ctx):
    key = upload(ctx, i64(np.arange(100)))
    with pytest.raises(RvError) as e:
        ctx.sort_indices(key, prior=ctx.upload(Column.from_numpy(np.arange(99, dtype=np.int64))))
    assert e.value.status == RV_ERR_LENGTH_MISMATCH
    good_call(ctx)
    bad = np.arange(100, dtype=np.int64)
    bad[40], bad[70] = 100, -1
    with pytest.raises(RvError) as e:
        ctx.sort_indices(key, prior=ctx.upload(Column.from_numpy(bad)))
    assert e.value.status == RV_ERR_OUT_OF_BOUNDS and "Index 100 out of bounds for 100 rows" in e.value.message
    good_call(ctx)
    with pytest.raises(RvError) as e:
        ctx.sort_indices(key, prior=ctx.upload(Column.from_numpy(np.arange(100, dtype=np.float64))))
    assert e.value.status == RV_ERR_TYPE_MISMATCH
    with pytest.raises(RvError) as e:
        ctx.sort_indices(key, prior=ctx.upload(Column.from_numpy(np.arange(100, dtype=np.int64), np.arange(100) != 5)))
    assert e.value.status == RV_ERR_INVALID_ARG
    good_call(ctx)


def test_key_dtypes_and_flags_refused(ctx):
    for col in (Column.from_numpy(np.array([True, False])), Column.from_strings(["b", "a"])):
        with pytest.raises(RvError) as e:
            ctx.sort_indices(ctx.upload(col))
        assert e.value.status == RV_ERR_UNSUPPORTED
        good_call(ctx)
    with pytest.raises(RvError) as e:
        ctx.sort_indices(upload(ctx, i64([1, 2])), flags=4)
    assert e.value.status == RV_ERR_INVALID_ARG
    good_call(ctx)


# ---- rv_sort ------------------------------------------------------------------------------------------------------------------------
def test_sort_of_a_frame(ctx):
    rng = np.random.default_rng(11)
    n = TILE + 99
    cols = frame_columns(rng, n)
    flags_b = rng.random(n) < 0.5
    bvalid = rng.random(n) >= 0.2
    strings = [None if i % 7 == 3 else f"s{i % 13}" * (i % 3) for i in range(n)]
    host = [Column.from_numpy(c[1], c[2]) for c in cols] + [Column.from_numpy(flags_b, bvalid), Column.from_strings(strings)]
    devs = [ctx.upload(h) for h in host]
    keys = [(1, capi.RV_SORT_DESCENDING), (0, capi.RV_SORT_NULLS_LAST)]
    outs = ctx.sort(devs, keys)
    assert ctx.last_kernel().startswith("sort_")
    perm = M.sort_frame(cols, keys)
    expect = ctx.take(devs, perm)
    for j, (o, e) in enumerate(zip(outs, expect)):
        assert o.download().same_as(e.download()) is None, j
    assert outs[4].download().to_strings() == [strings[i] for i in perm]
    one = ctx.sort(devs, [2])  # a key by index alone: flags 0
    assert np.array_equal(one[2].download().logical_values(), np.sort(cols[2][1], kind="stable"))


def test_sort_errors_leave_the_context_usable(ctx):
    a, b = upload(ctx, i64([2, 1, 3])), upload(ctx, i64([1, 2, 3, 4]))
    s, t = ctx.upload(Column.from_strings(["x", "y", "z"])), ctx.upload(Column.from_numpy(np.array([True, False, True])))
    for cols, keys, status in [([a], [], RV_ERR_INVALID_ARG), ([a], [1], RV_ERR_INVALID_ARG), ([a], [(0, 4)], RV_ERR_INVALID_ARG),
                               ([a, b], [0], RV_ERR_LENGTH_MISMATCH), ([a, s], [1], RV_ERR_UNSUPPORTED), ([a, t], [(1, 1)], RV_ERR_UNSUPPORTED)]:
        with pytest.raises(RvError) as e:
            ctx.sort(cols, keys)
        assert e.value.status == status, (keys, e.value)
        out = ctx.sort([a, s], [0])
        assert out[0].download().logical_values().tolist() == [1, 2, 3] and out[1].download().to_strings() == ["y", "x", "z"]


# ---- engines, determinism -----------------------------------------------------------------------------------------------------------
def random_case(rng):
    n = int(rng.integers(0, 20001))
    card = int(rng.integers(1, max(2, n + 1)))
    is_float = rng.random() < 0.5
    pool = random_i64(rng, card) if rng.random() < 0.5 else rng.integers(0, max(1, card), card)
    v = pool[rng.integers(0, card, n)] if n else np.zeros(0, np.int64)
    share = float(rng.choice([0.0, 0.0, 0.05, 0.5, 1.0]))
    valid = rng.random(n) >= share if share > 0 else None
    col = ("f64", v.astype(np.int64).view(np.float64) if rng.random() < 0.5 else v.astype(np.float64), valid) if is_float else i64(v, valid)
    return col, int(rng.integers(0, 4)), int(rng.choice([0, 0, 1, 63, 65]))


def test_engines_agree_with_each_other_and_the_model(ctx):
    rng = np.random.default_rng(12)
    try:
        for k in range(100):
            col, flags, offset = random_case(rng)
            dev = upload(ctx, col, offset)
            want = M.sort_indices(col, flags)
            for engine in (0, 1):
                ctx.set_option("sort_engine", engine)
                got = indices_of(ctx.sort_indices(dev, flags=flags), len(col[1]))
                assert np.array_equal(got, want), (k, engine, col[0], len(col[1]), flags, offset)
    finally:
        ctx.set_option("sort_engine", 0)
    assert ctx.get_option("sort_engine") == 0


def test_three_runs_are_identical(ctx):
    rng = np.random.default_rng(13)
    n = 6 * TILE + 3
    dev = upload(ctx, i64(rng.integers(0, 50, n), rng.random(n) >= 0.1))
    runs = [indices_of(ctx.sort_indices(dev, flags=1), n) for _ in range(3)]
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


def test_kernel_name_and_timer(ctx):
    rng = np.random.default_rng(14)
    dev = upload(ctx, i64(random_i64(rng, 2 * TILE)))
    ctx.set_option("profile_kernels", 1)
    try:
        ctx.kernel_stats(reset=True)
        ctx.sort_indices(dev)
        assert ctx.last_kernel() == "sort_scatter"
        ms, launches = ctx.kernel_stats(reset=True)
        assert ms > 0 and launches >= 8
    finally:
        ctx.set_option("profile_kernels", 0)


# ---- large --------------------------------------------------------------------------------------------------------------------------
def test_large_random_int64(ctx):
    rng = np.random.default_rng(15)
    check(ctx, i64(random_i64(rng, 1 << 24)))


def test_large_float64_ten_values_with_nulls(ctx):
    rng = np.random.default_rng(16)
    n = 1 << 24
    check(ctx, ("f64", rng.integers(0, 10, n).astype(np.float64) * 0.5 - 2.0, rng.random(n) >= 0.05), flags=1)
