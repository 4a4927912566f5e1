"""GPU suite: rv_hash_aggregate / rv_group_ids against tests/group_agg_model.py, cell by cell -- valid flags, the bits of valid cells,
0 under nulls, null_count, bitmap attached or not, first_row, gids.  Integer results and MIN / MAX are compared exactly; a Float64 SUM
bit for bit where every partial sum is representable and by the derived gamma bound otherwise (never by a measured tolerance)."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import group_agg_model as M
from helpers import CSRC, const
from rivulus_amd import capi
from rivulus_amd.capi import RV_FLOAT64, RV_INT64, RV_NULL, Column, RvError

pytestmark = pytest.mark.gpu

RV_ERR_INVALID_ARG, RV_ERR_LENGTH_MISMATCH, RV_ERR_TYPE_MISMATCH, RV_ERR_UNSUPPORTED = 1, 2, 3, 5
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
LDS_MOST = const("kGroupAggLdsGroupsMost")
WAVE_LIST = const("kGroupAggWaveListMost")
with open(os.path.join(CSRC, "group_agg_kernel.hpp")) as _f:
    _src = _f.read()
TILE = int(re.search(r"kGroupAggThreads = (\d+)", _src).group(1)) * int(re.search(r"kGroupAggRowsPerThread = (\d+)", _src).group(1))
DTYPE = {"i64": RV_INT64, "f64": RV_FLOAT64}
GARBAGE = np.array([np.nan, np.inf, -np.inf, 1e300])  # what lies under null Float64 cells, in rotation
ALL_OPS = [("count_rows", None), ("count", 0), ("sum", 0), ("min", 0), ("max", 0), ("count", 1), ("sum", 1), ("min", 1), ("max", 1)]


# ---- building inputs ----------------------------------------------------------------------------------------------------------------
def keys_of(rng, n, groups, null_share=0.0, spread=True):
    """n Int64 keys over `groups` distinct values (every value present when n >= groups), null_share of them null."""
    pool = rng.permutation(groups).astype(np.int64)
    if spread:
        pool = pool * 0x1E3779B97F4A7C15 % (1 << 62) - (1 << 61)  # spread over the 64 bits, both signs
    picks = np.concatenate([np.arange(min(n, groups)), rng.integers(0, groups, max(0, n - groups))])
    rng.shuffle(picks)
    valid = None
    if null_share > 0 and n:
        valid = rng.random(n) >= null_share
    return pool[picks], valid


def i64_col(rng, n, null_share=0.2, lo=-1000, hi=1000):
    return "i64", rng.integers(lo, hi, n, dtype=np.int64), (rng.random(n) >= null_share if null_share > 0 else None)


def f64_col(rng, n, null_share=0.2, exact=True):
    """Float64 cells k * 2^-10, |k| < 2^20 (every partial sum of up to 2^32 of them is representable), garbage under the nulls."""
    values = np.ldexp(rng.integers(-(1 << 20) + 1, 1 << 20, n).astype(np.float64), -10)
    if not exact:
        values = values * rng.choice(np.array([1.0, 1e16, 1e-7, -3.3]), n)
    valid = None
    if null_share > 0:
        valid = rng.random(n) >= null_share
        nulls = np.flatnonzero(~valid)
        values[nulls] = GARBAGE[np.arange(len(nulls)) % len(GARBAGE)]
    return "f64", values, valid


def upload(ctx, col, offset=0):
    """A device column of (dtype, values, valid); offset > 0: a slice at that element offset of a longer upload whose other cells are
    valid garbage."""
    dtype, values, valid = col[:3]
    n = len(values) if values is not None else 0
    if dtype == "null":
        return ctx.upload(Column.nulls(col[3]))
    if dtype == "str":
        cells = [None if valid is not None and not valid[i] else values[i] for i in range(n)]
        pad = ["pad"] * offset
        dev = ctx.upload(Column.from_strings(pad + cells + pad[:3]))
        return dev.slice(offset, n) if offset else dev
    if offset:
        fill = np.full(offset, 77, values.dtype) if values.dtype != np.bool_ else np.ones(offset, bool)
        values = np.concatenate([fill, values, fill[:3]])
        valid = np.concatenate([np.ones(offset, bool), np.ones(n, bool) if valid is None else valid, np.ones(min(3, offset), bool)])
    dev = ctx.upload(Column.from_numpy(values, valid))
    return dev.slice(offset, n) if offset else dev


def model_col(col):
    dtype, values, valid = col[:3]
    return (dtype if dtype in ("i64", "f64") else "other"), (values if dtype in ("i64", "f64") else None), valid


# ---- comparing ----------------------------------------------------------------------------------------------------------------------
def cells_of(dev, dtype_name):
    """(canonical cells or None, Column) of an output; checks what every output promises about itself."""
    info = dev.info()
    assert info.dtype == DTYPE[dtype_name] and info.offset == 0
    col = dev.download()
    bits = col.logical_values().view(np.uint64)
    valid = col.logical_valid()
    nulls = 0 if valid is None else int((~valid).sum())
    assert info.null_count == nulls and dev.null_count() == nulls, "null_count is known"
    assert (col.validity is not None) == (nulls > 0), "a bitmap is attached iff some cell is null"
    if nulls:
        assert not bits[~valid].any(), "0 under nulls"
    cells = [None if valid is not None and not valid[i] else M.canonical(dtype_name, b) for i, b in enumerate(bits.tolist())]
    return cells, col


def rows_of(dev):
    """the Int64 values of a gids / first_row column: no nulls, no bitmap"""
    info = dev.info()
    assert info.dtype == RV_INT64 and info.offset == 0 and info.null_count == 0 and info.has_validity == 0
    return dev.download().logical_values()


def check(ctx, key, cols, specs, offset=0, exact_float=True, kernel=None, what=""):
    """One rv_hash_aggregate + rv_group_ids call against the model.  key: (values, valid) or ("null", n)."""
    if isinstance(key[0], str):
        n = key[1]
        kdev, mkey = ctx.upload(Column.nulls(n)), (np.zeros(n, np.int64), np.zeros(n, bool))
    else:
        kdev, mkey = upload(ctx, ("i64", key[0], key[1]), offset), key
    devs = [upload(ctx, c, offset) for c in cols]
    want = M.aggregate(mkey, [model_col(c) for c in cols], specs, exact_float=exact_float)
    outs, first, groups = ctx.hash_aggregate(kdev, devs, specs)
    name = ctx.last_kernel()
    G = want["groups"]
    assert groups == G, what
    assert np.array_equal(rows_of(first), want["first_row"]), f"{what}: first_row"
    # out[0]: the key cells
    kinfo = outs[0].info()
    if isinstance(key[0], str):
        assert kinfo.dtype == RV_NULL and kinfo.length == G
    else:
        kcells, _ = cells_of(outs[0], "i64")
        assert kcells == [int(v) if ok else None for v, ok in zip(want["key_values"], want["key_valid"])], f"{what}: key cells"
    for j, (dev, agg) in enumerate(zip(outs[1:], want["aggs"])):
        got, _ = cells_of(dev, agg[0])
        exp = M.agg_cells(agg)
        if agg[3] is None or exact_float:
            assert got == exp, f"{what}: aggregate {j} {specs[j]}"
            continue
        assert len(got) == len(exp)
        for g, (a, b, cells) in enumerate(zip(got, exp, agg[3])):  # a Float64 SUM whose order matters: the gamma bound per group
            if a == b:
                continue
            fa, fb = (float(np.array([x], np.uint64).view(np.float64)[0]) for x in (a, b))
            assert np.isfinite(fa) and np.isfinite(fb), f"{what}: aggregate {j} group {g}: {fa} != {fb}"
            assert abs(Fraction(fa) - Fraction(fb)) <= M.gamma_bound(cells), f"{what}: aggregate {j} group {g}: {fa} against fsum {fb}, n = {len(cells)}"
    # rv_group_ids: the same groups
    gids, first2, groups2 = ctx.group_ids(kdev)
    assert groups2 == G
    assert np.array_equal(rows_of(gids), want["gids"]), f"{what}: gids"
    assert np.array_equal(rows_of(first2), want["first_row"])
    if kernel is not None:
        assert name == kernel, what
    return outs, name


def two_cols(rng, n, nulls=0.2):
    return [i64_col(rng, n, nulls), f64_col(rng, n, nulls)]


# ---- row counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1])
def test_row_counts(gpu_ctx, n):
    rng = np.random.default_rng(n)
    key = keys_of(rng, n, max(1, n // 5), 0.1)
    check(gpu_ctx, key, two_cols(rng, n), ALL_OPS, what=f"n={n}")


def test_one_row_past_a_full_sweep_of_the_grid(gpu_ctx):
    cus = gpu_ctx.device_info()["compute_units"]
    n = cus * 8 * TILE + 1  # the accumulate grid is at most 8 workgroups per CU: the first workgroup takes a second tile
    rng = np.random.default_rng(5)
    key = keys_of(rng, n, 37, 0.01)
    check(gpu_ctx, key, two_cols(rng, n, 0.1), [("count_rows", None), ("sum", 0), ("min", 1), ("sum", 1), ("count", 1)], what="sweep")


# ---- group counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 2, 3])
def test_few_groups(gpu_ctx, groups):
    rng = np.random.default_rng(groups)
    n = 5000
    check(gpu_ctx, keys_of(rng, n, groups), two_cols(rng, n), ALL_OPS, kernel="group_accumulate<lds>+group_f64_sum", what=f"G={groups}")


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_either_side_of_the_lds_switch(gpu_ctx, delta):
    """kGroupAggLdsGroupsMost groups and fewer: LDS accumulators; one more: global atomics.  The results agree with the model on both."""
    groups = LDS_MOST + delta
    rng = np.random.default_rng(groups)
    n = 3 * groups + 17
    form = "lds" if delta <= 0 else "global"
    check(gpu_ctx, keys_of(rng, n, groups), two_cols(rng, n), ALL_OPS[:5], kernel=f"group_accumulate<{form}>", what=f"G={groups}")
    check(gpu_ctx, keys_of(rng, n, groups, 0.05), two_cols(rng, n), [("sum", 1)], kernel="group_f64_sum", what=f"G={groups} f64 only")
    check(gpu_ctx, keys_of(rng, n, groups), two_cols(rng, n), [("max", 0), ("sum", 1)], kernel=f"group_accumulate<{form}>+group_f64_sum")


def test_all_keys_distinct(gpu_ctx):
    rng = np.random.default_rng(9)
    n = LDS_MOST + 3000  # more groups than the LDS form takes
    outs, _ = check(gpu_ctx, keys_of(rng, n, n), two_cols(rng, n), ALL_OPS, kernel="group_accumulate<global>+group_f64_sum", what="G=N")
    assert outs[1].length == n


def test_sorted_and_clustered_keys(gpu_ctx):
    """Runs of equal keys inside a wave take the segmented scan: one atomic per run."""
    rng = np.random.default_rng(10)
    n = 20_000
    for groups in (7, 3000):
        key = np.sort(keys_of(rng, n, groups, spread=False)[0])
        valid = np.ones(n, bool)
        valid[100:180] = False  # a run of null keys across a wave boundary
        check(gpu_ctx, (key, valid), two_cols(rng, n), ALL_OPS, what=f"sorted G={groups}")


# ---- key values ---------------------------------------------------------------------------------------------------------------------
def test_extreme_key_values(gpu_ctx):
    rng = np.random.default_rng(11)
    pool = np.array([I64_MIN, I64_MAX, 0, -1, 1, I64_MIN + 1, I64_MAX - 1], np.int64)
    n = 700
    key = pool[rng.integers(0, len(pool), n)]
    valid = rng.random(n) >= 0.1
    check(gpu_ctx, (key, valid), two_cols(rng, n), ALL_OPS, what="extreme keys")


def test_colliding_hash_bits(gpu_ctx):
    """Option agg_hash_bits = 2: four chain starts for 300 groups at N = 4097 -- chains of hundreds of slots, every hit confirmed by the key."""
    rng = np.random.default_rng(12)
    n = 4097
    key = keys_of(rng, n, 300, 0.05)
    cols = two_cols(rng, n)
    try:
        gpu_ctx.set_option("agg_hash_bits", 2)
        assert gpu_ctx.get_option("agg_hash_bits") == 2
        check(gpu_ctx, key, cols, ALL_OPS, what="agg_hash_bits=2")
    finally:
        gpu_ctx.set_option("agg_hash_bits", 0)
    check(gpu_ctx, key, cols, ALL_OPS, what="agg_hash_bits=0")


@pytest.mark.parametrize("where", ["first", "last", "absent", "only"])
def test_null_group_position(gpu_ctx, where):
    rng = np.random.default_rng(13)
    n = 1000
    key, _ = keys_of(rng, n, 40)
    valid = np.ones(n, bool)
    if where == "first":
        valid[[0, 5, 500]] = False
    elif where == "last":
        valid[n - 1] = False
    elif where == "only":
        valid[:] = False
    outs, _ = check(gpu_ctx, (key, None if where == "absent" else valid), two_cols(rng, n), ALL_OPS, what=where)
    kcol = outs[0].download()
    if where == "first":
        assert not kcol.logical_valid()[0]
    elif where == "last":
        assert not kcol.logical_valid()[-1] and kcol.logical_valid()[:-1].all()
    elif where == "only":
        assert kcol.length == 1
    else:
        assert kcol.validity is None


def test_null_typed_key_column(gpu_ctx):
    rng = np.random.default_rng(14)
    check(gpu_ctx, ("null", 300), two_cols(rng, 300), ALL_OPS, what="RV_NULL key")
    check(gpu_ctx, ("null", 0), two_cols(rng, 0), ALL_OPS, what="RV_NULL key, no rows")


@pytest.mark.parametrize("offset", [1, 63, 65])
def test_slices(gpu_ctx, offset):
    """Key and value slices at element offsets 1, 63 and 65 of a longer upload: validity and values are read at the offset."""
    rng = np.random.default_rng(offset)
    n = 1500
    check(gpu_ctx, keys_of(rng, n, 90, 0.1), two_cols(rng, n, 0.3), ALL_OPS, offset=offset, what=f"offset {offset}")


# ---- ops ----------------------------------------------------------------------------------------------------------------------------
def test_int64_sum_wraps(gpu_ctx):
    rng = np.random.default_rng(15)
    n = 3000
    vals = rng.integers(I64_MAX - 10, I64_MAX, n, dtype=np.int64)
    vals[::3] = I64_MIN
    check(gpu_ctx, keys_of(rng, n, 5), [("i64", vals, None), f64_col(rng, n)], [("sum", 0), ("min", 0), ("max", 0)], what="wrap")


def test_all_null_groups(gpu_ctx):
    """Groups without a non-null cell: MIN / MAX null (bitmap attached, 0 under it), SUM 0 / +0.0, COUNT 0."""
    rng = np.random.default_rng(16)
    n = 2000
    key, _ = keys_of(rng, n, 10, spread=False)
    cols = two_cols(rng, n, 0.1)
    dead = key % 3 == 0
    cols = [(c[0], c[1], c[2] & ~dead) for c in cols]
    cols[1][1][dead] = GARBAGE[np.arange(dead.sum()) % 4]
    outs, _ = check(gpu_ctx, (key, None), cols, ALL_OPS, what="all-null groups")
    assert outs[4].null_count() == 4 and outs[8].null_count() == 4  # keys 0, 3, 6, 9
    # ... and no group is all null: no bitmap at all
    outs, _ = check(gpu_ctx, (key, None), two_cols(rng, n, 0.1), ALL_OPS, what="no all-null group")
    assert outs[4].info().has_validity == 0


def test_float_specials(gpu_ctx):
    """NaN wins MIN and MAX, -0.0 < +0.0, +-inf order as values; NaN / inf under null cells never show."""
    key = np.array([1, 1, 2, 2, 3, 3, 4, 4, 5, 6, 6, 7, 7, 7], np.int64)
    vals = np.array([-0.0, 0.0, np.nan, 1.0, np.inf, -np.inf, np.nan, np.inf, -0.0, np.inf, 5.0, -np.inf, -1.0, 0.0])
    valid = np.array([1, 1, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0], bool)
    neg_nan = np.array([0xFFF8000000000001], np.uint64).view(np.float64)[0]
    vals2 = vals.copy()
    vals2[2] = neg_nan  # a NaN with the sign bit set and a payload
    for v in (vals, vals2):
        outs, _ = check(gpu_ctx, (key, None), [("f64", v, valid)], [("min", 0), ("max", 0), ("sum", 0), ("count", 0)], exact_float=False,
                        what="float specials")
    mn = outs[1].download()
    assert np.signbit(mn.logical_values()[0]) and mn.logical_values()[0] == 0.0  # MIN(-0.0, +0.0) is -0.0
    assert not np.signbit(outs[2].download().logical_values()[0])                 # MAX is +0.0
    assert not mn.logical_valid()[3]                                              # the group whose cells are all null (garbage NaN, inf)


def test_count_over_string_boolean_and_null_columns(gpu_ctx):
    rng = np.random.default_rng(17)
    n = 900
    strings = ("str", [f"s{i % 13}" if i % 7 else "" for i in range(n)], rng.random(n) >= 0.3)
    bools = ("bool", rng.random(n) < 0.5, rng.random(n) >= 0.4)
    plain = ("bool", rng.random(n) < 0.5, None)
    nulls = ("null", None, np.zeros(n, bool), n)
    for offset in (0, 3):
        check(gpu_ctx, keys_of(rng, n, 20, 0.1), [strings, bools, plain], [("count", 0), ("count", 1), ("count", 2), ("count_rows", None)], offset=offset)
    check(gpu_ctx, keys_of(rng, n, 20, 0.1), [strings, nulls], [("count", 1), ("count", 0)])


def test_many_aggregates_in_one_call(gpu_ctx):
    """More accumulators than one launch takes (several launches), the same column several times, nine MIN / MAX outputs (two read-backs)."""
    rng = np.random.default_rng(18)
    n = 4000
    cols = [i64_col(rng, n), f64_col(rng, n), i64_col(rng, n, 0.9), f64_col(rng, n, 0.0)]
    specs = [(op, c) for c in range(4) for op in ("min", "max", "sum", "count")] + [("count_rows", None), ("min", 0), ("sum", 1), ("sum", 0)]
    check(gpu_ctx, keys_of(rng, n, 50, 0.05), cols, specs, what="20 aggregates")


# ---- Float64 SUM --------------------------------------------------------------------------------------------------------------------
def test_float_sum_bit_exact_by_group_size(gpu_ctx):
    """Cells k * 2^s: every partial sum of every order is representable, so the sum has ONE right bit pattern.  Group sizes round a lane,
    a wave, one past a wave's list (the workgroup form) and one past a whole stride of the workgroup."""
    sizes = [1, 2, 63, 64, 65, WAVE_LIST - 1, WAVE_LIST, WAVE_LIST + 1, 5 * 256 + 1, 3 * WAVE_LIST + 5]
    rng = np.random.default_rng(19)
    key = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    for scale in (-1074, -10, 960):
        for interleave in (False, True):
            k = rng.permutation(key) if interleave else key
            n = len(k)
            values = np.ldexp(rng.integers(-(1 << 20) + 1, 1 << 20, n).astype(np.float64), scale)
            valid = rng.random(n) >= 0.15
            values[~valid] = GARBAGE[np.arange((~valid).sum()) % 4]
            plain = np.where(valid, values, np.ldexp(1.0, scale))  # the same cells without a bitmap
            check(gpu_ctx, (k, None), [("f64", values, valid), ("f64", plain, None)], [("sum", 0), ("sum", 1), ("count", 0)],
                  kernel="group_accumulate<lds>+group_f64_sum", what=f"scale {scale} interleave {interleave}")


def test_float_sum_gamma_bound_on_mixed_signs(gpu_ctx):
    """+-1e16 next to 1.0: the order matters; every order is within gamma_{n-1} x sum|x| of the exact sum, per group."""
    rng = np.random.default_rng(20)
    n = 6000
    values = rng.choice(np.array([1e16, -1e16, 1.0, 1.0, 3.5, -2.25e-3]), n)
    valid = rng.random(n) >= 0.1
    for groups in (1, 4, 700, 2000):
        check(gpu_ctx, keys_of(rng, n, groups), [("f64", values, valid)], [("sum", 0), ("count", 0)], exact_float=False, what=f"gamma G={groups}")


def test_the_same_call_three_times_gives_the_same_bits(gpu_ctx):
    rng = np.random.default_rng(21)
    n = 50_000
    for groups in (3, 5000):
        kdev = upload(gpu_ctx, ("i64",) + keys_of(rng, n, groups, 0.05))
        devs = [upload(gpu_ctx, i64_col(rng, n)), upload(gpu_ctx, f64_col(rng, n, 0.2, exact=False))]
        runs = []
        for _ in range(3):
            outs, first, g = gpu_ctx.hash_aggregate(kdev, devs, ALL_OPS)
            cols = [o.download() for o in outs + [first]]
            runs.append([(c.values.tobytes(), None if c.validity is None else c.validity.tobytes()) for c in cols] + [g])
        assert runs[0] == runs[1] == runs[2]


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def _status(fn):
    with pytest.raises(RvError) as e:
        fn()
    return e.value


def test_errors_leave_the_context_usable(gpu_ctx):
    rng = np.random.default_rng(22)
    n = 100
    key = keys_of(rng, n, 7, 0.1)
    cols = two_cols(rng, n)
    kdev, devs = upload(gpu_ctx, ("i64",) + key), [upload(gpu_ctx, c) for c in cols]
    ok = lambda: check(gpu_ctx, key, cols, ALL_OPS, what="after an error")  # noqa: E731
    lib, C = capi.load(), capi.C
    out, groups = (C.c_void_p * 4)(), C.c_uint64()
    spec = (capi.RvAggSpec * 2)()
    spec[0].op, spec[0].col = capi.RV_AGG_SUM, 0
    vals = capi._handles(devs)
    call = lambda ctx=gpu_ctx.handle, k=kdev.handle, v=vals, nv=2, s=spec, ns=1, o=out: lib.rv_hash_aggregate(ctx, k, v, nv, s, ns, o, None, C.byref(groups))  # noqa: E731
    assert call() == 0 and groups.value == len(set(key[0][key[1]].tolist())) + int(not key[1].all())
    for i in range(2):
        lib.rv_free(gpu_ctx.handle, C.c_void_p(out[i]))
    for bad in (dict(ctx=None), dict(k=None), dict(v=None), dict(s=None), dict(o=None), dict(ns=0)):
        assert call(**bad) == RV_ERR_INVALID_ARG, bad
        ok()
    spec[0].col = 2
    assert call() == RV_ERR_INVALID_ARG  # col out of range
    spec[0].op, spec[0].col = 5, 0
    assert call() == RV_ERR_INVALID_ARG  # unknown op
    spec[0].op, spec[0].col = capi.RV_AGG_COUNT_ROWS, 99
    assert call() == 0                   # COUNT_ROWS ignores col
    for i in range(2):
        lib.rv_free(gpu_ctx.handle, C.c_void_p(out[i]))
    ok()
    gids, first = C.c_void_p(), C.c_void_p()
    assert lib.rv_group_ids(gpu_ctx.handle, None, C.byref(gids), C.byref(first), None) == RV_ERR_INVALID_ARG
    assert lib.rv_group_ids(gpu_ctx.handle, kdev.handle, None, C.byref(first), None) == RV_ERR_INVALID_ARG
    # lengths and dtypes
    short = upload(gpu_ctx, i64_col(rng, n - 1))
    assert _status(lambda: gpu_ctx.hash_aggregate(kdev, [short], [("sum", 0)])).status == RV_ERR_LENGTH_MISMATCH
    ok()
    strs = gpu_ctx.upload(Column.from_strings(["a"] * n))
    bools = gpu_ctx.upload(Column.from_numpy(np.ones(n, bool)))
    floats = devs[1]
    for op in ("sum", "min", "max"):
        for col in (strs, bools, gpu_ctx.upload(Column.nulls(n))):
            assert _status(lambda: gpu_ctx.hash_aggregate(kdev, [col], [(op, 0)])).status == RV_ERR_TYPE_MISMATCH
    ok()
    for bad_key in (floats, bools, strs):
        assert _status(lambda: gpu_ctx.hash_aggregate(bad_key, [devs[0]], [("sum", 0)])).status == RV_ERR_UNSUPPORTED
        assert _status(lambda: gpu_ctx.group_ids(bad_key)).status == RV_ERR_UNSUPPORTED
    ok()


def test_keys_of_two_to_the_32_rows_are_refused(gpu_ctx):
    """The 32-bit row ids inside: a key of 2^32 rows is RV_ERR_UNSUPPORTED before anything is read (an RV_NULL column has no buffers)."""
    huge = gpu_ctx.upload(Column.nulls(1 << 32))
    e = _status(lambda: gpu_ctx.hash_aggregate(huge, [], [("count_rows", None)]))
    assert e.status == RV_ERR_UNSUPPORTED and "2^32" in str(e)
    assert _status(lambda: gpu_ctx.group_ids(huge)).status == RV_ERR_UNSUPPORTED
    rng = np.random.default_rng(23)
    check(gpu_ctx, keys_of(rng, 50, 5), two_cols(rng, 50), ALL_OPS, what="after the refusal")


def test_agg_max_groups(gpu_ctx):
    key5 = (np.array([10, 20, 30, 40, 50, 10, 20, 30, 40, 50], np.int64), None)
    key4 = (np.array([10, 20, 30, 40, 40, 10, 20, 30, 40, 10], np.int64), None)
    key3n = (key4[0], np.array([1, 1, 1, 0, 0, 1, 1, 1, 0, 1], bool))  # 3 keys and the null group: 4 groups
    key4n = (key4[0], np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 0], bool))  # 4 keys and the null group: 5 groups
    rng = np.random.default_rng(24)
    cols = two_cols(rng, 10)
    big = keys_of(rng, 5000, 1000)  # rows > agg_max_groups: the insert counts its claims and stops
    try:
        gpu_ctx.set_option("agg_max_groups", 4)
        assert gpu_ctx.get_option("agg_max_groups") == 4
        for bad in (key5, key4n):
            kdev = upload(gpu_ctx, ("i64",) + bad)
            e = _status(lambda: gpu_ctx.hash_aggregate(kdev, [upload(gpu_ctx, cols[0])], [("sum", 0)]))
            assert e.status == RV_ERR_UNSUPPORTED and "5 distinct" in str(e) and "agg_max_groups = 4" in str(e)
            assert _status(lambda: gpu_ctx.group_ids(kdev)).status == RV_ERR_UNSUPPORTED
            check(gpu_ctx, key4, cols, ALL_OPS, what="4 keys at agg_max_groups = 4")
        check(gpu_ctx, key3n, cols, ALL_OPS, what="3 keys + null at agg_max_groups = 4")
        e = _status(lambda: gpu_ctx.hash_aggregate(upload(gpu_ctx, ("i64",) + big), [], [("count_rows", None)]))
        assert e.status == RV_ERR_UNSUPPORTED and "agg_max_groups = 4" in str(e)
        gpu_ctx.set_option("agg_max_groups", 1000)
        check(gpu_ctx, big, two_cols(rng, 5000), ALL_OPS, what="1000 keys at agg_max_groups = 1000, 5000 rows")
        gpu_ctx.set_option("agg_max_groups", 999)
        assert _status(lambda: gpu_ctx.group_ids(upload(gpu_ctx, ("i64",) + big))).status == RV_ERR_UNSUPPORTED
    finally:
        gpu_ctx.set_option("agg_max_groups", 0)
    check(gpu_ctx, key5, cols, ALL_OPS, what="default agg_max_groups")


# ---- randomised differential cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(100))
def test_random_case(gpu_ctx, seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([rng.integers(0, 300), rng.integers(300, 5000), rng.integers(5000, 20_001)]))
    groups = int(max(1, rng.choice([rng.integers(1, 8), rng.integers(1, 2 * LDS_MOST), max(1, n // 2), n + 1])))
    key = keys_of(rng, n, groups, float(rng.choice([0.0, 0.0, 0.01, 0.5])), spread=bool(rng.integers(0, 2)))
    if rng.integers(0, 4) == 0 and n:
        order = np.argsort(key[0], kind="stable")
        key = (key[0][order], None if key[1] is None else key[1][order])
    exact = bool(rng.integers(0, 2))
    cols = [i64_col(rng, n, float(rng.choice([0.0, 0.2, 0.95])), I64_MIN // 2 if seed % 5 == 0 else -1000, I64_MAX // 2 if seed % 5 == 0 else 1000),
            f64_col(rng, n, float(rng.choice([0.0, 0.2, 0.95])), exact=exact)]
    pool = ALL_OPS + [("sum", 1), ("min", 1)]
    specs = [pool[i] for i in rng.integers(0, len(pool), int(rng.integers(1, 8)))]
    offset = int(rng.choice([0, 0, 1, 63, 65]))
    print(f"seed {seed}: n={n} groups<={groups} specs={specs} offset={offset} exact={exact}")
    check(gpu_ctx, key, cols, specs, offset=offset, exact_float=exact, what=f"seed {seed}")


# ---- larger runs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [10, 1_000_000])
def test_two_to_the_24_rows(gpu_ctx, groups):
    rng = np.random.default_rng(groups)
    n = 1 << 24
    key = (rng.integers(0, groups, n, dtype=np.int64) * 7919 - 12345, None)
    cols = [("i64", rng.integers(-1000, 1000, n, dtype=np.int64), None), f64_col(rng, n, 0.0)]
    form = "lds" if groups <= LDS_MOST else "global"
    check(gpu_ctx, key, cols, [("sum", 0), ("count_rows", None), ("min", 1), ("sum", 1)], kernel=f"group_accumulate<{form}>+group_f64_sum", what=f"2^24 rows, {groups} groups")
