"""GPU suite: rv_hash_aggregate_keys / rv_group_ids_keys against tests/group_keys_model.py, cell by cell -- gids, first_row, the key
cells of every key column (valid flags and bits, NaN payloads canonicalised), every aggregate.  Everything is compared bit for bit; a
Float64 SUM the way tests/test_group_agg_gpu.py does it: cells whose partial sums are all representable, or the model's gamma bound."""
from fractions import Fraction

import numpy as np
import pytest

import group_agg_model as M
import group_keys_model as K
from helpers import const
from rivulus_amd import capi
from rivulus_amd.capi import RV_BOOLEAN, RV_FLOAT64, RV_INT64, RV_NULL, Column, RvError

pytestmark = pytest.mark.gpu

RV_ERR_INVALID_ARG, RV_ERR_LENGTH_MISMATCH, RV_ERR_UNSUPPORTED = 1, 2, 5
I64_MIN = -(1 << 63)
LDS_MOST = const("kGroupAggLdsGroupsMost")
RV_DTYPE = {"i64": RV_INT64, "f64": RV_FLOAT64, "bool": RV_BOOLEAN, "null": RV_NULL}
DTYPES = ["i64", "f64", "bool", "null"]
NANS = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FF80000DEADBEEF], np.uint64).view(np.float64)
F64_SPECIALS = np.concatenate([NANS[:3], np.array([0.0, -0.0, np.inf, -np.inf])])
I64_SPECIALS = np.array([I64_MIN, -1, 0, (1 << 63) - 1], np.int64)
SPECS = [("count_rows", None), ("sum", 0), ("min", 0), ("max", 1), ("sum", 1), ("count", 1)]
TUPLE_IDS = "group_ids<keys>"


# ---- building inputs ----------------------------------------------------------------------------------------------------------------
def key_col(rng, dtype, n, card, null_rate=0.0, specials=False):
    """One key column of n rows over about `card` distinct values; the cells under nulls hold values of the same pool."""
    if dtype == "null":
        return "null", None, n
    if dtype == "bool":
        values = rng.random(n) < 0.5
    elif dtype == "i64":
        pool = rng.integers(-(1 << 62), 1 << 62, max(1, card), dtype=np.int64)
        if specials:
            pool[:min(len(pool), 4)] = I64_SPECIALS[:min(len(pool), 4)]
        values = pool[rng.integers(0, len(pool), n)]
    else:
        pool = np.ldexp(rng.integers(-(1 << 30), 1 << 30, max(1, card)).astype(np.float64), -8)
        if specials:
            pool[:min(len(pool), 7)] = F64_SPECIALS[:min(len(pool), 7)]
        values = pool[rng.integers(0, len(pool), n)]
        if specials and n:  # NaNs of other payloads in the same column: one key
            at = rng.integers(0, n, max(1, n // 50))
            values[at] = NANS[rng.integers(0, len(NANS), len(at))]
    valid = None
    if null_rate >= 1.0:
        valid = np.zeros(n, bool)
    elif null_rate > 0:
        valid = rng.random(n) >= null_rate
    return dtype, values, valid


def value_cols(rng, n, nulls=0.2):
    """an Int64 column and a Float64 column of cells k * 2^-10 (every partial sum representable)"""
    f = np.ldexp(rng.integers(-(1 << 20) + 1, 1 << 20, n).astype(np.float64), -10)
    return [("i64", rng.integers(-1000, 1000, n, dtype=np.int64), rng.random(n) >= nulls if nulls else None),
            ("f64", f, rng.random(n) >= nulls if nulls else None)]


def upload(ctx, col, offset=0):
    """A device column of (dtype, values, valid); offset > 0: a slice at that element offset of a longer upload."""
    dtype, values, valid = col
    if dtype == "null":
        return ctx.upload(Column.nulls(valid))
    n = len(values)
    if offset:
        fill = np.ones(offset, bool) if values.dtype == np.bool_ else np.full(offset, 77, values.dtype)
        values = np.concatenate([fill, values, fill[:3]])
        if valid is not None:
            valid = np.concatenate([np.ones(offset, bool), valid, np.ones(min(3, offset), bool)])
    dev = ctx.upload(Column.from_numpy(values, valid))
    return dev.slice(offset, n) if offset else dev


# ---- comparing ----------------------------------------------------------------------------------------------------------------------
def rows_of(dev):
    info = dev.info()
    assert info.dtype == RV_INT64 and info.offset == 0 and info.null_count == 0 and info.has_validity == 0
    return dev.download().logical_values()


def key_cells_of(dev, dtype, groups):
    """the canonical cells of a key output (None: null); null_count is known"""
    info = dev.info()
    assert info.dtype == RV_DTYPE[dtype] and info.length == groups
    if dtype == "null":
        return [None] * groups
    col = dev.download()
    valid = col.logical_valid()
    nulls = 0 if valid is None else int((~valid).sum())
    assert info.null_count == nulls and dev.null_count() == nulls
    if dtype == "bool":
        cells = [int(b) for b in col.logical_values().tolist()]
    else:
        cells = [M.canonical(dtype, b) for b in col.logical_values().view(np.uint64).tolist()]
    return [None if valid is not None and not valid[g] else c for g, c in enumerate(cells)]


def agg_cells_of(dev, dtype):
    info = dev.info()
    assert info.dtype == RV_DTYPE[dtype] and info.offset == 0
    col = dev.download()
    bits, valid = col.logical_values().view(np.uint64), col.logical_valid()
    nulls = 0 if valid is None else int((~valid).sum())
    assert info.null_count == nulls and (col.validity is not None) == (nulls > 0)
    if nulls:
        assert not bits[~valid].any(), "0 under nulls"
    return [None if valid is not None and not valid[i] else M.canonical(dtype, b) for i, b in enumerate(bits.tolist())]


def check(ctx, keys, cols, specs, offsets=None, exact_float=True, kernel=None, ids_kernel=None, what=""):
    """One rv_hash_aggregate_keys + rv_group_ids_keys call against the model."""
    offsets = offsets or [0] * (len(keys) + len(cols))
    kdevs = [upload(ctx, k, o) for k, o in zip(keys, offsets)]
    devs = [upload(ctx, c, o) for c, o in zip(cols, offsets[len(keys):])]
    want = K.aggregate(keys, cols, specs, exact_float=exact_float)
    G = want["groups"]
    outs, first, groups = ctx.hash_aggregate_keys(kdevs, devs, specs)
    name = ctx.last_kernel()
    assert groups == G and len(outs) == len(keys) + len(specs), what
    assert np.array_equal(rows_of(first), want["first_row"]), f"{what}: first_row"
    for k, key in enumerate(keys):
        assert key_cells_of(outs[k], key[0], G) == K.canonical_key_cells(key[0], want["key_cells"][k]), f"{what}: cells of key column {k}"
    for j, (dev, agg) in enumerate(zip(outs[len(keys):], want["aggs"])):
        got, exp = agg_cells_of(dev, agg[0]), M.agg_cells(agg)
        if agg[3] is None or exact_float:
            assert got == exp, f"{what}: aggregate {j} {specs[j]}"
            continue
        assert len(got) == len(exp)
        for g, (a, b, cells) in enumerate(zip(got, exp, agg[3])):  # a Float64 SUM whose order matters: the gamma bound per group
            if a == b:
                continue
            fa, fb = (float(np.array([x], np.uint64).view(np.float64)[0]) for x in (a, b))
            assert np.isfinite(fa) and np.isfinite(fb), f"{what}: aggregate {j} group {g}: {fa} != {fb}"
            assert abs(Fraction(fa) - Fraction(fb)) <= M.gamma_bound(cells), f"{what}: aggregate {j} group {g}"
    gids, first2, groups2 = ctx.group_ids_keys(kdevs)
    ids_name = ctx.last_kernel()
    assert groups2 == G
    assert np.array_equal(rows_of(gids), want["gids"]), f"{what}: gids"
    assert np.array_equal(rows_of(first2), want["first_row"])
    if kernel is not None:
        assert name == kernel, what
    if ids_kernel is not None:
        assert ids_name == ids_kernel, what
    return outs, want


# ---- row counts at the wave, workgroup and accumulate-tile boundaries -----------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2049])
def test_boundary_row_counts(gpu_ctx, n):
    """Two keys whose equal tuples come in runs of five that cross rows 64, 256 and 2048, and -- inside such a run -- rows 63, 255 and
    2047 with the second key NULL over the same bits as their neighbours': tuples that differ only in one null flag at lanes 63 | 64."""
    i = np.arange(n, dtype=np.int64)
    a, b = (i + 3) // 5, ((i + 3) // 10) % 3
    valid = np.ones(n, bool)
    valid[np.array([r for r in (63, 255, 2047) if r < n], np.int64)] = False
    rng = np.random.default_rng(n)
    cols = value_cols(rng, n)
    check(gpu_ctx, [("i64", a, None), ("i64", b, valid)], cols, SPECS, ids_kernel=TUPLE_IDS if n else None, what=f"n={n}")
    # the null flag in the FIRST column, the other a Float64 key
    check(gpu_ctx, [("i64", a, valid), ("f64", b.astype(np.float64) - 1.0, None)], cols, SPECS, what=f"n={n} flag in column 0")


# ---- key counts and dtypes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", [1, 2, 3, 8])
def test_key_counts_every_dtype_in_every_position(gpu_ctx, nkeys):
    rng = np.random.default_rng(100 + nkeys)
    n = 700
    cols = value_cols(rng, n)
    for shift in range(4):
        dtypes = [DTYPES[(k + shift) % 4] for k in range(nkeys)]
        keys = [key_col(rng, d, n, 3, 0.1, specials=True) for d in dtypes]
        tuple_kernels = nkeys > 1 or dtypes[0] in ("f64", "bool")
        check(gpu_ctx, keys, cols, SPECS, ids_kernel=TUPLE_IDS if tuple_kernels else None, what=f"{dtypes}")


@pytest.mark.parametrize("dtype", ["f64", "bool"])
def test_single_float64_and_boolean_keys_run_the_tuple_kernels(gpu_ctx, dtype):
    rng = np.random.default_rng(7)
    n = 1000
    for nulls in (0.0, 0.2):
        outs, want = check(gpu_ctx, [key_col(rng, dtype, n, 40, nulls, specials=True)], value_cols(rng, n), SPECS, ids_kernel=TUPLE_IDS, what=f"{dtype} {nulls}")
        if dtype == "bool":
            assert want["groups"] == 2 + (nulls > 0)


def test_float_key_rules(gpu_ctx):
    """Every NaN one group whose key cell is the FIRST row's own NaN; -0.0 and +0.0 two groups; a null neither."""
    key = np.concatenate([NANS, np.array([0.0, -0.0, 0.0, -0.0, 1.0])])
    valid = np.ones(len(key), bool)
    valid[-1] = False
    cols = value_cols(np.random.default_rng(8), len(key), 0)
    outs, want = check(gpu_ctx, [("f64", key, valid)], cols, SPECS, ids_kernel=TUPLE_IDS, what="float rules")
    assert want["first_row"].tolist() == [0, 5, 6, 9]
    cells = outs[0].download().logical_values().view(np.uint64)
    assert int(cells[0]) == int(NANS.view(np.uint64)[0]), "the first row's own bits"
    assert int(cells[1]) == 0 and int(cells[2]) == 1 << 63
    # ... and with the rows the other way round the negative, payload-carrying NaN is the key cell
    outs, _ = check(gpu_ctx, [("f64", key[::-1].copy(), valid[::-1].copy())], cols, SPECS, what="float rules reversed")
    assert int(outs[0].download().logical_values().view(np.uint64)[3]) == int(NANS.view(np.uint64)[4])


def test_the_four_null_and_zero_tuples_and_the_order_of_the_columns(gpu_ctx):
    z = np.zeros(8, np.int64)
    va = np.array([0, 1, 1, 0, 1, 0, 0, 1], bool)
    vb = np.array([1, 0, 1, 0, 1, 0, 1, 0], bool)
    cols = value_cols(np.random.default_rng(9), 8, 0)
    _, want = check(gpu_ctx, [("i64", z, va), ("i64", z, vb)], cols, SPECS, ids_kernel=TUPLE_IDS, what="null/zero")
    assert want["groups"] == 4
    a = np.array([1, 2, 1, 2, 2, 1], np.int64)
    b = np.array([2, 1, 2, 1, 2, 1], np.int64)
    _, want = check(gpu_ctx, [("i64", a, None), ("i64", b, None)], value_cols(np.random.default_rng(9), 6, 0), SPECS, what="(1, 2) and (2, 1)")
    assert want["gids"].tolist() == [0, 1, 0, 1, 2, 3]


# ---- slices ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [(1, 7, 13), (7, 13, 1), (13, 1, 7)])
def test_slices_at_different_offsets_per_column(gpu_ctx, offsets):
    """Boolean bits and validity bits at offsets that are no multiple of 8, another one for every column of the call."""
    rng = np.random.default_rng(sum(o * 31 ** i for i, o in enumerate(offsets)))
    n = 1500
    keys = [key_col(rng, "bool", n, 2, 0.2), key_col(rng, "f64", n, 9, 0.2, specials=True), key_col(rng, "i64", n, 5, 0.2, specials=True)]
    check(gpu_ctx, keys, value_cols(rng, n, 0.3), SPECS, offsets=list(offsets) + [offsets[1], offsets[0]], ids_kernel=TUPLE_IDS, what=f"offsets {offsets}")
    check(gpu_ctx, keys[:1], value_cols(rng, n, 0.3), SPECS, offsets=[offsets[0], 0, offsets[2]], ids_kernel=TUPLE_IDS, what=f"bool key at {offsets[0]}")


# ---- collisions -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [4, 1])
def test_colliding_hash_bits(gpu_ctx, bits):
    """agg_hash_bits = 4 / 1: 16 / 2 chain starts and no tag bits for about 500 tuples -- long chains, equal tags with unequal tuples."""
    rng = np.random.default_rng(bits)
    n = 2000
    keys = [key_col(rng, "i64", n, 25, 0.05), key_col(rng, "f64", n, 20, 0.05, specials=True), key_col(rng, "bool", n, 2, 0.1)]
    cols = value_cols(rng, n)
    try:
        gpu_ctx.set_option("agg_hash_bits", bits)
        _, want = check(gpu_ctx, keys, cols, SPECS, ids_kernel=TUPLE_IDS, what=f"agg_hash_bits={bits}")
    finally:
        gpu_ctx.set_option("agg_hash_bits", 0)
    assert 300 <= want["groups"] <= 1200
    check(gpu_ctx, keys, cols, SPECS, what="agg_hash_bits=0")


# ---- equivalences with the single-key entry points ----------------------------------------------------------------------------------------
def _bytes_of(devs):
    cols = [d.download() for d in devs]
    return [(c.dtype, c.length, c.logical_values().tobytes(), None if c.validity is None else c.logical_valid().tobytes()) for c in cols]


def test_one_int64_key_gives_what_rv_hash_aggregate_gives(gpu_ctx):
    rng = np.random.default_rng(30)
    n = 3000
    key = key_col(rng, "i64", n, 70, 0.1, specials=True)
    kdev, devs = upload(gpu_ctx, key), [upload(gpu_ctx, c) for c in value_cols(rng, n)]
    outs, first, groups = gpu_ctx.hash_aggregate_keys([kdev], devs, SPECS)
    outs1, first1, groups1 = gpu_ctx.hash_aggregate(kdev, devs, SPECS)
    assert groups == groups1 and _bytes_of(outs + [first]) == _bytes_of(outs1 + [first1])
    gids, f, g = gpu_ctx.group_ids_keys([kdev])
    gids1, f1, g1 = gpu_ctx.group_ids(kdev)
    assert g == g1 and _bytes_of([gids, f]) == _bytes_of([gids1, f1])
    check(gpu_ctx, [key], value_cols(rng, n), SPECS, what="one Int64 key against the model")


def test_two_keys_below_two_to_the_31_give_what_the_packed_key_gives(gpu_ctx):
    rng = np.random.default_rng(31)
    n = 5000
    a = rng.integers(0, 1 << 31, 40, dtype=np.int64)[rng.integers(0, 40, n)]
    b = rng.integers(0, 1 << 31, 30, dtype=np.int64)[rng.integers(0, 30, n)]
    cols = value_cols(rng, n)
    devs = [upload(gpu_ctx, c) for c in cols]
    outs, first, groups = gpu_ctx.hash_aggregate_keys([upload(gpu_ctx, ("i64", a, None)), upload(gpu_ctx, ("i64", b, None))], devs, SPECS)
    assert gpu_ctx.get_option("agg_hash_bits") == 0
    packed = upload(gpu_ctx, ("i64", (a << 32) | b, None))
    outs1, first1, groups1 = gpu_ctx.hash_aggregate(packed, devs, SPECS)
    assert groups == groups1 and _bytes_of(outs[2:] + [first]) == _bytes_of(outs1[1:] + [first1])
    ka, kb = (o.download().logical_values() for o in outs[:2])
    assert np.array_equal((ka << 32) | kb, outs1[0].download().logical_values())
    gids, _, _ = gpu_ctx.group_ids_keys([upload(gpu_ctx, ("i64", a, None)), upload(gpu_ctx, ("i64", b, None))])
    assert gpu_ctx.last_kernel() == TUPLE_IDS
    gids1, _, _ = gpu_ctx.group_ids(packed)
    assert _bytes_of([gids]) == _bytes_of([gids1])


# ---- the global accumulate path behind tuple ids --------------------------------------------------------------------------------------------
def test_global_accumulate_behind_tuple_ids(gpu_ctx):
    rng = np.random.default_rng(40)
    n = 1 << 20
    a, b = rng.integers(0, 200, n, dtype=np.int64), rng.integers(0, 150, n, dtype=np.int64) - 75
    cols = [("i64", rng.integers(-1000, 1000, n, dtype=np.int64), None), ("f64", np.ldexp(rng.integers(-999, 999, n).astype(np.float64), -4), None)]
    _, want = check(gpu_ctx, [("i64", a, None), ("i64", b, rng.random(n) >= 0.01)], cols, [("sum", 0), ("count_rows", None), ("min", 1)],
                    kernel="group_accumulate<global>", ids_kernel=TUPLE_IDS, what="2^20 rows")
    assert want["groups"] > LDS_MOST


# ---- agg_max_groups -----------------------------------------------------------------------------------------------------------------------
def _status(fn):
    with pytest.raises(RvError) as e:
        fn()
    return e.value


def test_agg_max_groups(gpu_ctx):
    a = np.array([1, 1, 2, 2, 1, 1, 2, 2, 1, 3], np.int64)
    b5 = np.array([1, 2, 1, 2, 1, 2, 1, 2, 1, 1], np.int64)
    valid5 = np.ones(10, bool)
    valid4 = np.ones(10, bool)
    valid4[9] = False
    a4 = a.copy()
    a4[9] = 1
    b4 = b5.copy()  # row 9 is (1, 1) over these bits: with its second cell null the fifth tuple, without the first tuple again
    rng = np.random.default_rng(50)
    cols = value_cols(rng, 10)
    five = [("i64", a, None), ("i64", b5, valid5)]
    five_by_flag = [("i64", a4, None), ("i64", b4, valid4)]  # the fifth tuple differs from (1, 1) only in its null flag
    four = [("i64", a4, None), ("i64", b4, None)]
    big = [key_col(rng, "i64", 5000, 40), key_col(rng, "i64", 5000, 40)]
    try:
        gpu_ctx.set_option("agg_max_groups", 4)
        for bad in (five, five_by_flag):
            kdevs = [upload(gpu_ctx, k) for k in bad]
            e = _status(lambda: gpu_ctx.hash_aggregate_keys(kdevs, [upload(gpu_ctx, cols[0])], [("sum", 0)]))
            assert e.status == RV_ERR_UNSUPPORTED and "5 distinct" in str(e) and "agg_max_groups = 4" in str(e)
            assert _status(lambda: gpu_ctx.group_ids_keys(kdevs)).status == RV_ERR_UNSUPPORTED
            check(gpu_ctx, four, cols, SPECS, what="4 tuples at agg_max_groups = 4: the context is usable")
        kdevs = [upload(gpu_ctx, k) for k in big]  # rows > agg_max_groups: the insert counts its claims and stops
        e = _status(lambda: gpu_ctx.hash_aggregate_keys(kdevs, [], [("count_rows", None)]))
        assert e.status == RV_ERR_UNSUPPORTED and "agg_max_groups = 4" in str(e)
    finally:
        gpu_ctx.set_option("agg_max_groups", 0)
    check(gpu_ctx, five, cols, SPECS, what="default agg_max_groups")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(gpu_ctx):
    rng = np.random.default_rng(60)
    n = 100
    keys = [key_col(rng, "i64", n, 4, 0.1), key_col(rng, "bool", n, 2, 0.1)]
    cols = value_cols(rng, n)
    kdevs, devs = [upload(gpu_ctx, k) for k in keys], [upload(gpu_ctx, c) for c in cols]
    ok = lambda: check(gpu_ctx, keys, cols, SPECS, what="after a refusal")  # noqa: E731
    lib, C = capi.load(), capi.C
    out, first, gids, groups = (C.c_void_p * 8)(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    spec = (capi.RvAggSpec * 2)()
    spec[0].op, spec[0].col = capi.RV_AGG_SUM, 0
    karr, varr = capi._handles(kdevs), capi._handles(devs)
    call = lambda ctx=gpu_ctx.handle, k=karr, nk=2, v=varr, nv=2, s=spec, ns=1, o=out: lib.rv_hash_aggregate_keys(ctx, k, nk, v, nv, s, ns, o, None, C.byref(groups))  # noqa: E731
    assert call() == 0
    for i in range(3):
        lib.rv_free(gpu_ctx.handle, C.c_void_p(out[i]))
    hole = (C.c_void_p * 2)()
    hole[0] = kdevs[0].handle  # keys[1] is NULL
    for bad in (dict(ctx=None), dict(k=None), dict(v=None), dict(s=None), dict(o=None), dict(ns=0), dict(nk=0), dict(nk=9), dict(k=hole)):
        assert call(**bad) == RV_ERR_INVALID_ARG, bad
    ok()
    ids = lambda ctx=gpu_ctx.handle, k=karr, nk=2, g=C.byref(gids), f=C.byref(first): lib.rv_group_ids_keys(ctx, k, nk, g, f, None)  # noqa: E731
    for bad in (dict(ctx=None), dict(k=None), dict(g=None), dict(f=None), dict(nk=0), dict(nk=9), dict(k=hole)):
        assert ids(**bad) == RV_ERR_INVALID_ARG, bad
    assert gids.value is None and first.value is None, "nothing is created"
    nine = [kdevs[0]] * 9
    assert _status(lambda: gpu_ctx.hash_aggregate_keys(nine, devs, [("sum", 0)])).status == RV_ERR_INVALID_ARG
    assert _status(lambda: gpu_ctx.group_ids_keys(nine)).status == RV_ERR_INVALID_ARG
    gpu_ctx.group_ids_keys([kdevs[0]] * 8)  # eight are taken
    ok()
    # lengths
    short = upload(gpu_ctx, key_col(rng, "i64", n - 1, 4))
    assert _status(lambda: gpu_ctx.hash_aggregate_keys([kdevs[0], short], devs, [("sum", 0)])).status == RV_ERR_LENGTH_MISMATCH
    assert _status(lambda: gpu_ctx.group_ids_keys([short, kdevs[1]])).status == RV_ERR_LENGTH_MISMATCH
    assert _status(lambda: gpu_ctx.hash_aggregate_keys(kdevs, [short], [("sum", 0)])).status == RV_ERR_LENGTH_MISMATCH
    ok()
    # a String key names the dictionary
    strs = gpu_ctx.upload(Column.from_strings(["a"] * n))
    for fn in (lambda: gpu_ctx.hash_aggregate_keys([kdevs[0], strs], devs, [("sum", 0)]), lambda: gpu_ctx.group_ids_keys([strs])):
        e = _status(fn)
        assert e.status == RV_ERR_UNSUPPORTED and "rv_string_dict_build" in str(e)
    ok()


def test_keys_of_two_to_the_32_rows_are_refused(gpu_ctx):
    """An RV_NULL column has no buffers: 2^32 rows of it are refused before anything is read."""
    huge = gpu_ctx.upload(Column.nulls(1 << 32))
    e = _status(lambda: gpu_ctx.hash_aggregate_keys([huge, huge], [], [("count_rows", None)]))
    assert e.status == RV_ERR_UNSUPPORTED and "2^32" in str(e)
    assert _status(lambda: gpu_ctx.group_ids_keys([huge])).status == RV_ERR_UNSUPPORTED
    rng = np.random.default_rng(61)
    check(gpu_ctx, [key_col(rng, "f64", 50, 5), key_col(rng, "null", 50, 1)], value_cols(rng, 50), SPECS, what="after the refusal")


# ---- determinism ----------------------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bytes(gpu_ctx):
    rng = np.random.default_rng(70)
    n = 20_000
    kdevs = [upload(gpu_ctx, key_col(rng, "i64", n, 60, 0.05)), upload(gpu_ctx, key_col(rng, "f64", n, 50, 0.05, specials=True))]
    f = np.ldexp(rng.integers(-(1 << 20) + 1, 1 << 20, n).astype(np.float64), -10) * rng.choice(np.array([1.0, 1e16, 1e-7, -3.3]), n)
    devs = [upload(gpu_ctx, value_cols(rng, n)[0]), upload(gpu_ctx, ("f64", f, rng.random(n) >= 0.2))]
    runs = []
    for _ in range(2):
        outs, first, g = gpu_ctx.hash_aggregate_keys(kdevs, devs, SPECS)
        gids, _, _ = gpu_ctx.group_ids_keys(kdevs)
        runs.append(_bytes_of(outs + [first, gids]) + [g])
    assert runs[0] == runs[1]


# ---- randomised differential cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(200))
def test_random_case(gpu_ctx, seed):
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.choice([rng.integers(0, 130), rng.integers(130, 1000), rng.integers(1000, 4097)]))
    nkeys = int(rng.integers(1, 5))
    dtypes = [str(rng.choice(DTYPES, p=[0.4, 0.3, 0.2, 0.1])) for _ in range(nkeys)]
    card = int(rng.choice([1, 2, rng.integers(1, 20), max(1, n // 3), max(1, n)]))
    keys = [key_col(rng, d, n, card, float(rng.choice([0.0, 0.1, 1.0], p=[0.45, 0.45, 0.1])), specials=bool(rng.integers(0, 2))) for d in dtypes]
    if rng.integers(0, 4) == 0 and n and dtypes[0] in ("i64", "f64"):  # runs of equal tuples: the first key sorted by its bits
        order = np.argsort(keys[0][1].view(np.int64), kind="stable")
        keys = [k if k[0] == "null" else (k[0], k[1][order], None if k[2] is None else k[2][order]) for k in keys]
    exact = bool(rng.integers(0, 2))
    cols = value_cols(rng, n, float(rng.choice([0.0, 0.2, 0.95])))
    if not exact:
        cols[1] = ("f64", cols[1][1] * rng.choice(np.array([1.0, 1e16, 1e-7, -3.3]), n), cols[1][2])
    pool = SPECS + [("sum", 1), ("min", 1), ("max", 0), ("count", 0)]
    specs = [pool[i] for i in rng.integers(0, len(pool), int(rng.integers(1, 7)))]
    offsets = [int(rng.choice([0, 0, 1, 7, 13, 63, 65])) for _ in range(nkeys + 2)]
    print(f"seed {seed}: n={n} dtypes={dtypes} card={card} specs={specs} offsets={offsets} exact={exact}")
    check(gpu_ctx, keys, cols, specs, offsets=offsets, exact_float=exact, what=f"seed {seed}")
