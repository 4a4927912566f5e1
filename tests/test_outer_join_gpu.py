"""GPU suite: the outer, semi and anti hash joins (rv_join_probe_kind / rv_hash_join_kind / rv_take_device_nullable) against the model
(tests/outer_join_model.py) and the hand-written cases of tests/golden/outer_join_cases.json, compared at AnyValue level as
test_join_gpu.py compares the inner join: the value where a cell is valid, null where not."""
import numpy as np
import pytest

from join_model import comparable
from outer_join_model import (FULL_OUTER, INNER, KIND_NAMES, KINDS, PROBE_ANTI, PROBE_OUTER, PROBE_SEMI, join_pairs, load_golden_cases,
                              materialize_kind)
from rivulus_amd.capi import RV_BOOLEAN, RV_FLOAT64, RV_INT64, RV_NULL, RV_STRING, Column, RvError
from test_join_gpu import cells_of, host_column, payloads, random_keys, upload

pytestmark = pytest.mark.gpu

RV_ERR_INVALID_ARG, RV_ERR_OUT_OF_BOUNDS, RV_ERR_UNSUPPORTED, RV_ERR_OOM = 1, 4, 5, 7
CASES = load_golden_cases()
NO_BUILD_IDX = (PROBE_SEMI, PROBE_ANTI)


def index_cells(col, rows, may_be_null):
    """An index column of rv_join_probe_kind as cells; checks its shape: Int64, `rows` long, validity attached exactly when a cell is
    null, null_count right, 0 under a null."""
    assert col.length == rows
    host = col.download() if rows else None
    if not rows:
        assert col.null_count() == 0
        return []
    assert host.dtype == RV_INT64
    valid = host.logical_valid()
    vals = host.logical_values()
    nulls = 0 if valid is None else int((~valid).sum())
    assert col.null_count() == nulls
    assert (valid is not None) == (nulls > 0)
    assert may_be_null or nulls == 0
    if valid is not None:
        assert not vals[~valid].any()
    return [None if valid is not None and not valid[i] else int(vals[i]) for i in range(rows)]


def probe_pairs_kind(table, key, kind):
    pi, bi, rows = table.probe(key, kind)
    ps = index_cells(pi, rows, kind == FULL_OUTER)
    if kind in NO_BUILD_IDX:
        assert bi is None
        return [(p, None) for p in ps]
    return list(zip(ps, index_cells(bi, rows, kind in (PROBE_OUTER, FULL_OUTER))))


def key_of(frame, name):
    return next((d, c) for n, d, c in frame if n == name)


def run_kind(ctx, kind, probe_frame, build_frame, build_key, probe_key, pad=0, want=None):
    """rv_hash_join_kind over frames of (name, dtype, cells) against the model (or the literal frame `want`); returns the row count."""
    bcols = [upload(ctx, d, c, pad) for _, d, c in build_frame]
    pcols = [upload(ctx, d, c, pad) for _, d, c in probe_frame]
    bi = [n for n, _, _ in build_frame].index(build_key)
    pi = [n for n, _, _ in probe_frame].index(probe_key)
    outs, rows = ctx.hash_join(bcols, bi, pcols, pi, kind=kind)
    if want is None:
        pairs = join_pairs(kind, build_frame[bi][1], build_frame[bi][2], probe_frame[pi][1], probe_frame[pi][2])
        want = materialize_kind(kind, probe_frame, build_frame, build_key, pairs)
    nrows = len(want[0][2])
    assert rows == nrows, KIND_NAMES[kind]
    assert len(outs) == len(want), KIND_NAMES[kind]
    for o, (name, dtype, cells) in zip(outs, want):
        got = o.download()
        assert got.dtype == dtype, (KIND_NAMES[kind], name)
        assert got.length == nrows, (KIND_NAMES[kind], name)
        assert comparable(dtype, cells_of(got)) == comparable(dtype, cells), (KIND_NAMES[kind], name)
        nulls = sum(c is None for c in cells)
        assert o.null_count() == nulls, (KIND_NAMES[kind], name)
        if dtype != RV_NULL:
            assert (o.info().has_validity != 0) == (nulls > 0), (KIND_NAMES[kind], name)
    return rows


# ---- the hand-written cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases(gpu_ctx, case):
    bd, bk = key_of(case["build"], case["build_key"])
    pd, pk = key_of(case["probe"], case["probe_key"])
    table = gpu_ctx.join_build(upload(gpu_ctx, bd, bk))
    key = upload(gpu_ctx, pd, pk)
    for kind in KINDS:
        assert probe_pairs_kind(table, key, kind) == case["pairs"][kind], KIND_NAMES[kind]
        run_kind(gpu_ctx, kind, case["probe"], case["build"], case["build_key"], case["probe_key"], want=case["frames"].get(kind))
    table.free()


# ---- every key dtype, with and without nulls, payloads of every dtype on both sides -----------------------------------------------
@pytest.mark.parametrize("dtype", [RV_INT64, RV_FLOAT64, RV_BOOLEAN, RV_NULL])
@pytest.mark.parametrize("null_share", [0.0, 0.1])
def test_key_dtypes_with_payloads(gpu_ctx, dtype, null_share):
    rng = np.random.default_rng(100 + dtype * 10 + int(null_share * 10))
    nb, np_ = (60, 150) if dtype in (RV_BOOLEAN, RV_NULL) else (2000, 3000)
    build = [("k", dtype, random_keys(rng, dtype, nb, 1500, null_share))] + payloads(rng, nb, "b")
    probe = payloads(rng, np_, "p") + [("k", dtype, random_keys(rng, dtype, np_, 1500, null_share))]
    for kind in KINDS:
        run_kind(gpu_ctx, kind, probe, build, "k", "k")


def test_boolean_build_side_with_one_value_leaves_a_tail(gpu_ctx):
    build = [("k", RV_BOOLEAN, [True, None, False, True]), ("s", RV_STRING, ["a", "b", None, "d"])]
    probe = [("k", RV_BOOLEAN, [True] * 70), ("v", RV_INT64, list(range(70)))]
    for kind in KINDS:
        run_kind(gpu_ctx, kind, probe, build, "k", "k")


def test_int64_keys_against_float64_keys(gpu_ctx):
    rng = np.random.default_rng(7)
    build = [("k", RV_INT64, random_keys(rng, RV_INT64, 400, 50, 0.1)), ("v", RV_INT64, list(range(400)))]
    probe = [("k", RV_FLOAT64, random_keys(rng, RV_FLOAT64, 600, 50, 0.1)), ("s", RV_STRING, [str(i) for i in range(600)])]
    for kind in KINDS:
        run_kind(gpu_ctx, kind, probe, build, "k", "k")


# ---- wave and tile seams x emit modes: pairs and kernel names ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5])
@pytest.mark.parametrize("longest", [1, 32, 33, 300])
def test_probe_lengths_and_list_lengths(gpu_ctx, n, longest):
    """kJoinLaneListMost = 32 (thresholds.hpp): mode 0 for lists of one row, 1 up to 32, 2 beyond; semi and anti joins always 0."""
    rng = np.random.default_rng(n * 1000 + longest)
    bcells = list(range(200)) + [7] * (longest - 1) + [None]
    bcells = [bcells[i] for i in rng.permutation(len(bcells))]
    pcells = rng.integers(-20, 280, n).tolist()
    if n > 2:
        pcells[n // 2] = None
        pcells[-1] = 7
    mode = 0 if longest <= 1 else 1 if longest <= 32 else 2
    table = gpu_ctx.join_build(upload(gpu_ctx, RV_INT64, bcells))
    assert table.info()[2] == longest
    key = upload(gpu_ctx, RV_INT64, pcells)
    for kind in KINDS:
        want = join_pairs(kind, RV_INT64, bcells, RV_INT64, pcells)
        assert probe_pairs_kind(table, key, kind) == want, KIND_NAMES[kind]
        probe_rows = sum(p is not None for p, _ in want)
        if kind == INNER:
            name = f"join_probe_emit<{mode}>"
        elif kind in NO_BUILD_IDX:
            name = f"join_probe_emit<0,{KIND_NAMES[kind]}>"
        else:
            name = f"join_probe_emit<{mode},{KIND_NAMES[kind]}>"
        assert gpu_ctx.last_kernel() == (name if probe_rows else "join_probe_count"), KIND_NAMES[kind]
    table.free()


def test_nothing_matches_and_everything_matches(gpu_ctx):
    build = [("k", RV_INT64, list(range(100, 3100))), ("s", RV_STRING, [str(i) for i in range(3000)])]
    miss = [("k", RV_INT64, list(range(-5000, 0))), ("f", RV_FLOAT64, [0.5] * 5000)]
    hit = [("k", RV_INT64, [100 + (i * 7) % 3000 for i in range(6000)]), ("b", RV_BOOLEAN, [True, False] * 3000)]
    for kind in KINDS:
        rows = run_kind(gpu_ctx, kind, miss, build, "k", "k")
        assert rows == {INNER: 0, PROBE_OUTER: 5000, FULL_OUTER: 8000, PROBE_SEMI: 0, PROBE_ANTI: 5000}[kind]
        rows = run_kind(gpu_ctx, kind, hit, build, "k", "k")
        assert rows == {INNER: 6000, PROBE_OUTER: 6000, FULL_OUTER: 6000, PROBE_SEMI: 6000, PROBE_ANTI: 0}[kind]


def test_table_without_a_single_list_still_emits_the_probe_rows(gpu_ctx):
    """A build side of NaNs only: the table's longest list is 0, the inner probe skips its passes; the other kinds may not."""
    table = gpu_ctx.join_build(upload(gpu_ctx, RV_FLOAT64, [float("nan")] * 5))
    assert table.info()[2] == 0
    key = upload(gpu_ctx, RV_FLOAT64, [1.0, None, float("nan")] * 1500)
    for kind in KINDS:
        want = join_pairs(kind, RV_FLOAT64, [float("nan")] * 5, RV_FLOAT64, [1.0, None, float("nan")] * 1500)
        assert probe_pairs_kind(table, key, kind) == want, KIND_NAMES[kind]
    table.free()


def test_empty_build_side_and_empty_probe_side(gpu_ctx):
    cols = lambda n, base: [("k", RV_INT64, [base + i for i in range(n)]), ("s", RV_STRING, ["v"] * n), ("b", RV_BOOLEAN, [True] * n),
                            ("f", RV_FLOAT64, [1.0] * n), ("z", RV_NULL, [None] * n)]
    for kind in KINDS:
        run_kind(gpu_ctx, kind, cols(5, 0), cols(0, 0), "k", "k")
        run_kind(gpu_ctx, kind, cols(0, 0), cols(5, 0), "k", "k")
        run_kind(gpu_ctx, kind, cols(0, 0), cols(0, 0), "k", "k")


# ---- collisions under the marks ------------------------------------------------------------------------------------------------------
def test_hash_masked_to_three_bits(gpu_ctx):
    rng = np.random.default_rng(3)
    gpu_ctx.set_option("join_hash_bits", 3)
    try:
        build = [("k", RV_FLOAT64, random_keys(rng, RV_FLOAT64, 2000, 400, 0.05)), ("v", RV_INT64, list(range(2000)))]
        probe = [("k", RV_FLOAT64, random_keys(rng, RV_FLOAT64, 3000, 400, 0.05))]
        for kind in KINDS:
            run_kind(gpu_ctx, kind, probe, build, "k", "k")
        bk = rng.integers(0, 10**15, 3000).tolist()
        pk = [bk[i] for i in rng.integers(0, 1500, 2000)] + rng.integers(0, 10**15, 500).tolist()  # half the build keys are never probed
        table = gpu_ctx.join_build(upload(gpu_ctx, RV_INT64, bk))
        key = upload(gpu_ctx, RV_INT64, pk)
        for kind in KINDS:
            assert probe_pairs_kind(table, key, kind) == join_pairs(kind, RV_INT64, bk, RV_INT64, pk), KIND_NAMES[kind]
        table.free()
    finally:
        gpu_ctx.set_option("join_hash_bits", 0)


# ---- slices ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [37, 101])
def test_sliced_inputs(gpu_ctx, pad):
    rng = np.random.default_rng(pad)
    build = [("k", RV_INT64, random_keys(rng, RV_INT64, 700, 400, 0.1))] + payloads(rng, 700, "b")
    probe = [("k", RV_INT64, random_keys(rng, RV_INT64, 900, 400, 0.1))] + payloads(rng, 900, "p")
    bk = [("k", RV_BOOLEAN, random_keys(rng, RV_BOOLEAN, 90, 2, 0.2))]
    pk = [("k", RV_BOOLEAN, random_keys(rng, RV_BOOLEAN, 70, 2, 0.2)), ("s", RV_STRING, [str(i) for i in range(70)])]
    for kind in KINDS:
        run_kind(gpu_ctx, kind, probe, build, "k", "k", pad=pad)
        run_kind(gpu_ctx, kind, pk, bk, "k", "k", pad=pad)


# ---- the inner kind is the inner join, and every kind is the same on every run -----------------------------------------------------
def raw(col):
    h = col.download()
    return (h.dtype, h.length, h.values.tobytes(), None if h.validity is None else h.validity.tobytes(),
            None if h.offsets is None else h.offsets.tobytes())


def test_inner_kind_equals_rv_join_probe_bit_for_bit(gpu_ctx):
    rng = np.random.default_rng(21)
    for longest in (1, 5, 40):
        bcells = random_keys(rng, RV_INT64, 3000, 3000 // longest, 0.05)
        pcells = random_keys(rng, RV_INT64, 9000, 3000 // longest, 0.05)
        table = gpu_ctx.join_build(upload(gpu_ctx, RV_INT64, bcells))
        key = upload(gpu_ctx, RV_INT64, pcells)
        pi, bi, rows = table.probe(key)
        name = gpu_ctx.last_kernel()
        qi, ci, rows2 = table.probe(key, INNER)
        assert gpu_ctx.last_kernel() == name and rows2 == rows and rows > 0
        assert raw(pi) == raw(qi) and raw(bi) == raw(ci)
        assert qi.null_count() == 0 and ci.null_count() == 0 and not qi.info().has_validity and not ci.info().has_validity
        table.free()


def test_the_same_call_twice_gives_identical_bytes(gpu_ctx):
    rng = np.random.default_rng(22)
    build = [("k", RV_INT64, random_keys(rng, RV_INT64, 4000, 300, 0.1))] + payloads(rng, 4000, "b")
    probe = [("k", RV_INT64, random_keys(rng, RV_INT64, 9000, 600, 0.1))] + payloads(rng, 9000, "p")
    bcols = [upload(gpu_ctx, d, c) for _, d, c in build]
    pcols = [upload(gpu_ctx, d, c) for _, d, c in probe]
    table = gpu_ctx.join_build(bcols[0])
    for kind in KINDS:
        a, rows_a = gpu_ctx.hash_join(bcols, 0, pcols, 0, kind=kind)
        b, rows_b = gpu_ctx.hash_join(bcols, 0, pcols, 0, kind=kind)
        assert rows_a == rows_b and [raw(x) for x in a] == [raw(x) for x in b], KIND_NAMES[kind]
        p1 = table.probe(pcols[0], kind)
        p2 = table.probe(pcols[0], kind)
        assert p1[2] == p2[2] and raw(p1[0]) == raw(p2[0]) and (p1[1] is None or raw(p1[1]) == raw(p2[1])), KIND_NAMES[kind]
    table.free()


# ---- the nullable gather on its own ---------------------------------------------------------------------------------------------------
TAKE_SOURCES = [
    (RV_INT64, [5, None, -7, 9, 11]),
    (RV_FLOAT64, [0.5, -0.0, None, float("nan"), 2.0]),
    (RV_BOOLEAN, [True, False, None, True, False]),
    (RV_STRING, ["a", "", None, "dddd", "ee"]),
    (RV_NULL, [None] * 5),
]


def _status(fn):
    with pytest.raises(RvError) as e:
        fn()
    return e.value.status, str(e.value)


@pytest.mark.parametrize("dtype,cells", TAKE_SOURCES, ids=["int64", "float64", "boolean", "string", "null"])
def test_take_device_nullable(gpu_ctx, dtype, cells):
    src = upload(gpu_ctx, dtype, cells)
    nonull = upload(gpu_ctx, dtype, [c for c in cells if c is not None] or [None]) if dtype != RV_NULL else src
    rng = np.random.default_rng(dtype)
    lists = [
        [4, None, 0, 2, None, 1, 3],
        [None] * 130,                                                     # every index null, more than two validity words
        [int(x) if rng.random() < 0.7 else None for x in rng.integers(0, 5, 200)],
        [3, 1, 4, 1],                                                     # no null: rv_take_device's result
        [],
    ]
    for idx in lists:
        for pad in (0, 37):  # the index list's own bitmap at a bit offset
            icol = upload(gpu_ctx, RV_INT64, idx, pad)
            out, = gpu_ctx.take_device_nullable([src], icol)
            want = [None if i is None else cells[i] for i in idx]
            got = out.download()
            assert got.dtype == dtype and got.length == len(idx)
            assert comparable(dtype, cells_of(got)) == comparable(dtype, want)
            nulls = sum(w is None for w in want)
            assert out.null_count() == nulls
            if dtype != RV_NULL:
                assert (out.info().has_validity != 0) == (nulls > 0)
                if dtype in (RV_INT64, RV_FLOAT64) and nulls:  # 0 under a null
                    assert not got.logical_values().view(np.uint64)[~got.logical_valid()].any()
    # a column without a bitmap gets one from the null indices alone
    if dtype != RV_NULL:
        out, = gpu_ctx.take_device_nullable([nonull], upload(gpu_ctx, RV_INT64, [0, None, 0]))
        assert out.null_count() == 1 and out.info().has_validity
    # a non-null index out of bounds: rv_take_device's text; a null over it is fine
    st, text = _status(lambda: gpu_ctx.take_device_nullable([src], upload(gpu_ctx, RV_INT64, [1, None, 9, 7])))
    assert st == RV_ERR_OUT_OF_BOUNDS and "Index 9 out of bounds for 5 rows" in text
    st, text = _status(lambda: gpu_ctx.take_device_nullable([src], upload(gpu_ctx, RV_INT64, [None, -1])))
    assert st == RV_ERR_OUT_OF_BOUNDS and "out of bounds for 5 rows" in text
    host = host_column(RV_INT64, [99, 2, 99])
    hidden = gpu_ctx.upload(Column.from_numpy(host.values, np.array([False, True, False])))
    out, = gpu_ctx.take_device_nullable([src], hidden)  # 99 lies under nulls
    assert comparable(dtype, cells_of(out.download())) == comparable(dtype, [None, cells[2], None])


def test_take_device_nullable_of_a_probe_s_index_columns(gpu_ctx):
    """rv_join_probe_kind's index columns are what rv_take_device_nullable takes: gathering by them is rv_hash_join_kind."""
    case = next(c for c in CASES if c["name"] == "name_clash_and_column_order")
    bcols = [upload(gpu_ctx, d, c) for _, d, c in case["build"]]
    pcols = [upload(gpu_ctx, d, c) for _, d, c in case["probe"]]
    table = gpu_ctx.join_build(bcols[0])
    pi, bi, rows = table.probe(pcols[1], FULL_OUTER)
    outs = gpu_ctx.take_device_nullable(pcols, pi) + gpu_ctx.take_device_nullable(bcols, bi)
    for o, (name, dtype, cells) in zip(outs, case["frames"][FULL_OUTER]):
        assert comparable(dtype, cells_of(o.download())) == comparable(dtype, cells), name
    table.free()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors(gpu_ctx):
    a = gpu_ctx.upload(host_column(RV_INT64, [1, 2, 3]))
    s = gpu_ctx.upload(host_column(RV_STRING, ["x", "y", "z"]))
    t = gpu_ctx.join_build(a)
    assert _status(lambda: t.probe(a, 5))[0] == RV_ERR_INVALID_ARG
    assert _status(lambda: t.probe(a, -1))[0] == RV_ERR_INVALID_ARG
    assert _status(lambda: t.probe(s, PROBE_SEMI))[0] == RV_ERR_UNSUPPORTED
    assert _status(lambda: gpu_ctx.hash_join([a], 0, [a], 0, kind=9))[0] == RV_ERR_INVALID_ARG
    assert _status(lambda: gpu_ctx.hash_join([a], 1, [a], 0, kind=PROBE_OUTER))[0] == RV_ERR_INVALID_ARG
    assert probe_pairs_kind(t, a, PROBE_ANTI) == []
    t.free()


def test_row_count_beyond_the_device_is_oom_before_any_allocation(gpu_ctx):
    """2e5 equal build keys x 1e6 probe rows of that key = 2e11 rows, 3.2 TB of indices: refused after the count pass, before any
    output is allocated or written; the context still works."""
    t = gpu_ctx.join_build(gpu_ctx.upload(Column.from_numpy(np.full(200_000, 9, np.int64))))
    key = gpu_ctx.upload(Column.from_numpy(np.full(1_000_000, 9, np.int64)))
    for kind in (PROBE_OUTER, FULL_OUTER):
        assert _status(lambda: t.probe(key, kind))[0] == RV_ERR_OOM
        assert gpu_ctx.last_kernel() == "join_probe_count"
    pi, bi, rows = t.probe(key, PROBE_SEMI)
    assert rows == 1_000_000 and bi is None
    small = gpu_ctx.upload(Column.from_numpy(np.array([9, 8], np.int64)))
    pi, bi, rows = t.probe(small, PROBE_OUTER)
    assert rows == 200_001 and bi.null_count() == 1 and bi.download().logical_values()[-2] == 199_999
    t.free()
