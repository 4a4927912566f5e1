"""GPU suite: what the device units behind the pipeline breakers (sort / topk / group_agg / window / window_frame / join / string_dict /
aggregate .hip) promise about themselves and no other suite holds them to: the launches a call counts under option profile_kernels and
the kernel it names, the read-back of MIN / MAX null counts round its eight-counter boundary, the join of every kind at its edges with
the kernel names that go with them, and the texts of the refusals.  The counts and names below were recorded from the library before
the units came to share their host-side steps (csrc/breaker_steps.hpp); they are facts about a call -- which passes it runs over this
data -- and change only when a unit's passes do.  Values are checked by the helpers of the units' own suites, against their models."""
import re

import numpy as np
import pytest

import test_group_agg_gpu as G
import test_window_gpu as W
from helpers import const
from outer_join_model import FULL_OUTER, INNER, KIND_NAMES, KINDS, PROBE_ANTI, PROBE_OUTER, PROBE_SEMI, join_pairs
from rivulus_amd import capi
from rivulus_amd.capi import RV_FLOAT64, RV_INT64, RV_STRING, Column, Predicate, RvError, Term
from test_join_gpu import probe_pairs, run_join, upload
from test_outer_join_gpu import probe_pairs_kind, run_kind

pytestmark = pytest.mark.gpu

RV_ERR_INVALID_ARG, RV_ERR_UNSUPPORTED, RV_ERR_OOM = 1, 5, 7
SORT_TILE = 256 * const("kSortRowsPerLane")
TOPK_TILE = 256 * const("kTopKCollectRowsPerLane")
WIN_TILE = W.TILE
JOIN_TILE = 4096  # kJoinTileRows (join_kernel.hpp)
LANE_MOST = const("kJoinLaneListMost")
SELECT_FROM = 1000  # option top_k_select_from_rows of the top-k cases: the select runs from this many rows on


@pytest.fixture(scope="module")
def ctx():
    with capi.Context(0) as c:
        c.set_option("profile_kernels", 1)
        c.set_option("top_k_select_from_rows", SELECT_FROM)
        yield c


def baseline(ctx):
    """a call that names a kernel of its own: what a call that launches nothing leaves standing"""
    idx = ctx.sort_indices(ctx.upload(Column.from_numpy(np.array([3, 1, 2], np.int64))))
    assert idx.download().logical_values().tolist() == [1, 2, 0] and ctx.last_kernel() == "sort_scatter"
    ctx.kernel_stats(reset=True)


def counted(ctx, call):
    """(launches the call added to the context's kernel statistics, the kernel it named)"""
    baseline(ctx)
    call()
    return ctx.kernel_stats()[1], ctx.last_kernel()


# ---- launch counts ------------------------------------------------------------------------------------------------------------------
def frame_of(ctx, n, seed=1):
    """(partition / group key with nulls, order key with ties and nulls, Int64 values, Float64 values), all nullable but the last"""
    rng = np.random.default_rng(seed + n)
    mask = lambda: rng.random(n) >= 0.2 if n else None
    host = [Column.from_numpy(rng.integers(0, 7, n, dtype=np.int64), mask()), Column.from_numpy(rng.integers(-5, 5, n, dtype=np.int64), mask()),
            Column.from_numpy(rng.integers(-1000, 1000, n, dtype=np.int64), mask()), Column.from_numpy(rng.integers(-99, 99, n).astype(np.float64))]
    return [ctx.upload(c) for c in host]


def strings_of(ctx, n):
    return ctx.upload(Column.from_strings([None if i % 11 == 3 else f"s{i % 37}" for i in range(n)]))


# case -> (rows of the unit's tile, the call over a frame_of those rows)
LAUNCH_CASES = {
    "sort_indices": (SORT_TILE, lambda ctx, f: ctx.sort_indices(f[2])),
    "sort_two_keys": (SORT_TILE, lambda ctx, f: ctx.sort(f, [(1, 1), (2, 2)])),
    "top_k_select": (TOPK_TILE, lambda ctx, f: ctx.top_k(f, [(3, 0), (1, 1)], 10)),
    "top_k_whole_sort": (TOPK_TILE, lambda ctx, f: ctx.top_k(f, [(3, 0), (1, 1)], f[0].length)),
    "hash_aggregate": (G.TILE, lambda ctx, f: ctx.hash_aggregate(f[0], f[2:], [("sum", 0), ("sum", 1), ("min", 0)])),
    "hash_aggregate_keys": (G.TILE, lambda ctx, f: ctx.hash_aggregate_keys(f[:2], f[2:], [("sum", 0), ("sum", 1), ("min", 0)])),
    "window": (WIN_TILE, lambda ctx, f: ctx.window(f, [0], [(1, 0)], [("cum_sum", 2), ("lag", 3, 1)])),
    "window_frames": (WIN_TILE, lambda ctx, f: ctx.window_frames(f, [0], [(1, 0)], [("sum", 2, 1, 1)])),
    "string_dict_build": (4096, lambda ctx, f: ctx.string_dict_build(strings_of(ctx, f[0].length))),
    "filter_agg": (4096, lambda ctx, f: ctx.filter_agg(f, Predicate([Term(2, ">", 0)]), 3)),
}
# (case, rows) -> (kernel_launches, last_kernel) of the library before the units shared their steps
LAUNCHES = {
    ("sort_indices", 0): (0, "sort_scatter"),
    ("sort_indices", 1): (3, "sort_widen"),
    ("sort_indices", "tile+1"): (47, "sort_scatter"),
    ("sort_two_keys", 0): (0, "sort_scatter"),
    ("sort_two_keys", 1): (6, "sort_widen"),
    ("sort_two_keys", "tile+1"): (94, "sort_scatter"),
    ("top_k_select", 0): (0, "sort_scatter"),
    ("top_k_select", 1): (6, "sort_widen"),
    ("top_k_select", "tile+1"): (63, "topk_collect"),
    ("top_k_whole_sort", 0): (0, "sort_scatter"),
    ("top_k_whole_sort", 1): (6, "sort_widen"),
    ("top_k_whole_sort", "tile+1"): (89, "sort_scatter"),
    ("hash_aggregate", 0): (0, "sort_scatter"),
    ("hash_aggregate", 1): (2, "group_accumulate<lds>+group_f64_sum"),
    ("hash_aggregate", "tile+1"): (2, "group_accumulate<lds>+group_f64_sum"),
    ("hash_aggregate_keys", 0): (0, "sort_scatter"),
    ("hash_aggregate_keys", 1): (2, "group_accumulate<lds>+group_f64_sum"),
    ("hash_aggregate_keys", "tile+1"): (2, "group_accumulate<lds>+group_f64_sum"),
    ("window", 0): (0, ""),
    ("window", 1): (11, "window_scan"),
    ("window", "tile+1"): (59, "window_scan"),
    ("window_frames", 0): (0, ""),
    ("window_frames", 1): (21, "window_frame"),
    ("window_frames", "tile+1"): (70, "window_frame"),
    ("string_dict_build", 0): (0, "sort_scatter"),
    ("string_dict_build", 1): (2, "str_dict_encode"),
    ("string_dict_build", "tile+1"): (2, "str_dict_encode"),
    ("filter_agg", 0): (0, "sort_scatter"),
    ("filter_agg", 1): (1, "filter_agg_kernel<2,8,1,4,3>"),
    ("filter_agg", "tile+1"): (1, "filter_agg_kernel<2,8,1,4,3>"),
}


def launch_case(ctx, case, rows):
    tile, call = LAUNCH_CASES[case]
    n = tile + 1 if rows == "tile+1" else rows
    f = frame_of(ctx, n)
    return counted(ctx, lambda: call(ctx, f))


@pytest.mark.parametrize("rows", [0, 1, "tile+1"])
@pytest.mark.parametrize("case", list(LAUNCH_CASES))
def test_launches_counted_and_kernel_named(ctx, case, rows):
    got = launch_case(ctx, case, rows)
    print(f"{case} {rows}: {got}")
    assert got == LAUNCHES[case, rows]


def test_the_select_ran_where_the_case_says_so(ctx):
    f = frame_of(ctx, TOPK_TILE + 1)
    ctx.top_k(f, [(3, 0), (1, 1)], 10)
    assert ctx.last_kernel() == "topk_collect"
    ctx.top_k(f, [(3, 0), (1, 1)], TOPK_TILE + 1)
    assert ctx.last_kernel() != "topk_collect"


# ---- the eight-counter boundary of the null-count read-back ---------------------------------------------------------------------------
def null_shapes(rng, n, key):
    """Value columns whose MIN / MAX differ in what they leave of the bitmap: no null at all (no bitmap), nulls in every group but never a
    whole group (the bitmap is dropped again), whole groups null (kept), every cell null (every result null); Int64 and Float64 of each."""
    some = rng.random(n) >= 0.3
    some[:16] = True  # (the first rows hold every key: no group is null throughout)
    groups_out = key % 3 != 0
    none = np.zeros(n, bool)
    cols = []
    for valid in (None, some, groups_out, none):
        cols.append(("i64", rng.integers(-1000, 1000, n, dtype=np.int64), valid))
        cols.append(G.f64_col(rng, n, 0.0)[:2] + (valid,))
    return cols


@pytest.mark.parametrize("outputs", [8, 9, 17])
def test_group_min_max_round_the_eight_counters(ctx, outputs):
    """8 MIN / MAX outputs are one read-back, 9 two, 17 three: values, null_count and validity presence of every one (G.check)."""
    rng = np.random.default_rng(outputs)
    n = 3000
    key = np.concatenate([np.arange(7), rng.integers(0, 7, n - 7)]).astype(np.int64)
    cols = null_shapes(rng, n, key)
    specs = [(("min", "max")[(j // len(cols)) % 2], (j * 3) % len(cols)) for j in range(outputs)]
    specs.insert(1, ("sum", 0))  # the read-backs are counted over MIN / MAX alone, wherever the others stand
    outs, _ = G.check(ctx, (key, None), cols, specs, what=f"{outputs} MIN / MAX")
    bitmaps = [bool(o.info().has_validity) for o, s in zip(outs[1:], specs) if s[0] != "sum"]
    assert any(bitmaps) and not all(bitmaps)


def test_window_nine_cum_min(ctx):
    """nine CUM_MIN expressions: the ninth attaches after the first eight were read back"""
    n = WIN_TILE + 1
    rng = np.random.default_rng(9)
    part = rng.integers(0, 7, n).astype(np.int64)
    part[:7] = np.arange(7)
    shapes = null_shapes(rng, n, part)
    cols = [W.i64(part), W.i64(rng.integers(-5, 5, n))] + [(d, v, m) for d, v, m in shapes]
    exprs = [("cum_min", 2 + (j * 3) % len(shapes)) for j in range(9)]
    got = W.check(ctx, cols, [0], [(1, 0)], exprs, exact_float=True, what="nine cum_min")
    bitmaps = [bool(o.info().has_validity) for o in got]
    assert any(bitmaps) and not all(bitmaps)
    assert ctx.last_kernel() == "window_scan"


# ---- the join, all five kinds -------------------------------------------------------------------------------------------------------
NAN = float("nan")


def join_shapes():
    """name -> (build dtype, build key cells, probe dtype, probe key cells)"""
    rng = np.random.default_rng(5)
    shapes = {
        "empty_probe": (RV_INT64, [3, None, 5, 3], RV_INT64, []),
        "one_probe_row": (RV_INT64, [3, None, 5, 3], RV_INT64, [3]),
        "build_all_null": (RV_INT64, [None] * 5, RV_INT64, [1, None, 2]),
        "build_all_nan": (RV_FLOAT64, [NAN] * 5, RV_FLOAT64, [1.0, None, NAN]),
        "empty_build": (RV_INT64, [], RV_INT64, [1, None]),
        "dtypes_differ": (RV_INT64, [1, None, 2, None], RV_FLOAT64, [1.0, None, 2.0]),
    }
    for longest in (1, LANE_MOST, LANE_MOST + 1):
        build = list(range(50)) + [7] * (longest - 1)
        build = [build[i] for i in rng.permutation(len(build))]
        probe = rng.integers(-10, 70, JOIN_TILE + 1).tolist()
        probe[100], probe[-1] = None, 7
        shapes[f"lists_of_{longest}"] = (RV_INT64, build, RV_INT64, probe)
    return shapes


JOIN_SHAPES = join_shapes()
# (shape, kind or "rv_join_probe") -> (launches counted, kernel named by the probe, kernel named by the whole join)
JOIN_KERNELS = {
    ("empty_probe", "rv_join_probe"): (0, "sort_scatter", "sort_scatter"),
    ("empty_probe", INNER): (0, "sort_scatter", "sort_scatter"),
    ("empty_probe", PROBE_OUTER): (0, "join_probe_count", "join_probe_count"),
    ("empty_probe", FULL_OUTER): (0, "join_probe_count", "join_probe_count"),
    ("empty_probe", PROBE_SEMI): (0, "join_probe_count", "join_probe_count"),
    ("empty_probe", PROBE_ANTI): (0, "join_probe_count", "join_probe_count"),
    ("one_probe_row", "rv_join_probe"): (0, "join_probe_emit<1>", "join_probe_emit<1>"),
    ("one_probe_row", INNER): (0, "join_probe_emit<1>", "join_probe_emit<1>"),
    ("one_probe_row", PROBE_OUTER): (0, "join_probe_emit<1,outer>", "join_probe_emit<1,outer>"),
    ("one_probe_row", FULL_OUTER): (0, "join_probe_emit<1,full>", "join_probe_emit<1,full>"),
    ("one_probe_row", PROBE_SEMI): (0, "join_probe_emit<0,semi>", "join_probe_emit<0,semi>"),
    ("one_probe_row", PROBE_ANTI): (0, "join_probe_count", "join_probe_count"),
    ("build_all_null", "rv_join_probe"): (0, "join_probe_emit<1>", "join_probe_emit<1>"),
    ("build_all_null", INNER): (0, "join_probe_emit<1>", "join_probe_emit<1>"),
    ("build_all_null", PROBE_OUTER): (0, "join_probe_emit<1,outer>", "join_probe_emit<1,outer>"),
    ("build_all_null", FULL_OUTER): (0, "join_probe_emit<1,full>", "join_probe_emit<1,full>"),
    ("build_all_null", PROBE_SEMI): (0, "join_probe_emit<0,semi>", "join_probe_emit<0,semi>"),
    ("build_all_null", PROBE_ANTI): (0, "join_probe_emit<0,anti>", "join_probe_emit<0,anti>"),
    ("build_all_nan", "rv_join_probe"): (0, "sort_scatter", "sort_scatter"),
    ("build_all_nan", INNER): (0, "sort_scatter", "sort_scatter"),
    ("build_all_nan", PROBE_OUTER): (0, "join_probe_emit<0,outer>", "join_probe_emit<0,outer>"),
    ("build_all_nan", FULL_OUTER): (0, "join_probe_emit<0,full>", "join_probe_emit<0,full>"),
    ("build_all_nan", PROBE_SEMI): (0, "join_probe_count", "join_probe_count"),
    ("build_all_nan", PROBE_ANTI): (0, "join_probe_emit<0,anti>", "join_probe_emit<0,anti>"),
    ("empty_build", "rv_join_probe"): (0, "sort_scatter", "sort_scatter"),
    ("empty_build", INNER): (0, "sort_scatter", "sort_scatter"),
    ("empty_build", PROBE_OUTER): (0, "join_probe_emit<0,outer>", "join_probe_emit<0,outer>"),
    ("empty_build", FULL_OUTER): (0, "join_probe_emit<0,full>", "join_probe_emit<0,full>"),
    ("empty_build", PROBE_SEMI): (0, "join_probe_count", "join_probe_count"),
    ("empty_build", PROBE_ANTI): (0, "join_probe_emit<0,anti>", "join_probe_emit<0,anti>"),
    ("dtypes_differ", "rv_join_probe"): (0, "join_probe_emit<1>", "join_probe_emit<1>"),
    ("dtypes_differ", INNER): (0, "join_probe_emit<1>", "join_probe_emit<1>"),
    ("dtypes_differ", PROBE_OUTER): (0, "join_probe_emit<1,outer>", "join_probe_emit<1,outer>"),
    ("dtypes_differ", FULL_OUTER): (0, "join_probe_emit<1,full>", "join_probe_emit<1,full>"),
    ("dtypes_differ", PROBE_SEMI): (0, "join_probe_emit<0,semi>", "join_probe_emit<0,semi>"),
    ("dtypes_differ", PROBE_ANTI): (0, "join_probe_emit<0,anti>", "join_probe_emit<0,anti>"),
    ("lists_of_1", "rv_join_probe"): (0, "join_probe_emit<0>", "join_probe_emit<0>"),
    ("lists_of_1", INNER): (0, "join_probe_emit<0>", "join_probe_emit<0>"),
    ("lists_of_1", PROBE_OUTER): (0, "join_probe_emit<0,outer>", "join_probe_emit<0,outer>"),
    ("lists_of_1", FULL_OUTER): (0, "join_probe_emit<0,full>", "join_probe_emit<0,full>"),
    ("lists_of_1", PROBE_SEMI): (0, "join_probe_emit<0,semi>", "join_probe_emit<0,semi>"),
    ("lists_of_1", PROBE_ANTI): (0, "join_probe_emit<0,anti>", "join_probe_emit<0,anti>"),
    ("lists_of_32", "rv_join_probe"): (0, "join_probe_emit<1>", "join_probe_emit<1>"),
    ("lists_of_32", INNER): (0, "join_probe_emit<1>", "join_probe_emit<1>"),
    ("lists_of_32", PROBE_OUTER): (0, "join_probe_emit<1,outer>", "join_probe_emit<1,outer>"),
    ("lists_of_32", FULL_OUTER): (0, "join_probe_emit<1,full>", "join_probe_emit<1,full>"),
    ("lists_of_32", PROBE_SEMI): (0, "join_probe_emit<0,semi>", "join_probe_emit<0,semi>"),
    ("lists_of_32", PROBE_ANTI): (0, "join_probe_emit<0,anti>", "join_probe_emit<0,anti>"),
    ("lists_of_33", "rv_join_probe"): (0, "join_probe_emit<2>", "join_probe_emit<2>"),
    ("lists_of_33", INNER): (0, "join_probe_emit<2>", "join_probe_emit<2>"),
    ("lists_of_33", PROBE_OUTER): (0, "join_probe_emit<2,outer>", "join_probe_emit<2,outer>"),
    ("lists_of_33", FULL_OUTER): (0, "join_probe_emit<2,full>", "join_probe_emit<2,full>"),
    ("lists_of_33", PROBE_SEMI): (0, "join_probe_emit<0,semi>", "join_probe_emit<0,semi>"),
    ("lists_of_33", PROBE_ANTI): (0, "join_probe_emit<0,anti>", "join_probe_emit<0,anti>"),
}


def join_case(ctx, shape, kind):
    bd, build, pd, probe = JOIN_SHAPES[shape]
    table = ctx.join_build(upload(ctx, bd, build))
    key = upload(ctx, pd, probe)
    baseline(ctx)
    if kind == "rv_join_probe":
        got = probe_pairs(table, key)
        want = join_pairs(INNER, bd, build, pd, probe)
    else:
        got = probe_pairs_kind(table, key, kind)
        want = join_pairs(kind, bd, build, pd, probe)
    # (the index columns' own read-backs name no kernel: what stands after the probe is the probe's)
    launches, after_probe = ctx.kernel_stats()[1], ctx.last_kernel()
    assert got == want, (shape, kind)
    table.free()
    bframe = [("k", bd, build), ("v", RV_INT64, list(range(len(build))))]
    pframe = [("w", RV_STRING, [str(i) for i in range(len(probe))]), ("k", pd, probe)]
    if kind == "rv_join_probe":
        run_join(ctx, pframe, bframe, "k", "k")
    else:
        run_kind(ctx, kind, pframe, bframe, "k", "k")
    return launches, after_probe, ctx.last_kernel()


@pytest.mark.parametrize("kind", ["rv_join_probe"] + list(KINDS), ids=["rv_join_probe"] + [KIND_NAMES[k] for k in KINDS])
@pytest.mark.parametrize("shape", list(JOIN_SHAPES))
def test_join_kinds_at_the_edges(ctx, shape, kind):
    got = join_case(ctx, shape, kind)
    print(f"{shape} {kind}: {got}")
    assert got == JOIN_KERNELS[shape, kind]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def refusal(call):
    with pytest.raises(RvError) as e:
        call()
    return e.value.status, e.value.message


def test_refusal_texts_and_a_good_call_after_each(ctx):
    f = frame_of(ctx, 100)
    s = strings_of(ctx, 100)
    table = ctx.join_build(f[0])
    nine = [f[0]] * 9
    cases = [
        (lambda: ctx.sort(f, [(0, 0), (5, 0)]), RV_ERR_INVALID_ARG, "rv_sort: key 1 is column 5 of 4"),
        (lambda: ctx.top_k(f, [(9, 0)], 3), RV_ERR_INVALID_ARG, "rv_top_k: key 0 is column 9 of 4"),
        (lambda: ctx.sort(f, []), RV_ERR_INVALID_ARG, "rv_sort: no sort keys"),
        (lambda: ctx.top_k(f, [], 3), RV_ERR_INVALID_ARG, "rv_top_k: no sort keys"),
        (lambda: ctx.sort_indices(f[0], flags=4), RV_ERR_INVALID_ARG, "rv_sort_indices: unknown flag bits 0x4"),
        (lambda: ctx.sort(f, [(0, 7)]), RV_ERR_INVALID_ARG, "rv_sort: unknown flag bits 0x4"),
        (lambda: ctx.top_k_indices(f[0], 3, flags=8), RV_ERR_INVALID_ARG, "rv_top_k_indices: unknown flag bits 0x8"),
        (lambda: ctx.top_k(f, [(0, 12)], 3), RV_ERR_INVALID_ARG, "rv_top_k: unknown flag bits 0xc"),
        (lambda: ctx.window(f, [7], [], [("row_number", 0)]), RV_ERR_INVALID_ARG, "rv_window: partition key 0 is column 7 of 4"),
        (lambda: ctx.window(f, [], [(0, 0), (6, 0)], [("row_number", 0)]), RV_ERR_INVALID_ARG, "rv_window: order key 1 is column 6 of 4"),
        (lambda: ctx.window_frames(f, [0, 4], [], [("ntile", 0, 2)]), RV_ERR_INVALID_ARG, "rv_window_frames: partition key 1 is column 4 of 4"),
        (lambda: ctx.window_frames(f, [], [(5, 0)], [("ntile", 0, 2)]), RV_ERR_INVALID_ARG, "rv_window_frames: order key 0 is column 5 of 4"),
        (lambda: ctx.window(f, [], [(1, 4)], [("row_number", 0)]), RV_ERR_INVALID_ARG, "rv_window: unknown flag bits 0x4"),
        (lambda: ctx.hash_aggregate(f[0], f[2:], [("sum", 3)]), RV_ERR_INVALID_ARG, "rv_hash_aggregate: aggregate 0 reads value column 3 of 2"),
        (lambda: ctx.hash_aggregate_keys(nine, f[2:], [("sum", 0)]), RV_ERR_INVALID_ARG, "rv_hash_aggregate_keys: 9 key columns; one to 8 are taken"),
        (lambda: ctx.group_ids_keys(nine), RV_ERR_INVALID_ARG, "rv_group_ids_keys: 9 key columns; one to 8 are taken"),
        (lambda: ctx.group_ids(f[3]), RV_ERR_UNSUPPORTED,
         "rv_group_ids: only Int64 (and Null) key columns are supported on the device; String keys go through rv_string_dict_build ids"),
        (lambda: table.probe(f[0], 5), RV_ERR_INVALID_ARG, "rv_join_probe_kind: unknown join kind 5"),
        (lambda: ctx.hash_join(f, 0, f, 0, kind=7), RV_ERR_INVALID_ARG, "rv_hash_join_kind: unknown join kind 7"),
        (lambda: ctx.hash_join_chunked(table, f, 0, f, 0, 10, kind=-1), RV_ERR_INVALID_ARG, "rv_hash_join_chunked_kind: unknown join kind -1"),
        (lambda: ctx.hash_join_chunked(table, f, 0, f, 0, 10, kind=FULL_OUTER), RV_ERR_UNSUPPORTED,
         "rv_hash_join_chunked_kind: RV_JOIN_FULL_OUTER has no batched form (its unmatched build rows belong to no probe batch); use rv_hash_join_kind"),
        # the inner join answers under rv_join_probe's name whichever entry point it came through
        (lambda: table.probe(s), RV_ERR_UNSUPPORTED, "rv_join_probe: String join keys are not supported on the device (String payload columns are)"),
        (lambda: table.probe(s, INNER), RV_ERR_UNSUPPORTED, "rv_join_probe: String join keys are not supported on the device (String payload columns are)"),
        (lambda: table.probe(s, PROBE_SEMI), RV_ERR_UNSUPPORTED,
         "rv_join_probe_kind: String join keys are not supported on the device (String payload columns are)"),
    ]
    for call, status, text in cases:
        assert refusal(call) == (status, text)
        baseline(ctx)
    table.free()


def test_join_out_of_memory_texts(ctx):
    """150 000 equal build keys x 150 000 probe rows of that key are 2.25e10 rows, 360 GB of indices: refused after the count pass under
    the entry point's own wording; the inner join through rv_join_probe_kind words it as rv_join_probe does."""
    rows = 150_000
    table = ctx.join_build(ctx.upload(Column.from_numpy(np.full(rows, 9, np.int64))))
    key = ctx.upload(Column.from_numpy(np.full(rows, 9, np.int64)))
    total = rows * rows
    inner = rf"rv_join_probe: {total} pairs need {total} x 16 bytes of output, more than the device's \d+ bytes"
    other = rf"rv_join_probe_kind: {total} rows need {total} x 16 bytes of output, more than the device's \d+ bytes"
    for call, text in [(lambda: table.probe(key), inner), (lambda: table.probe(key, INNER), inner), (lambda: table.probe(key, PROBE_OUTER), other),
                       (lambda: table.probe(key, FULL_OUTER), other)]:
        status, message = refusal(call)
        assert status == RV_ERR_OOM and re.fullmatch(text, message), message
        assert ctx.last_kernel() == "join_probe_count"
        baseline(ctx)
    table.free()

# (No case fails an entry point after its outputs exist: option inject_failure reaches the filter and aggregate queries only -- rv_sort,
#  rv_top_k, the grouped aggregate, the window and the joins never ask it -- and the units have no other switch that fails them late.)
