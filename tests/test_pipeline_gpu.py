"""Operator pipelines on the device (-m gpu): every operator fed columns another operator wrote, against the composed model of
tests/pipeline_model.py.  Exact equality of bits throughout (every NaN one value: payloads are unspecified); no tolerance anywhere.

Random cases (tests/pipeline_cases.py; RV_PIPELINE_CASES seeds, default 200) run twice:
  hands-off   only the final frame is downloaded; no info() / null_count() touches an intermediate column;
  inspected   after every step every column is downloaded and compared with the model's intermediate frame, metadata included.
Both must equal the model, so a dependence on a cached null_count or a run-to-run difference shows as well.  Directed pipelines:
one named test per edge, each at most 2 * TILE + 1 rows; tests/golden/pipeline_cases.json holds the same pipelines at toy size.

Not reachable: a `place`d filter output (fused_launch.hip, run_segmented_pass) keeps its bitmap with zero nulls only on the per-stretch
views inside the library; the column rv_filter_project hands out gets a bitmap iff a null survived.  The state itself -- bitmap attached,
zero nulls, on a column an operator wrote -- is made through rv_eval_arith over a column uploaded with an all-valid bitmap instead
(test_bitmap_without_nulls_is_what_arith_wrote), and handed to arith, sort, group and join in one short pipeline each
(test_directed_pipeline[bitmap_without_nulls_*]), which assert that the consumer's input was in that state."""
import os

import numpy as np
import pytest

import pipeline_cases as pc
import pipeline_device as pd
import pipeline_model as pm
from rivulus_amd.capi import Column, Predicate, Term

pytestmark = pytest.mark.gpu
N_CASES = int(os.environ.get("RV_PIPELINE_CASES", 200))
ROWS = 2 * pc.TILE + 1


def _both_modes(ctx, case, tmp_path=None, what=None):
    model, build_models = pm.run_case(case)
    what = what or f"seed={case['seed']} n={case['n']} source={case['source']['how']}"
    for look in (False, True):
        frame = pd.run_pipeline(ctx, case["source"], case["steps"], case["builds"], model, build_models, look, what, tmp_path)
    return frame, model


@pytest.mark.parametrize("seed", range(N_CASES))
def test_random_pipeline_matches_model(gpu_ctx, tmp_path, seed):
    _both_modes(gpu_ctx, pc.case(seed), tmp_path)


def _usable(ctx):
    """the context answers a normal query"""
    x = ctx.upload(Column.from_numpy(np.arange(1000, dtype=np.int64)))
    outs, rows, _ = ctx.filter_project([x], Predicate([Term(0, ">", 899)]), [0])
    assert rows == 100 and list(outs[0].download().logical_values()[:2]) == [900, 901]


@pytest.mark.parametrize("name", [n for n in pc.DIRECTED if not n.startswith("empty_")])
def test_directed_pipeline(gpu_ctx, name):
    """div_probe_key: a / b with zeros in b as probe key against a build side that holds key 0 -- the 0 under a null quotient must not meet it;
    div_build_key: the same quotients on the side that is hashed; div_group_key: the same column as group key beside a genuine 0 group; div_sort_key_f: as sort key under the four flag combinations;
    minmax_null_groups: MIN / MAX with null groups -> sort by the aggregate -> take_device; null_columns_ride_along: Null-dtype columns through
    take, sort, join payloads and COUNT; bitmap_without_nulls_<consumer>: see the module text."""
    case = pc.directed_case(name, ROWS)
    _, model = _both_modes(gpu_ctx, case, what=name)
    if name in ("div_probe_key", "div_build_key"):
        q = model[1][0][3]
        assert pm.null_count(q) > 0 and (q[1][pm.valid_of(q)] == 0).any(), "the case lost its point: no null quotient beside a genuine 0"
    if name.startswith("bitmap_without_nulls_"):
        pc.assert_consumer_met_bitmap_without_nulls(case)


def test_bitmap_without_nulls_is_what_arith_wrote(gpu_ctx):
    """The state the pipelines `bitmap_without_nulls_*` are about, asserted through info(): attached, zero nulls, on a device-made column."""
    frame, steps, _ = pc.directed("bitmap_without_nulls_arith", ROWS)
    d = [gpu_ctx.upload(pd.to_host(c)) for c in frame]
    out = gpu_ctx.eval_arith(d, pm.tup(steps[0]["tree"]))
    i = out.info()
    assert i.has_validity == 1 and i.null_count == 0 and out.null_count() == 0


@pytest.mark.parametrize("name", [n for n in pc.DIRECTED if n.startswith("empty_")])
def test_empty_intermediate(gpu_ctx, name):
    """A filter that keeps nothing, then each consumer (and the empty frame as a join's build side): a zero-row frame of the right dtypes,
    and the context answers a normal query afterwards."""
    case = pc.directed_case(name, ROWS)
    frame, model = _both_modes(gpu_ctx, case, what=name)
    assert pm.rows(model[-1][0]) == 0
    assert [pm.DTYPE_OF_RV[c.info().dtype] for c in frame] == pm.dtypes(model[-1][0]) and all(c.info().length == 0 for c in frame)
    _usable(gpu_ctx)


def _keyed_frame(n, seed=11):
    rng = np.random.default_rng(seed)
    key = ("i64", rng.integers(-3, 40, n, dtype=np.int64), rng.random(n) > 0.1)
    val = ("f64", pc.dyadic_cells(seed, n, pc.SCALE)[1], rng.random(n) > 0.2)
    return [key, val]


def test_gids_and_first_row_as_key_and_index(gpu_ctx):
    """rv_group_ids' outputs consumed: hash_aggregate keyed on gids reproduces the grouping, take_device(first_row) the key cells."""
    frame = _keyed_frame(ROWS)
    d = [gpu_ctx.upload(pd.to_host(c)) for c in frame]
    gids, first, groups = gpu_ctx.group_ids(d[0])
    step = {"kind": "group", "key": 0, "specs": [("count_rows", None), ("sum", 1), ("min", 1)]}
    want = pm.step_group(frame, step)
    res = pm.group_result(frame, step)
    assert groups == res["groups"]
    outs, first2, groups2 = gpu_ctx.hash_aggregate(gids, d, step["specs"])
    assert groups2 == groups
    got = pd.download(outs)
    assert pm.column_diff(got[0], ("i64", np.arange(groups, dtype=np.int64), None)) is None, "the key cells of a grouping by gids are 0 .. G-1"
    assert pm.frame_diff(got[1:], want[1:]) is None, pm.frame_diff(got[1:], want[1:])
    assert pm.column_diff(pd.download([first2])[0], ("i64", res["first_row"], None)) is None
    cells = pd.download(gpu_ctx.take_device([d[0]], first))[0]
    assert pm.column_diff(cells, want[0]) is None, pm.column_diff(cells, want[0])
    # gids as a sort key: rows grouped, each group in row order
    order = pd.download(gpu_ctx.take_device(d, gpu_ctx.sort_indices(gids)))
    assert pm.frame_diff(order, pm.take_frame(frame, np.argsort(res["gids"], kind="stable"))) is None


def test_index_columns_made_on_the_device(gpu_ctx):
    """rv_sort_indices' output as `prior` of the next key and as the index of take_device; rv_selection_indices' output in the same roles."""
    frame = _keyed_frame(ROWS, seed=12)
    d = [gpu_ctx.upload(pd.to_host(c)) for c in frame]
    sm = pm.sort_columns(frame)
    by_val = gpu_ctx.sort_indices(d[1], flags=3)
    both = gpu_ctx.sort_indices(d[0], flags=0, prior=by_val)
    want = pm.sort_model.sort_indices(sm[0], 0, pm.sort_model.sort_indices(sm[1], 3))
    assert pm.frame_diff(pd.download(gpu_ctx.take_device(d, both)), pm.take_frame(frame, want)) is None
    assert np.array_equal(both.download().logical_values(), want)
    # a selection's indices as the index of a take; then, over the frame that take wrote, a selection that keeps every row: its indices
    # are the identity permutation, which the next sort takes as `prior`
    step = {"kind": "filter", "terms": [(0, ">=", 5)], "nulls": "drops", "expr": None}
    keep = np.flatnonzero(pm.survivors(frame, step))
    _, rows, sel = gpu_ctx.filter_project(d, pm.predicate_of(step), [0], True)
    idx = gpu_ctx.selection_indices(sel)
    assert rows == len(keep) and np.array_equal(idx.download().logical_values(), keep)
    kept = gpu_ctx.take_device(d, idx)
    small = pm.take_frame(frame, keep)
    assert pm.frame_diff(pd.download(kept), small) is None
    ident = gpu_ctx.selection_indices(gpu_ctx.compare(kept[0], ">=", 5))  # every kept row: 0 .. rows-1, a permutation made by a selection
    chained = gpu_ctx.sort_indices(kept[1], flags=1, prior=ident)
    assert np.array_equal(chained.download().logical_values(), pm.sort_model.sort_indices(pm.sort_columns(small)[1], 1))


def test_join_string_payload_sliced_into_string_consumers(gpu_ctx):
    """A join output's String payload, sliced at offset 1 (its first offset is then not 0), into string_dict_build, compare with a String
    literal and concat with itself."""
    n = ROWS
    rng = np.random.default_rng(13)
    probe = [("i64", rng.integers(0, 6, n, dtype=np.int64), rng.random(n) > 0.1)]
    build = [("i64", np.array([0, 1, 2, 3, 3, 9], np.int64), np.array([1, 1, 1, 1, 1, 0], bool)), ("str", ["Bob", "", None, "名前", "Bob", "zz"], np.array([1, 1, 0, 1, 1, 1], bool))]
    joined = pm.step_join(probe, {"probe_key": 0, "build_key": 0}, build)
    outs, rows = gpu_ctx.hash_join([gpu_ctx.upload(pd.to_host(c)) for c in build], 0, [gpu_ctx.upload(pd.to_host(c)) for c in probe], 0)
    assert rows == pm.rows(joined) > 100
    s = outs[1].slice(1, rows - 1)
    want = pm.take_col(joined[1], np.arange(1, rows))
    assert pm.column_diff(pd.download([s])[0], want) is None
    sdict, ids = gpu_ctx.string_dict_build(s)
    assert pm.column_diff(pd.download([ids])[0], pm.string_ids(want)) is None, "string_dict_build over the sliced join payload"
    assert sdict.info()[1] == len({x for x in want[1] if x is not None})
    sdict.free()
    mask = pd.download([gpu_ctx.compare(s, "==", "Bob")])[0]
    ok = pm.valid_of(want)
    assert np.array_equal(pm.valid_of(mask), ok) and np.array_equal(mask[1][ok], np.array([x == "Bob" for x in want[1]])[ok]), "compare with a String literal"
    twice = pd.download([gpu_ctx.concat([s, s])])[0]
    assert pm.column_diff(twice, pm.take_col(want, np.concatenate([np.arange(rows - 1)] * 2))) is None, "concat with itself"


@pytest.mark.parametrize("as_reference", [True, False])
def test_csv_batch_into_group_and_sort_hands_off(gpu_ctx, tmp_path, as_reference):
    """A CSV batch straight into group_by and sort; nothing looks at the batch's columns first."""
    n = 300
    rng = np.random.default_rng(14)
    raw = [("i64", rng.integers(0, 7, n, dtype=np.int64), rng.random(n) > 0.1), ("f64", pc.dyadic_cells(14, n, pc.SCALE)[1], rng.random(n) > 0.2),
           ("str", [pc.WORDS[i % 6] for i in rng.integers(0, 6, n)], None), ("i64", rng.integers(-50, 50, n, dtype=np.int64), None)]
    src = {"how": "csv", "frame": pc._csv_frame(raw, as_reference), "padded": None, "pad": 0, "ref": as_reference, "text": pc._csv_text(raw)}
    for steps in ([{"kind": "group", "key": 0, "specs": [("count_rows", None), ("sum", 1), ("max", 3), ("count", 2)]}],
                  [{"kind": "sort", "keys": [(0, 2), (1, 1)], "via": "sort"}],
                  [{"kind": "group", "key": 2, "specs": [("count_rows", None), ("min", 0)]}, {"kind": "sort", "keys": [(2, 1)], "via": "chain"}]):
        model = pm.run(pm.source_of(src), steps)
        pd.run_pipeline(gpu_ctx, src, steps, {}, model, {}, False, f"csv as_reference={as_reference}", tmp_path)


@pytest.mark.parametrize("offset", [0, 65])
def test_looking_at_a_column_changes_nothing(gpu_ctx, offset):
    """rv_null_count caches its answer in the column it was asked about.  An uploaded nullable column (and a slice of one) starts without
    a count; after null_count() the column claims one, and that claim, a second answer and every consumer's result must be the model's."""
    n = ROWS
    rng = np.random.default_rng(15 + offset)
    total = n + offset + 3
    full = [("i64", rng.integers(0, 9, total, dtype=np.int64), rng.random(total) > 0.3), ("f64", pc.dyadic_cells(15, total, pc.SCALE)[1], rng.random(total) > 0.5),
            ("str", [pc.WORDS[i % 7] for i in range(total)], rng.random(total) > 0.2)]
    full[2] = ("str", [x if v else None for x, v in zip(full[2][1], full[2][2])], full[2][2])
    frame = [pc._cut(c, offset, n) for c in full]
    d = [gpu_ctx.upload(pd.to_host(c)).slice(offset, n) for c in full]
    for c, w in zip(d, frame):
        nulls = pm.null_count(w)
        assert c.info().null_count == -1, "an uploaded nullable column (or its slice) starts without a count"
        assert c.null_count() == nulls
        assert c.info().null_count == nulls, "the count the column now claims"
        assert c.null_count() == nulls
    build = [("i64", np.array([0, 4, 4, 8, 1], np.int64), np.array([1, 1, 1, 1, 0], bool)), ("f64", np.array([1.0, 2.0, 3.0, 4.0, 5.0]), None)]
    for steps, builds in (([{"kind": "group", "key": 0, "specs": [("count", 1), ("sum", 1), ("count", 2), ("min", 1)]}], {}),
                          ([{"kind": "group", "key": 2, "specs": [("count_rows", None), ("count", 0)]}], {}),
                          ([{"kind": "sort", "keys": [(0, 3), (1, 0)], "via": "chain"}], {}),
                          ([{"kind": "arith", "tree": ("/", ("col", 1), ("col", 0))}, {"kind": "mask", "terms": [(3, "<", 0.0)], "expr": ("not", 0)}], {}),
                          ([{"kind": "join", "probe_key": 0, "build_key": 0, "chunked": True}], {0: build}),
                          ([{"kind": "window", "partition_by": [0, 2], "order_by": [(1, 2)], "exprs": [("cum_count", 2), ("cum_sum", 1), ("cum_max", 0), ("lag", 2, 1)]}], {}),
                          ([{"kind": "topk", "keys": [(1, 0), (0, 3)], "k": ["of", 1, 8], "via": "frame", "select": True}], {}),
                          ([{"kind": "topk", "keys": [(0, 2)], "k": ["abs", 7], "via": "indices", "select": True}], {}),
                          ([{"kind": "outer_join", "how": "full", "probe_key": 0, "build_key": 0, "chunked": False, "side": "probe"}], {0: build}),
                          ([{"kind": "outer_join", "how": "anti", "probe_key": 0, "build_key": 0, "chunked": True, "side": "probe"}], {0: build}),
                          ([{"kind": "group_keys", "keys": [0, 2, 1], "specs": [("count_rows", None), ("sum", 1), ("min", 0), ("count", 2)]}], {})):
        want = frame
        got, rows = d, n
        for k, step in enumerate(steps):
            b = builds.get(k)
            got, rows = pd.run_step(gpu_ctx, step, got, rows, pm.dtypes(want), None if b is None else ([gpu_ctx.upload(pd.to_host(c)) for c in b], pm.rows(b)), want)
            want = pm.apply(step, want, b)
        diff = pm.frame_diff(pd.download(got), want)
        assert diff is None, f"{[s['kind'] for s in steps]} over inspected columns: {diff}"
