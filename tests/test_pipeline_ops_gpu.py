"""Window functions, top-k, outer / semi / anti joins and multi-key grouping inside operator pipelines on the device (-m gpu): each fed
columns another operator wrote and feeding the next, against the composed model of tests/pipeline_model.py, bit for bit, in both modes of
tests/test_pipeline_gpu.py (hands-off, inspected).  Every top-k call's account of itself (passes, candidates) is compared with
topk_model.select over the model's key column: that is what shows the radix select running over a key an operator made.

Random cases: pipeline_cases.case_ops(seed), RV_PIPELINE_OPS_CASES seeds (default 216, the set tests/test_pipeline_ops_cpu.py's
conditions are about).  Directed pipelines: pipeline_cases.DIRECTED_OPS, each at most 2 * TILE + 1 rows, and below them the identities
that no single step list expresses."""
import os

import numpy as np
import pytest

import pipeline_cases as pc
import pipeline_device as pd
import pipeline_model as pm
from rivulus_amd.capi import RV_JOIN_PROBE_ANTI, RV_JOIN_PROBE_OUTER, RV_JOIN_PROBE_SEMI
from test_pipeline_gpu import ROWS, _both_modes, _usable

pytestmark = pytest.mark.gpu
N_CASES = int(os.environ.get("RV_PIPELINE_OPS_CASES", pc.N_CASES_OPS))


@pytest.mark.parametrize("seed", range(N_CASES))
def test_random_pipeline_matches_model(gpu_ctx, tmp_path, seed):
    _both_modes(gpu_ctx, pc.case_ops(seed), tmp_path)


@pytest.mark.parametrize("name", pc.DIRECTED_OPS)
def test_directed_pipeline(gpu_ctx, name):
    """full_outer_then_<c>: the columns FULL_OUTER padded (0 under the null) as window partition / order key, top-k key under every flag
    word with k on either side of the null count, group_keys tuple, sort and group key, arith operands, probe key of a second join
    against key 0; window_minmax_<bitmap | plain>_then_<c>_<offset>: CUM_MIN / CUM_MAX outputs, null at every partition's start (plain:
    no null, the bitmap dropped), sliced at the offset and read as key or predicate column; topk_indices_as_index_<flags>: top_k_indices
    over a / b, then take_device, then a window over the k rows; empty_*: zero-row frames into and out of every new operator, and the
    context answers a query afterwards; bitmap_without_nulls_<c>: an attached bitmap without nulls on every column the consumer reads;
    null_columns_ride_along_ops: Null-dtype columns in every role the new operators give a column."""
    case = pc.directed_ops_case(name, ROWS)
    frame, model = _both_modes(gpu_ctx, case, what=name)
    pc.assert_point(name, case)
    if name.startswith("empty_"):
        assert [pm.DTYPE_OF_RV[c.info().dtype] for c in frame] == pm.dtypes(model[-1][0])
        assert all(c.info().length == pm.rows(model[-1][0]) for c in frame)
        _usable(gpu_ctx)


def _upload(ctx, frame):
    return [ctx.upload(pd.to_host(c)) for c in frame]


def _same(got, want, what):
    diff = pm.frame_diff(pd.download(got), want)
    assert diff is None, f"{what}: {diff}"


def test_row_number_inverts_the_sort(gpu_ctx):
    """rv_sort by two keys; ROW_NUMBER over the same order_by without a partition is every row's place in that order; row_number - 1,
    computed by rv_eval_arith, is an index list, and take_device(sorted frame, it) is the source frame again."""
    rng = np.random.default_rng(21)
    n = ROWS
    frame = [("i64", rng.integers(0, 9, n, dtype=np.int64), rng.random(n) > 0.2), ("f64", pc.dyadic_cells(21, n, pc.SCALE)[1] % 4.0, rng.random(n) > 0.1),
             ("str", [pc.WORDS[i % 7] for i in range(n)], None), ("bool", rng.random(n) > 0.5, rng.random(n) > 0.3)]
    keys = [(0, 3), (1, 1)]
    d = _upload(gpu_ctx, frame)
    ordered = gpu_ctx.sort(d, keys)
    number = gpu_ctx.window(d, [], keys, [("row_number", 0)])
    place = gpu_ctx.eval_arith(number, ("-", ("col", 0), ("lit", 1)))
    perm = pm.sort_model.sort_frame(pm.sort_columns(frame), keys)
    inverse = np.empty(n, np.int64)
    inverse[perm] = np.arange(n)
    _same([place], [("i64", inverse, None)], "row_number - 1")
    _same(ordered, pm.take_frame(frame, perm), "the sorted frame")
    _same(gpu_ctx.take_device(ordered, place), frame, "take_device(sorted frame, row_number - 1)")


def test_gids_as_partition_key(gpu_ctx):
    """rv_group_ids_keys' gids as the single partition key give the window columns partition_by = keys gives; MAX of ROW_NUMBER per group
    through hash_aggregate_keys is COUNT_ROWS."""
    rng = np.random.default_rng(22)
    n = ROWS
    frame = [("i64", rng.integers(0, 5, n, dtype=np.int64), rng.random(n) > 0.2), ("f64", rng.choice(np.array(pc.SPECIALS + (1.5,)), n), rng.random(n) > 0.2),
             ("bool", rng.random(n) > 0.5, rng.random(n) > 0.3), ("i64", rng.integers(-99, 99, n, dtype=np.int64), rng.random(n) > 0.1)]
    keys, order = [0, 1, 2], [(3, 1)]
    exprs = [("row_number", 0), ("rank", 0), ("cum_sum", 3), ("cum_min", 3), ("lag", 1, 1), ("cum_count", 2)]
    d = _upload(gpu_ctx, frame)
    gids, _, groups = gpu_ctx.group_ids_keys([d[j] for j in keys])
    want = pm.step_window(frame, {"partition_by": keys, "order_by": order, "exprs": exprs})[len(frame):]
    by_keys = gpu_ctx.window(d, keys, order, exprs)
    by_gids = gpu_ctx.window(d + [gids], [len(d)], order, exprs)
    _same(by_keys, want, "partition_by = keys")
    _same(by_gids, want, "partition_by = [gids]")
    res = pm.group_keys_result(frame, {"keys": keys, "specs": [("count_rows", None)]})
    assert groups == res["groups"] > 20
    outs, _, _ = gpu_ctx.hash_aggregate_keys([d[j] for j in keys], [by_gids[0]], [("max", 0), ("count_rows", None)])
    got = pd.download(outs[len(keys):])
    assert pm.column_diff(got[0], got[1]) is None, "MAX(row_number) per group is the group's row count"
    assert pm.column_diff(got[1], pm.agg_columns(res["aggs"])[0]) is None


def test_lag_of_strings_into_dictionary_join(gpu_ctx):
    """LAG(String, 1) over a partitioned frame, sliced at offset 1 (nulls at the partition heads; its first offset is then not 0), into
    string_dict_build; the ids, and the encoding of an uploaded String column, as the keys of a PROBE_OUTER join."""
    rng = np.random.default_rng(23)
    n = ROWS
    frame = [("i64", rng.integers(0, 40, n, dtype=np.int64), None), ("str", [None if i % 11 == 3 else pc.WORDS[i % 8] + str(i % 3) for i in rng.integers(0, 90, n)], None)]
    frame[1] = ("str", frame[1][1], np.array([x is not None for x in frame[1][1]], bool))
    d = _upload(gpu_ctx, frame)
    lagged = gpu_ctx.window(d, [0], [], [("lag", 1, 1)])[0].slice(1, n - 1)
    want = pm.take_col(pm.step_window(frame, {"partition_by": [0], "order_by": [], "exprs": [("lag", 1, 1)]})[2], np.arange(1, n))
    assert pm.null_count(want) > 40
    _same([lagged], [want], "LAG(String, 1) sliced at 1")
    sdict, ids = gpu_ctx.string_dict_build(lagged)
    want_ids = pm.string_ids(want)
    _same([ids], [want_ids], "string_dict_build over the sliced LAG column")
    other = ("str", ["Bob0", "zz1", None, "absent", "a0", "Bob0"], np.array([1, 1, 0, 1, 1, 1], bool))
    first = {x: i for i, x in reversed(list(enumerate(want[1]))) if pm.valid_of(want)[i]}
    codes = pm.column_of("i64", [None if x is None else first.get(x, -1) for x in other[1]])
    encoded = sdict.encode(gpu_ctx.upload(pd.to_host(other)))
    _same([encoded], [codes], "encode: the string's id, -1 for an absent string, null under a null")
    payload = ("i64", np.arange(6, dtype=np.int64), None)
    outs, rows = gpu_ctx.hash_join([encoded, gpu_ctx.upload(pd.to_host(payload))], 0, [ids, lagged], 0, kind=RV_JOIN_PROBE_OUTER)
    step = {"kind": "outer_join", "how": "outer", "probe_key": 0, "build_key": 0, "side": "probe"}
    model = pm.step_outer_join([want_ids, want], step, [codes, payload])
    assert rows == pm.rows(model) > n
    _same(outs, model, "PROBE_OUTER over dictionary ids")
    sdict.free()


def test_semi_plus_anti_is_the_probe_frame(gpu_ctx):
    """PROBE_SEMI and PROBE_ANTI over the same a / b probe key (null quotients beside genuine 0) against a build side with a null key:
    the two outputs, concatenated and sorted by an uploaded row-number column, are the probe frame."""
    n = ROWS
    frame = pc._div_frame(n, 24) + [("i64", np.arange(n, dtype=np.int64), None)]
    d = _upload(gpu_ctx, frame)
    d.append(gpu_ctx.eval_arith(d, pm.tup(pc.DIV["tree"])))
    probe = pm.step_arith(frame, pc.DIV)
    build = [("i64", np.array([0, 3, 0, -2, 7], np.int64), np.array([1, 1, 1, 1, 0], bool))]
    b = _upload(gpu_ctx, build)
    parts = []
    for kind, how in ((RV_JOIN_PROBE_SEMI, "semi"), (RV_JOIN_PROBE_ANTI, "anti")):
        outs, rows = gpu_ctx.hash_join(b, 0, d, 4, kind=kind)
        want = pm.step_outer_join(probe, {"how": how, "probe_key": 4, "build_key": 0, "side": "probe"}, build)
        assert rows == pm.rows(want) > n // 8, how
        _same(outs, want, how)
        parts.append(outs)
    q = probe[4]
    assert pm.null_count(q) > 0 and (q[1][pm.valid_of(q)] == 0).any() and len(parts[0]) == len(parts[1]) == len(probe)
    both = [gpu_ctx.concat([x, y]) for x, y in zip(*parts)]
    _same(gpu_ctx.sort(both, [(3, 0)]), probe, "semi ++ anti, sorted by the row number")
