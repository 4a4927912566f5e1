"""Window frames over device-produced columns: the output of rv_filter_project and of rv_eval_arith, sliced, go into rv_window_frames as
partition key, order key and value columns -- buffers the library allocated itself, with its own padding, bitmaps and element offsets --
and the results equal tests/window_frame_model.py over the same rows computed on the host."""
import numpy as np
import pytest

import window_frame_model as F
from rivulus_amd import capi
from rivulus_amd.capi import Predicate, Term
from test_window_gpu import TILE, compare, f64, garbage_under_nulls, i64, upload

pytestmark = pytest.mark.gpu

EXPRS = [("sum", 2, 6, 0), ("avg", 3, 6, 0), ("sum", 4, None, None), ("min", 3, 2, -1), ("max", 4, -1, None), ("count", 3, 70, 70), ("first_value", 4, 1, 0),
         ("last_value", 2, 0, 65), ("ntile", 0, 4), ("row_number", 0), ("cum_sum", 4)]


@pytest.fixture(scope="module")
def ctx():
    with capi.Context(0) as c:
        yield c


def rows_of(col, keep):
    dtype, values, valid = col
    return dtype, values[keep], None if valid is None else valid[keep]


@pytest.mark.parametrize("offset", [0, 1, 65])
def test_frames_over_filtered_and_computed_columns(ctx, offset):
    n = 3 * TILE + 17
    rng = np.random.default_rng(40 + offset)
    table = [i64(rng.integers(0, 7, n)), i64(rng.integers(-20, 20, n), rng.random(n) >= 0.1), garbage_under_nulls(i64(rng.integers(-1000, 1000, n), rng.random(n) >= 0.2)),
             garbage_under_nulls(f64(rng.integers(-500, 500, n).astype(np.float64), rng.random(n) >= 0.2)), i64(rng.integers(0, 100, n))]
    devs = [upload(ctx, c) for c in table]
    # filter(gate > 29): about seven rows in ten survive; every column is a fresh device buffer with its own bitmap
    outs, rows, _ = ctx.filter_project(devs, Predicate([Term(4, ">", 29)]), [0, 1, 2, 3])
    keep = table[4][1] > 29
    assert rows == int(keep.sum()) > TILE
    host = [rows_of(c, keep) for c in table[:4]]
    # a computed value column: 2 * x + 1, null where x is
    outs.append(ctx.eval_arith(outs, ("+", ("*", ("col", 2), ("lit", 2)), ("lit", 1))))
    host.append(("i64", host[2][1] * 2 + 1, host[2][2]))
    m = rows - offset
    sliced = [c.slice(offset, m) if offset else c for c in outs]
    host = [rows_of(c, np.arange(rows) >= offset) for c in host]
    for part, order in (([0], [(1, 2)]), ([], [])):
        want = F.window_frames(host, part, order, EXPRS, exact_float=True, fast=True)
        got = ctx.window_frames(sliced, part, order, EXPRS)
        for e, g, w in zip(EXPRS, got, want):
            compare(g, w, f"{e} over filtered / computed columns sliced at {offset}, partition {part}")
        assert ctx.last_kernel() == "window_frame"
