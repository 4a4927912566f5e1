"""rv_eval_arith on the device against the model (tests/arith_model.py), cell by cell: valid flags, the bits of valid cells, 0 under
nulls, null_count and whether a bitmap is attached.  Sizes round a lane, a bitmap word, a workgroup and one sweep of the capped
grid; inputs sliced at unaligned bit offsets; every operator over every type pair and operand form on the edge cells."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import arith_model as M
from rivulus_amd import capi
from rivulus_amd.capi import (RV_BOOLEAN, RV_ERR_INVALID_ARG, RV_ERR_LENGTH_MISMATCH, RV_ERR_TYPE_MISMATCH, RV_ERR_UNSUPPORTED, RV_FLOAT64,
                              RV_INT64, RV_NULL, Column)

pytestmark = pytest.mark.gpu

NAN_BITS = M.f64_bits(math.nan)
GARBAGE = {RV_INT64: 0x5555555555555555, RV_FLOAT64: math.nan}  # what lies under a null input cell: it must never show


def host_column(dtype, cells, bitmap=None):
    """Column of `cells` (None for null).  bitmap: attach a validity bitmap (default: iff there is a null)."""
    if dtype == RV_NULL:
        return Column.nulls(len(cells))
    np_dtype = np.int64 if dtype == RV_INT64 else np.float64
    values = np.array([GARBAGE[dtype] if c is None else c for c in cells], dtype=np_dtype)
    valid = np.array([c is not None for c in cells], dtype=bool)
    if bitmap is None:
        bitmap = not valid.all()
    return Column.from_numpy(values, valid if bitmap else None)


def device_column(ctx, dtype, cells, bitmap=None, offset=0):
    """The column on the device; offset > 0: as a slice at that element offset of a longer upload (its first cells are fillers)."""
    filler = [None if (bitmap or any(c is None for c in cells)) and k % 3 == 0 else (1 if dtype == RV_INT64 else 1.0) for k in range(offset)]
    if dtype == RV_NULL:
        filler = [None] * offset
    has_bitmap = bitmap if bitmap is not None else any(c is None for c in cells)
    col = ctx.upload(host_column(dtype, filler + list(cells), has_bitmap))
    return col.slice(offset, len(cells)) if offset else col


def check_output(out, dtype, cells, want_bitmap, what=""):
    info = out.info()
    assert info.dtype == dtype and info.length == len(cells) and info.offset == 0, what
    assert bool(info.has_validity) == want_bitmap, f"{what}: bitmap attached {bool(info.has_validity)}, expected {want_bitmap}"
    assert info.null_count == sum(c is None for c in cells), f"{what}: null_count {info.null_count}"
    if dtype == RV_NULL:
        return
    got = out.download()
    valid = got.logical_valid()
    valid = np.ones(len(cells), bool) if valid is None else valid
    want_valid = np.array([c is not None for c in cells], dtype=bool)
    assert np.array_equal(valid, want_valid), f"{what}: valid flags differ first at row {int(np.flatnonzero(valid != want_valid)[0])}"
    bits = got.values.view(np.uint64).copy()
    if dtype == RV_FLOAT64:
        bits[np.isnan(got.values)] = NAN_BITS  # NaN-ness is kept, payloads are not specified
    want = np.array([M.cell_bits(dtype, c) for c in cells], dtype=np.uint64)
    if not np.array_equal(bits, want):
        i = int(np.flatnonzero(bits != want)[0])
        raise AssertionError(f"{what}: row {i}: {int(bits[i]):#018x} != {int(want[i]):#018x}")


def run_and_check(ctx, tree, dtypes, columns, bitmaps=None, offsets=None, what=""):
    """Evaluate `tree` over device copies of `columns` and compare with the model; returns the output column."""
    k = len(columns)
    bitmaps = bitmaps or [None] * k
    offsets = offsets or [0] * k
    dev = [device_column(ctx, dtypes[j], columns[j], bitmaps[j], offsets[j]) for j in range(k)]
    has = [bool(d.info().has_validity) for d in dev]
    out = ctx.eval_arith(dev, tree)
    dtype, cells = M.evaluate(tree, dtypes, columns)
    check_output(out, dtype, cells, M.bitmap_expected(tree, dtypes, has), what)
    return out


def random_cells(rng, dtype, n, nulls):
    if dtype == RV_INT64:
        small = rng.integers(-50, 50, n)
        wide = rng.integers(M.I64_MIN, M.I64_MAX, n, dtype=np.int64, endpoint=True)
        cells = [int(x) for x in np.where(rng.random(n) < 0.5, small, wide)]
    else:
        cells = [float(x) for x in (rng.random(n) - 0.5) * 1e6]
    if nulls:
        for i in np.flatnonzero(rng.random(n) < 0.2):
            cells[int(i)] = None
    return cells


# ---- sizes, offsets, null patterns ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 4097])
def test_sizes_offsets_and_null_patterns(gpu_ctx, n):
    rng = np.random.default_rng(1000 + n)
    trees = [(("*", ("+", ("col", 0), ("col", 1)), ("lit", 3)), [RV_INT64, RV_INT64]),
             (("-", ("col", 0), ("/", ("col", 1), ("lit", 4.0))), [RV_FLOAT64, RV_INT64])]
    for (tree, dtypes), offset, (nulls_a, nulls_b) in itertools.product(trees, [0, 1, 63, 65], [(False, False), (True, False), (True, True)]):
        cols = [random_cells(rng, dtypes[0], n, nulls_a), random_cells(rng, dtypes[1], n, nulls_b)]
        # the two inputs sit at DIFFERENT bit offsets: their validity words are gathered independently
        run_and_check(gpu_ctx, tree, dtypes, cols, bitmaps=[nulls_a, nulls_b], offsets=[offset, (offset * 2) % 67],
                      what=f"n={n} offset={offset} nulls={nulls_a, nulls_b} {dtypes}")


def test_more_rows_than_one_sweep_of_the_grid(gpu_ctx):
    """2^20 + 77 rows: the capped grid is 2048 workgroups of 256 lanes, 524 288 lanes; arith_kernel<2> takes two rows per lane, so
    one sweep covers 2^20 rows and the grid-stride loop runs a second time for the rest (a kernel with one row per lane: a third)."""
    n = (1 << 20) + 77
    rng = np.random.default_rng(7)
    a = rng.integers(M.I64_MIN, M.I64_MAX, n, dtype=np.int64, endpoint=True)
    b = rng.integers(M.I64_MIN, M.I64_MAX, n, dtype=np.int64, endpoint=True)
    valid_b = rng.random(n) >= 0.1
    da = gpu_ctx.upload(Column.from_numpy(np.concatenate([[5], a]))).slice(1, n)
    db = gpu_ctx.upload(Column.from_numpy(b, valid_b))
    tree = ("+", ("col", 0), ("col", 1))
    out = gpu_ctx.eval_arith([da, db], tree)
    cells_b = [int(x) if ok else None for x, ok in zip(b.tolist(), valid_b.tolist())]
    dtype, cells = M.evaluate(tree, [RV_INT64, RV_INT64], [a.tolist(), cells_b])
    check_output(out, dtype, cells, True, "2^20 + 77 rows")
    assert gpu_ctx.last_kernel() == "arith_kernel<2>"


@pytest.mark.parametrize("ncols,n,kernel", [(3, (1 << 20) + 77, "arith_kernel<4>"), (5, (1 << 19) + 3 * 64 + 5, "arith_kernel<8>")])
def test_the_wider_kernels_stride_on_too(gpu_ctx, ncols, n, kernel):
    """The same past one sweep of arith_kernel<4> (two rows per lane: 2^20 rows) and of arith_kernel<8> (one: 2^19), which a
    program takes for its columns: c0 + c1 + ... left to right, Int64 with one nullable input."""
    rng = np.random.default_rng(ncols)
    arrays = [rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64) for _ in range(ncols)]
    valid = rng.random(n) >= 0.1
    dev = [gpu_ctx.upload(Column.from_numpy(a, valid if j == 1 else None)) for j, a in enumerate(arrays)]
    tree = ("col", 0)
    for j in range(1, ncols):
        tree = ("+", tree, ("col", j))
    out = gpu_ctx.eval_arith(dev, tree)
    assert gpu_ctx.last_kernel() == kernel
    columns = [a.tolist() for a in arrays]
    columns[1] = [x if ok else None for x, ok in zip(columns[1], valid.tolist())]
    dtype, cells = M.evaluate(tree, [RV_INT64] * ncols, columns)
    check_output(out, dtype, cells, True, kernel)


# ---- operators, types, operand forms --------------------------------------------------------------------------------------
EDGES = {RV_INT64: M.INT_EDGES, RV_FLOAT64: M.FLOAT_EDGES}
LITERALS = {RV_INT64: [0, 1, -1, M.I64_MIN, M.I64_MAX, (1 << 53) + 1, 7], RV_FLOAT64: [0.0, -0.0, math.inf, math.nan, 5e-324, 1.5, 1e200]}


@pytest.mark.parametrize("left,right", [(RV_INT64, RV_INT64), (RV_FLOAT64, RV_FLOAT64), (RV_INT64, RV_FLOAT64), (RV_FLOAT64, RV_INT64)])
def test_every_operator_on_the_edge_cells(gpu_ctx, left, right):
    ctx = gpu_ctx
    pairs = list(itertools.product(EDGES[left] + [None], EDGES[right] + [None]))  # every edge against every edge, and against a null
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    da, db = device_column(ctx, left, a), device_column(ctx, right, b)
    ea, eb = device_column(ctx, left, EDGES[left] + [None]), device_column(ctx, right, EDGES[right] + [None])
    for op in "+-*/":
        tree = (op, ("col", 0), ("col", 1))
        dtype, cells = M.evaluate(tree, [left, right], [a, b])
        check_output(ctx.eval_arith([da, db], tree), dtype, cells, True, f"col {op} col")
        for lit in LITERALS[right]:
            tree = (op, ("col", 0), ("lit", lit))
            dtype, cells = M.evaluate(tree, [left], [EDGES[left] + [None]])
            check_output(ctx.eval_arith([ea], tree), dtype, cells, True, f"col {op} lit {lit!r}")
        for lit in LITERALS[left]:
            tree = (op, ("lit", lit), ("col", 0))
            dtype, cells = M.evaluate(tree, [right], [EDGES[right] + [None]])
            check_output(ctx.eval_arith([eb], tree), dtype, cells, True, f"lit {lit!r} {op} col")


def test_contraction_witness_on_the_device(gpu_ctx):
    """(a * b) + c, a = 1 + 2^-30, b = 1 - 2^-30, c = -1: exactly +0.0 with two roundings, -2^-60 from a fused multiply-add."""
    a, b, c = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0
    n = 130
    tree = ("+", ("*", ("col", 0), ("col", 1)), ("col", 2))
    out = run_and_check(gpu_ctx, tree, [RV_FLOAT64] * 3, [[a] * n, [b] * n, [c] * n], what="witness")
    assert out.download().values.view(np.uint64).tolist() == [0] * n
    assert gpu_ctx.last_kernel() == "arith_kernel<4>"  # two entries deep, but three columns
    # the same with the multiply as the right operand (three entries deep) and the addend a literal (two columns, two entries)
    run_and_check(gpu_ctx, ("+", ("col", 2), ("*", ("col", 0), ("col", 1))), [RV_FLOAT64] * 3, [[a] * n, [b] * n, [c] * n], what="witness, right")
    assert gpu_ctx.last_kernel() == "arith_kernel<4>"
    out = run_and_check(gpu_ctx, ("+", ("*", ("col", 0), ("col", 1)), ("lit", c)), [RV_FLOAT64] * 2, [[a] * n, [b] * n], what="witness, literal")
    assert out.download().values.view(np.uint64).tolist() == [0] * n
    assert gpu_ctx.last_kernel() == "arith_kernel<2>"


def test_division_by_zero_inside_a_deeper_expression(gpu_ctx):
    """A null made by an inner Int64 division stays null through the operators above it; without a nullable input the bitmap is
    attached for the division alone."""
    a, b, c = [10, 11, 12, -9, 5], [2, 0, 3, 0, 1], [1, 2, 0, 4, 5]
    tree = ("+", ("*", ("/", ("col", 0), ("col", 1)), ("col", 2)), ("/", ("col", 0), ("col", 2)))
    out = run_and_check(gpu_ctx, tree, [RV_INT64] * 3, [a, b, c], what="inner division")
    assert out.info().null_count == 3
    out = run_and_check(gpu_ctx, ("/", ("col", 0), ("lit", 1)), [RV_INT64], [a], what="no zero divisor")  # still a bitmap, no null
    assert out.info().has_validity and out.info().null_count == 0
    run_and_check(gpu_ctx, ("/", ("col", 0), ("lit", 0)), [RV_INT64], [a], what="literal zero divisor")  # all null, by the kernel
    assert gpu_ctx.last_kernel() == "arith_kernel<2>"
    run_and_check(gpu_ctx, ("/", ("col", 0), ("lit", 0.0)), [RV_INT64], [a], what="float zero divisor")  # +-inf, never null


# ---- program shape ---------------------------------------------------------------------------------------------------------
def _limit_columns(rng, n):
    dtypes = [RV_INT64, RV_FLOAT64, RV_INT64, RV_INT64, RV_FLOAT64, RV_INT64, RV_FLOAT64, RV_INT64]
    return dtypes, [random_cells(rng, d, n, nulls=(j % 3 == 0)) for j, d in enumerate(dtypes)]


def test_a_program_at_the_limits(gpu_ctx):
    """Eight distinct columns, the operand stack eight deep, and 31 steps: a well-formed postfix program of binary operators has
    an odd number of steps (L leaves and L - 1 operators), so 31 is the longest one inside the limit of 32."""
    rng = np.random.default_rng(31)
    dtypes, cols = _limit_columns(rng, 333)
    steps = [("col", j) for j in range(8)]  # depth 8
    steps += ["*", "+", "-", "+", "/", "-", "+"]  # 15 steps, depth 1
    for j in range(8):  # 16 more: 31
        steps += [("col", j) if j % 2 else ("lit", 3 if j % 4 else 2.5), "+-*/"[j % 4]]
    assert len(steps) == 31
    stack = []
    for s in steps:  # the tree of the step list, for the model
        if isinstance(s, str):
            b, a = stack.pop(), stack.pop()
            stack.append((s, a, b))
        else:
            stack.append(s)
    (tree,) = stack
    assert capi.arith_postfix(tree) == steps
    dev = [device_column(gpu_ctx, dtypes[j], cols[j]) for j in range(8)]
    out = gpu_ctx.eval_arith(dev, steps)
    dtype, cells = M.evaluate(tree, dtypes, cols)
    assert dtype == RV_FLOAT64
    check_output(out, dtype, cells, True, "31 steps, depth 8, 8 columns")
    assert gpu_ctx.last_kernel() == "arith_kernel<8>"


def _unsupported(ctx, dev, steps):
    with pytest.raises(capi.RvError) as e:
        ctx.eval_arith(dev, steps)
    assert e.value.status == RV_ERR_UNSUPPORTED, e.value
    return e.value.message


def test_one_past_each_limit_is_unsupported(gpu_ctx):
    ctx = gpu_ctx
    dev = [device_column(ctx, RV_INT64, [j, j + 1, j + 2]) for j in range(9)]
    ok = [("col", 0), ("col", 1), "+"]
    # 33 steps: 17 leaves, depth 2
    steps = [("col", 0)]
    for j in range(16):
        steps += [("col", j % 8), "+"]
    assert len(steps) == 33 and "steps" in _unsupported(ctx, dev, steps)
    assert ctx.eval_arith(dev, ok).download().values.tolist() == [1, 3, 5]
    # a stack of nine
    steps = [("col", j % 8) for j in range(9)] + ["+"] * 8
    assert "stack" in _unsupported(ctx, dev, steps)
    assert ctx.eval_arith(dev, ok).download().values.tolist() == [1, 3, 5]
    # nine distinct columns, depth 2
    steps = [("col", 0)]
    for j in range(1, 9):
        steps += [("col", j), "+"]
    assert "columns" in _unsupported(ctx, dev, steps)
    assert ctx.eval_arith(dev, ok).download().values.tolist() == [1, 3, 5]
    # ... and exactly at them: 8 distinct columns, and the same column any number of times
    assert ctx.eval_arith(dev, steps[:-2]).download().values.tolist() == [28, 36, 44]


def test_every_error_leaves_the_context_usable(gpu_ctx):
    ctx, lib = gpu_ctx, capi.load()
    i3, i4 = device_column(ctx, RV_INT64, [1, 2, 3]), device_column(ctx, RV_INT64, [1, 2, 3, 4])
    boolean = ctx.upload(Column.from_numpy(np.array([True, False, True])))
    string = ctx.upload(Column.from_strings(["a", "b", "c"]))
    plus = [("col", 0), ("col", 1), "+"]

    def still_works():
        out = ctx.eval_arith([i3, i3], plus)
        assert out.download().values.tolist() == [2, 4, 6]

    def fails(cols, steps, status):
        with pytest.raises(capi.RvError) as e:
            ctx.eval_arith(cols, steps)
        assert e.value.status == status, e.value
        assert e.value.message
        still_works()

    # NULL arguments
    arr, handles, out = capi.arith_steps(plus), capi._handles([i3, i3]), C.c_void_p()
    for args in [(None, handles, 2, arr, 3, C.byref(out)), (ctx.handle, None, 2, arr, 3, C.byref(out)), (ctx.handle, handles, 2, None, 3, C.byref(out)),
                 (ctx.handle, handles, 2, arr, 3, None)]:
        assert lib.rv_eval_arith(*args) == RV_ERR_INVALID_ARG
        still_works()
    # malformed programs
    fails([i3], [("col", 0), "+"], RV_ERR_INVALID_ARG)                       # an operator with one operand
    fails([i3], ["+"], RV_ERR_INVALID_ARG)
    fails([i3, i3], [("col", 0), ("col", 1)], RV_ERR_INVALID_ARG)            # two values left
    fails([i3], [("lit", 1), ("lit", 2), "+"], RV_ERR_INVALID_ARG)           # no column read
    fails([i3], [], RV_ERR_INVALID_ARG)
    bad = capi.arith_steps(plus)
    bad[2].op = 9                                                            # an unknown step
    assert lib.rv_eval_arith(ctx.handle, handles, 2, bad, 3, C.byref(out)) == RV_ERR_INVALID_ARG and not out.value
    still_works()
    fails([i3, i3], [("col", 0), ("col", 2), "+"], RV_ERR_INVALID_ARG)       # a column index >= ncols
    fails([i3, i4], plus, RV_ERR_LENGTH_MISMATCH)
    fails([i3, boolean], plus, RV_ERR_TYPE_MISMATCH)
    fails([i3, string], plus, RV_ERR_TYPE_MISMATCH)
    fails([i3], [("col", 0), ("lit", True), "+"], RV_ERR_TYPE_MISMATCH)
    fails([i3], [("col", 0), ("lit", "x"), "+"], RV_ERR_TYPE_MISMATCH)
    # a column the program does not read may be anything, of any length
    assert ctx.eval_arith([i3, string, i4], [("col", 0), ("lit", 1), "+"]).download().values.tolist() == [2, 3, 4]


# ---- all-null results --------------------------------------------------------------------------------------------------------
def test_null_leaves_make_every_cell_null_without_a_kernel(gpu_ctx):
    ctx = gpu_ctx
    n = 70
    ints, floats = list(range(n)), [float(k) for k in range(n)]
    cases = [(("+", ("col", 0), ("col", 1)), [RV_NULL, RV_INT64], [[None] * n, ints], RV_INT64),
             (("*", ("col", 1), ("col", 0)), [RV_NULL, RV_FLOAT64], [[None] * n, floats], RV_FLOAT64),
             (("-", ("col", 0), ("lit", None)), [RV_FLOAT64], [floats], RV_FLOAT64),
             (("/", ("lit", None), ("col", 0)), [RV_INT64], [ints], RV_INT64),
             (("+", ("*", ("col", 0), ("lit", 2.0)), ("col", 1)), [RV_INT64, RV_NULL], [ints, [None] * n], RV_FLOAT64),
             (("+", ("col", 0), ("col", 1)), [RV_NULL, RV_NULL], [[None] * n, [None] * n], RV_NULL),
             (("+", ("col", 0), ("lit", None)), [RV_NULL], [[None] * n], RV_NULL)]
    for tree, dtypes, cols, want in cases:
        run_and_check(ctx, ("+", ("col", 0), ("lit", 1)), [RV_INT64], [ints])  # a kernel runs ...
        assert ctx.last_kernel() == "arith_kernel<2>"
        out = run_and_check(ctx, tree, dtypes, cols, what=str(tree))             # ... and here none does
        assert ctx.last_kernel() == "arith_all_null"
        assert out.info().dtype == want and out.info().null_count == n
    # types are still checked under a Null leaf
    with pytest.raises(capi.RvError) as e:
        ctx.eval_arith([ctx.upload(Column.nulls(3))], [("col", 0), ("lit", True), "+"])
    assert e.value.status == RV_ERR_TYPE_MISMATCH


def test_the_same_call_twice_gives_the_same_bytes(gpu_ctx):
    rng = np.random.default_rng(99)
    n = 5000
    a = device_column(gpu_ctx, RV_FLOAT64, random_cells(rng, RV_FLOAT64, n, True))
    b = device_column(gpu_ctx, RV_INT64, [int(x) for x in rng.integers(-3, 4, n)])
    tree = ("/", ("-", ("col", 0), ("col", 0)), ("/", ("col", 1), ("col", 1)))  # NaNs (0.0 / ...), nulls (x / 0), values
    one, two = gpu_ctx.eval_arith([a, b], tree).download(), gpu_ctx.eval_arith([a, b], tree).download()
    assert one.values.tobytes() == two.values.tobytes() and one.validity.tobytes() == two.validity.tobytes()
    assert 0 < one.logical_valid().sum() < n
