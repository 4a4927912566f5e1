"""Float64 SUM of rv_filter_agg / rv_group_filter_agg, checked exactly (-m gpu).

Every cell is k * 2^s with integer |k| < 2^20 (helpers.dyadic_cells; premise and teeth of the compare: test_agg_exact_cpu.py), so
a sum has ONE correct bit pattern whatever the reduction tree, and it comes from integer arithmetic over the host arrays --
never from a GPU output.  The oracle must give the same bits.  Every case names the filter_agg_kernel instantiation it expects,
so a launch that silently took another path fails.  NaN, +inf, -inf and 1e300 lie under every null cell: they must not leak.
The one tolerance in this file is the derived bound of test_general_data_within_the_derived_bound."""
import math

import numpy as np
import pytest

from helpers import (AGG_CASES, AGG_F, AGG_R, DYADIC_SCALES, NULL_FILL, agg_case, agg_expected, agg_kernel_name, agg_sizes,
                     dyadic_cells, dyadic_sum, host_survivors, same_float)
from rivulus_amd import capi
from rivulus_amd.capi import RV_INT64, Column, Predicate, Term, synth_spec

pytestmark = pytest.mark.gpu


class _options:
    """Context options for the length of a with block; back to the defaults afterwards."""

    def __init__(self, ctx, **values):
        self.ctx, self.values = ctx, values

    def __enter__(self):
        for key, v in self.values.items():
            self.ctx.set_option(key, v)

    def __exit__(self, *exc):
        for key in self.values:
            self.ctx.set_option(key, 0)


def _assert_exact(ctx, oracle, cols, k, scale, pred, agg, kernel, what, dcols=None, ask_oracle=True, expected=None):
    """One launch: the expected kernel, the numpy count, the integer-derived sum bit for bit, and the oracle's bits."""
    want, want_count = expected or agg_expected(cols, k, scale, pred, agg)
    _, got, count = ctx.filter_agg(dcols if dcols is not None else [ctx.upload(c) for c in cols], pred, agg)
    assert ctx.last_kernel() == kernel, what
    assert count == want_count, what
    assert same_float(got, want), f"{what}: got {got!r} ({got.hex()}), the cells sum to {want!r} ({want.hex()})"
    if ask_oracle:
        _, osum, ocount = oracle.filter_agg(cols, pred, agg)
        assert ocount == want_count and same_float(osum, want), f"{what}: the oracle has {osum!r}"
    return got


def _policies(case):
    if case == "plain1":
        return ["drops"]  # no null anywhere
    if case == "boolean1":
        return ["drops"]  # is_true has no ordering to apply to a null
    return ["drops", "least"]


_VARIANTS = [c for c in AGG_CASES if c != "cols5"]


@pytest.mark.parametrize("vec", [1, 2])
@pytest.mark.parametrize("case,n", [(c, n) for c in _VARIANTS for n in agg_sizes(AGG_CASES[c][0])])
def test_every_variant_sums_exactly(gpu_ctx, oracle, case, n, vec):
    """filter_agg_kernel<1,16,v,4,0>, <1,16,v,4,F> (nullable aggregated column; Boolean is_true term), <2,8,v,4,F>, <3,4,v,4,F>,
    <4,4,v,4,F>, v = 1 and 2, at row counts round a lane, a wave and the variant's tile, at all three scales, under both null
    policies where a column is nullable.  The aggregated column has the highest index; the predicate reads the others (a
    launch with one 8-byte column and no Boolean has nothing else to test)."""
    ncols, flags, _ = AGG_CASES[case]
    kernel = agg_kernel_name(ncols, vec, flags)
    with _options(gpu_ctx, vec=vec):
        for scale in DYADIC_SCALES:
            for nulls in _policies(case):
                cols, k, pred, agg = agg_case(case, n, scale, seed=1000 + n, nulls=nulls)
                _assert_exact(gpu_ctx, oracle, cols, k, scale, pred, agg, kernel, f"{case} n={n} vec={vec} scale={scale} nulls={nulls}")


@pytest.mark.parametrize("case", ["plain1", "nullable1", "cols3"])
@pytest.mark.parametrize("n", [65, 4097, 8193])
def test_unaligned_slice_forces_vec1(gpu_ctx, oracle, case, n):
    """Rows [1, n + 1) of columns whose first row is 16-byte aligned start at an odd multiple of 8 bytes: 8-byte loads even where
    option "vec" asks for 16 (and the validity bits start at bit 1 of their word)."""
    ncols, flags, _ = AGG_CASES[case]
    for scale in DYADIC_SCALES:
        whole, k, pred, agg = agg_case(case, n + 1, scale, seed=2000 + n, nulls="least" if case != "plain1" else "drops")
        cols = [c.slice(1, n) for c in whole]
        for vec in (0, 2):
            with _options(gpu_ctx, vec=vec):
                dcols = [gpu_ctx.upload(c).slice(1, n) for c in whole]
                _assert_exact(gpu_ctx, oracle, cols, k[1:], scale, pred, agg, agg_kernel_name(ncols, 1, flags),
                              f"slice {case} n={n} scale={scale} vec option {vec}", dcols)
        # the aligned whole, default options: 16-byte loads for one column, 8-byte loads for several
        _assert_exact(gpu_ctx, oracle, whole, k, scale, pred, agg, agg_kernel_name(ncols, 2 if ncols == 1 else 1, flags),
                      f"whole {case} n={n + 1} scale={scale}")


@pytest.mark.parametrize("vec", [1, 2])
@pytest.mark.parametrize("nulls", ["drops", "least"])
def test_or_not_tree_with_strict_nullable_columns(gpu_ctx, oracle, nulls, vec):
    """(NOT a) OR (b AND NOT c) over two nullable Int64 columns: under "drops" a null in either column drops the row (strict
    operators), under "least" it orders lowest.  Three 8-byte columns either way."""
    for n in (65, 1025, 5000):
        cols, k, _, agg = agg_case("cols3", n, -10, seed=3000 + n)
        pred = Predicate([Term(0, "<", 70), Term(1, ">=", 15), Term(0, "==", 5)], nulls, ("or", ("not", 0), ("and", 1, ("not", 2))))
        with _options(gpu_ctx, vec=vec):
            _assert_exact(gpu_ctx, oracle, cols, k, -10, pred, agg, agg_kernel_name(3, vec, AGG_F), f"tree n={n} nulls={nulls} vec={vec}")


@pytest.mark.parametrize("vec", [1, 2])
@pytest.mark.parametrize("n", [1, 65, 4097, 20_011])
def test_more_columns_than_a_pass_reads(gpu_ctx, oracle, n, vec):
    """Aggregated column + four Int64 predicate columns: the predicate goes into a selection bitmap first, the aggregate reads
    that as a Boolean is_true term next to its one column."""
    for scale in DYADIC_SCALES:
        for nulls in ("drops", "least"):
            cols, k, pred, agg = agg_case("cols5", n, scale, seed=4000 + n, nulls=nulls)
            with _options(gpu_ctx, vec=vec):
                _assert_exact(gpu_ctx, oracle, cols, k, scale, pred, agg, agg_kernel_name(1, vec, AGG_F),
                              f"five columns n={n} scale={scale} nulls={nulls} vec={vec}")


def test_grid_stride_and_every_grid_give_the_same_bits(gpu_ctx, oracle):
    """agg_grid = 1: one workgroup per CU, each with two or three 1024-row tiles of the three-column variant (lanes accumulate
    across tiles) and a ragged last tile.  One workgroup per tile (-1), the default constant grid (0) and a grid request
    beyond the tile count (the min) add in other orders: identical bits all the same, the integer-derived ones."""
    cus = gpu_ctx.device_info()["compute_units"]
    n = (2 * cus + 1) * 1024 + 65
    kernel = agg_kernel_name(3, 1, AGG_F)
    for scale in DYADIC_SCALES:
        cols, k, pred, agg = agg_case("cols3", n, scale, seed=5000, nulls="least")
        dcols = [gpu_ctx.upload(c) for c in cols]
        try:
            sums = []
            for grid in (1, -1, 0, 1000):
                gpu_ctx.set_option("agg_grid", grid)
                sums.append(_assert_exact(gpu_ctx, oracle, cols, k, scale, pred, agg, kernel, f"agg_grid={grid} n={n} scale={scale}",
                                          dcols, ask_oracle=grid == 1))
        finally:
            gpu_ctx.set_option("agg_grid", 0)
        assert all(same_float(s, sums[0]) for s in sums)
        for d in dcols:
            d.free()


def test_two_level_fold(gpu_ctx, oracle):
    """One workgroup per tile and 16384 * 1024 + 1025 rows of the three-column variant: 16386 partials, the smallest launch whose
    partials are folded in two levels (1024-partial chunks, then the chunk sums)."""
    n = 16384 * 1024 + 1025
    scale = -10
    k, values, valid = dyadic_cells(6000, n, scale, 0.2)
    specs = [synth_spec(RV_INT64, seed=61, length=n, modulus=100, validity_seed=62, null_percent=15),
             synth_spec(RV_INT64, seed=63, length=n, modulus=100, validity_seed=64, null_percent=15)]
    cols = [oracle.generate(s) for s in specs] + [Column.from_numpy(values, valid)]
    dcols = [gpu_ctx.generate(s) for s in specs] + [gpu_ctx.upload(cols[2])]
    pred = Predicate([Term(0, "<", 70), Term(1, ">=", 15)], "least")
    keep = host_survivors(cols, pred)
    assert 0 < (keep & ~valid).sum() < (keep & valid).sum()
    expected = (dyadic_sum(k, scale, keep & valid), int(keep.sum()))
    kernel = agg_kernel_name(3, 1, AGG_F)
    try:
        gpu_ctx.set_option("agg_grid", -1)
        # the oracle would walk 16.8 M rows cell by cell (ten seconds): the integer sum is the authority here, as everywhere
        two = _assert_exact(gpu_ctx, oracle, cols, k, scale, pred, 2, kernel, "two-level fold", dcols, False, expected)
        gpu_ctx.set_option("agg_grid", 0)
        one = _assert_exact(gpu_ctx, oracle, cols, k, scale, pred, 2, kernel, "default grid", dcols, False, expected)
    finally:
        gpu_ctx.set_option("agg_grid", 0)
    assert same_float(one, two)
    for d in dcols:
        d.free()


# ---- which cells contribute -------------------------------------------------------------------------------------------------
_SPECIALS = {  # the special cells -> the sum when they survive
    "plus_inf": ([math.inf, math.inf], math.inf),
    "minus_inf": ([-math.inf], -math.inf),
    "both_infs": ([math.inf, -math.inf], math.nan),
    "nan": ([math.nan], math.nan),
    "nan_and_infs": ([math.inf, math.nan, -math.inf, 1e300], math.nan),
}


@pytest.mark.parametrize("vec", [1, 2])
@pytest.mark.parametrize("name", list(_SPECIALS))
def test_specials_count_only_where_they_survive(gpu_ctx, oracle, name, vec):
    """Finite dyadic cells plus a handful of NaN / inf cells in the two-column variant.  In surviving valid rows they decide the
    sum (+inf, -inf, NaN); the same cells in rows the predicate drops and under nulls leave the exact finite sum -- a kernel
    that multiplied by its mask instead of selecting would turn it into NaN."""
    cells, want_special = _SPECIALS[name]
    n = 2 * 256 * AGG_R[2] + 1
    kernel = agg_kernel_name(2, vec, AGG_F)
    for scale in DYADIC_SCALES:
        cols, k, pred, agg = agg_case("cols2", n, scale, seed=7000, nulls="least")
        keep, valid = host_survivors(cols, pred), cols[agg].logical_valid()

        def spread(rows):  # the first and the last of these rows and rows of other lanes, waves and tiles in between
            return rows[np.linspace(0, len(rows) - 1, len(cells)).astype(int)]

        for where, rows in (("surviving", spread(np.flatnonzero(keep & valid))), ("dropped", spread(np.flatnonzero(~keep & valid))),
                            ("null", spread(np.flatnonzero(keep & ~valid)))):
            values = cols[agg].values.copy()
            values[rows] = cells
            kk = k.copy()
            kk[rows] = 0  # the integer sum of everything else
            table = [cols[0], Column.from_numpy(values, valid)]
            what = f"{name} in {where} rows, scale={scale} vec={vec}"
            with _options(gpu_ctx, vec=vec):
                if where != "surviving":
                    _assert_exact(gpu_ctx, oracle, table, kk, scale, pred, agg, kernel, what)
                    continue
                _, got, count = gpu_ctx.filter_agg([gpu_ctx.upload(c) for c in table], pred, agg)
            assert gpu_ctx.last_kernel() == kernel and count == int(keep.sum()), what
            assert same_float(got, want_special), f"{what}: {got!r}"
            assert same_float(oracle.filter_agg(table, pred, agg)[1], want_special), what


@pytest.mark.parametrize("vec", [1, 2])
def test_zero_sums(gpu_ctx, oracle, vec):
    """All survivors -0.0: +0.0 (the sum starts at +0.0).  No survivors: 0.0 and count 0.  Every aggregated cell null under
    surviving rows: 0.0 with a count."""
    n = 2 * 256 * AGG_R[2] + 1
    cols, k, pred, agg = agg_case("cols2", n, -10, seed=8000, nulls="least")
    keep, valid = host_survivors(cols, pred), cols[agg].logical_valid()
    fill = np.array(NULL_FILL)[np.arange(n) % 4]
    cases = {
        "minus_zeros": ([cols[0], Column.from_numpy(np.where(keep & valid, -0.0, fill), valid)], pred, int(keep.sum())),
        "no_survivors": (cols, Predicate([Term(0, ">", 1000)], "drops"), 0),
        "all_null": ([cols[0], Column.from_numpy(fill, np.zeros(n, bool))], pred, int(keep.sum())),
    }
    assert keep.sum() > 0
    for what, (table, p, want_count) in cases.items():
        with _options(gpu_ctx, vec=vec):
            _, got, count = gpu_ctx.filter_agg([gpu_ctx.upload(c) for c in table], p, agg)
        assert gpu_ctx.last_kernel() == agg_kernel_name(2, vec, AGG_F), what
        assert count == want_count and same_float(got, 0.0), f"{what} vec={vec}: {got!r}, count {count}"
        _, osum, ocount = oracle.filter_agg(table, p, agg)
        assert ocount == want_count and same_float(osum, 0.0), what


# ---- row-range shards -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[1, 3], ids=lambda n: f"ranks{n}")
def group(request):
    g = capi.Group([0] * request.param)
    yield g
    g.close()


@pytest.mark.parametrize("n", [77, 200_003])
def test_sharded_sum_equals_unsharded_bits(group, gpu_ctx, oracle, n):
    """rv_group_filter_agg over an uploaded nullable dyadic column, predicate on a second column: the shards add in another
    order than the whole table and give the same bits, the integer-derived ones (one rank: through the RCCL all-reduce)."""
    for scale in DYADIC_SCALES:
        for nulls in ("drops", "least"):
            cols, k, pred, agg = agg_case("cols2", n, scale, seed=9000 + n, nulls=nulls)
            want, want_count = agg_expected(cols, k, scale, pred, agg)
            shards = [group.upload(c) for c in cols]
            _, got, count = group.filter_agg(shards, pred, agg)
            what = f"ranks={group.n} n={n} scale={scale} nulls={nulls}"
            assert count == want_count, what
            assert same_float(got, want), f"{what}: got {got!r}, the cells sum to {want!r}"
            single = _assert_exact(gpu_ctx, oracle, cols, k, scale, pred, agg, agg_kernel_name(2, 1, AGG_F), what)
            assert same_float(got, single), what
            for s in shards:
                s.free()


# ---- general data: the one tolerance, derived ---------------------------------------------------------------------------------
def test_general_data_within_the_derived_bound(gpu_ctx, oracle):
    """Cells +-m * 2^e, m a random 53-bit integer, e in [-40, 40], mixed signs: |sum x| << sum |x|, every addition rounds.

    Reference: math.fsum over the taken cells (the correctly rounded sum).  Bound (Higham, Accuracy and Stability of Numerical
    Algorithms, section 4.2): a sum formed by ANY order of additions in which no input takes part in more than k additions has
    |computed - exact| <= gamma_k * sum |x_i|, gamma_k = k u / (1 - k u), u = 2^-53; fsum adds at most u |exact| <= u sum |x_i|,
    which the slack below covers.  The additions an input of filter_agg_kernel<3,4,1,4,F> meets, ntiles = ceil(n / 1024):
      r * ceil(ntiles / grid)   its lane's running sum over the lane's 4 rows of each of the workgroup's tiles
      6 + 4                     the xor butterfly over 64 lanes, the fold of the 4 wave sums
      ceil(grid / 1024)         the running sum of one of the final fold's 1024 threads over the partials
      6 + 16                    that workgroup's butterfly and the fold of its 16 wave sums
    so k = r * ceil(ntiles / grid) + ceil(grid / 1024) + 64 is an upper bound (32 to spare), with grid = min(ntiles, 8192) by
    default and min(ntiles, CUs) under agg_grid = 1 (include/rivulus_gpu.h).  The selected zeros of dropped cells add exactly."""
    n = 300_007
    rng = np.random.default_rng(77)
    m = rng.integers(1 << 52, 1 << 53, n, dtype=np.int64)
    values = np.ldexp(m.astype(np.float64), rng.integers(-40, 41, n).astype(np.int32)) * rng.choice([-1.0, 1.0], n)
    valid = rng.random(n) >= 0.2
    values[~valid] = np.array(NULL_FILL)[np.arange(int((~valid).sum())) % 4]
    others, _, pred, agg = agg_case("cols3", n, 0, seed=78, nulls="least")
    cols = others[:2] + [Column.from_numpy(values, valid)]
    take = host_survivors(cols, pred) & valid
    taken = values[take]
    want, total_abs = math.fsum(taken), math.fsum(np.abs(taken))
    assert abs(want) < 0.1 * total_abs  # the signs do cancel
    dcols = [gpu_ctx.upload(c) for c in cols]
    r, ntiles, u = AGG_R[3], (n + 256 * AGG_R[3] - 1) // (256 * AGG_R[3]), 2.0 ** -53
    cus = gpu_ctx.device_info()["compute_units"]
    try:
        for option, grid in ((0, min(ntiles, 8192)), (1, min(ntiles, cus))):
            gpu_ctx.set_option("agg_grid", option)
            _, got, count = gpu_ctx.filter_agg(dcols, pred, agg)
            assert gpu_ctx.last_kernel() == agg_kernel_name(3, 1, AGG_F)
            assert count == int(host_survivors(cols, pred).sum())
            depth = r * -(-ntiles // grid) + -(-grid // 1024) + 64
            bound = depth * u / (1 - depth * u) * total_abs
            print(f"agg_grid={option}: |got - fsum| = {abs(got - want):.3e}, bound {bound:.3e} (k = {depth}), |fsum| = {abs(want):.3e}")
            assert abs(got - want) <= bound, f"agg_grid={option}: {got!r} against {want!r}, bound {bound!r}"
    finally:
        gpu_ctx.set_option("agg_grid", 0)
    orc = oracle.filter_agg(cols, pred, agg)[1]  # row order: every cell but the first meets up to n additions
    assert abs(orc - want) <= n * u / (1 - n * u) * total_abs
