"""The exact Float64 SUM checks of test_agg_float_gpu.py, without a GPU: the generator's premise, the oracle on the same data,
and proof that the bit compare notices the faults a blocked reduction can have.

Cells are k * 2^s with integer |k| < 2^20 (helpers.dyadic_cells).  While sum(|k|) < 2^53 every partial sum of every reduction
tree is exactly representable, so the sum has one correct bit pattern and integer arithmetic gives it."""
import numpy as np
import pytest

from helpers import (AGG_CASES, AGG_R, DYADIC_K_BITS, DYADIC_SCALES, NULL_FILL, agg_case, agg_expected, agg_sizes, dyadic_cells,
                     dyadic_sum, float_bits, host_survivors, same_float)

# every row count test_agg_float_gpu.py uses; the grid-stride case is (2 * CUs + 1) * 1024 + 65 rows: covered up to 4096 CUs
GPU_TEST_SIZES = sorted({n for c in AGG_R for n in agg_sizes(c)} | {77, 200_003, 300_007, 4097, (2 * 4096 + 1) * 1024 + 65,
                                                                     16384 * 1024 + 1025})


def test_every_partial_sum_is_exactly_representable():
    """sum(|k|) < 2^53 for every size used, from the generator's bound on |k| and, for the sizes cheap enough, from its cells;
    the cells are what they claim to be at every scale, subnormals included."""
    for n in GPU_TEST_SIZES:
        assert n * ((1 << DYADIC_K_BITS) - 1) < 1 << 53
    for n in [s for s in GPU_TEST_SIZES if s <= 300_007]:
        k, _, _ = dyadic_cells(5, n, -10)
        assert np.abs(k).max() < 1 << DYADIC_K_BITS and int(np.abs(k).sum()) < 1 << 53
    k, _, _ = dyadic_cells(5, 20_000, -10)
    assert (k == 0).any() and (k < 0).any() and (k > 0).any()
    for scale in DYADIC_SCALES:
        k, values, valid = dyadic_cells(5, 20_000, scale, 0.2)
        assert np.array_equal(dyadic_cells(5, 20_000, -10, 0.2)[0], k)  # the same integers at every scale
        for i in np.flatnonzero(valid)[:500]:
            assert values[i] == float(int(k[i])) * 2.0 ** scale
        assert np.isfinite(values[valid]).all()
        under = values[~valid]
        assert len(under) > 8 and all(same_float(float(under[j]), NULL_FILL[j % 4]) for j in range(len(under)))
    # subnormal cells are the integers themselves in the low bits: nothing was rounded on the way
    k, values, _ = dyadic_cells(5, 20_000, -1074)
    assert np.array_equal(np.abs(values).view(np.int64), np.abs(k))
    # the largest sums stay finite: 2^20 * 2^20 rows * 2^960 < 2^1000
    assert dyadic_sum(np.full(1 << 20, (1 << 20) - 1, np.int64), 960, np.ones(1 << 20, bool)) < 2.0 ** 1000


def test_compare_is_by_bits():
    assert same_float(0.0, 0.0) and not same_float(0.0, -0.0) and not same_float(-0.0, 0.0)
    assert same_float(float("nan"), -float("nan")) and not same_float(float("nan"), float("inf"))
    assert same_float(float("inf"), float("inf")) and not same_float(float("inf"), float("-inf"))
    assert not same_float(1.0, float(np.nextafter(1.0, 2.0))) and not same_float(5e-324, 0.0)
    assert float_bits(-0.0) == b"\0\0\0\0\0\0\0\x80"


@pytest.mark.parametrize("nulls", ["drops", "least"])
@pytest.mark.parametrize("scale", DYADIC_SCALES)
@pytest.mark.parametrize("case", list(AGG_CASES))
def test_oracle_sum_equals_the_integer_sum(oracle, case, scale, nulls):
    """oracle.filter_agg over the GPU tests' tables == the integer-derived sum and the numpy count, bit for bit, with NaN / inf /
    1e300 under every null cell."""
    if case == "boolean1" and nulls == "least":
        nulls = "drops"  # is_true has no ordering to apply to a null
    ncols = AGG_CASES[case][0]
    for n in (1, 65, 256 * AGG_R[ncols] + 1, 20_011):
        cols, k, pred, agg = agg_case(case, n, scale, seed=n, nulls=nulls)
        want, want_count = agg_expected(cols, k, scale, pred, agg)
        _, got, count = oracle.filter_agg(cols, pred, agg)
        what = f"{case} n={n} scale={scale} nulls={nulls}"
        assert count == want_count == oracle.eval_predicate(cols, pred)[1], what
        assert same_float(got, want), f"{what}: {got!r} != {want!r}"
    if case not in ("plain1", "boolean1"):  # the largest table has null cells, in surviving rows too unless the predicate drops them
        valid, keep = cols[agg].logical_valid(), host_survivors(cols, pred)
        assert (~valid).sum() > 1000 and (keep & valid).any()
        assert (keep & ~valid).any() == (not (case == "nullable1" and nulls == "drops"))


def test_oracle_expression_tree_equals_the_integer_sum(oracle):
    from rivulus_amd.capi import Predicate, Term
    for nulls in ("drops", "least"):
        cols, k, _, agg = agg_case("cols3", 20_011, -10, seed=3)
        pred = Predicate([Term(0, "<", 70), Term(1, ">=", 15), Term(0, "==", 5)], nulls, ("or", ("not", 0), ("and", 1, ("not", 2))))
        want, want_count = agg_expected(cols, k, -10, pred, agg)
        _, got, count = oracle.filter_agg(cols, pred, agg)
        assert count == want_count and same_float(got, want), nulls


# ---- the compare has teeth: a numpy model of the kernel's blocked reduction, right and wrong ------------------------------------
FAULTS = {  # fault -> scales at which it must show
    "drop_last_row": DYADIC_SCALES,
    "take_null_cells": DYADIC_SCALES,
    "multiply_by_mask": DYADIC_SCALES,
    "accumulate_in_float32": DYADIC_SCALES,
    "flush_subnormals": (-1074,),
    # a subnormal partial is the integer itself in its low bits: the high half only carries the sign there
    "low_32_bits_of_one_partial": (-10, 960),
}


def blocked_sum(values, valid, keep, fault=None, lanes=64, rows_per_lane=4, grid=3):
    """filter_agg_kernel in numpy: `grid` workgroups of one wave stride over tiles of lanes * rows_per_lane rows, every lane keeps
    its sum across its tiles, an xor butterfly folds the lanes, the partials are added in index order."""
    n = len(values)
    take = keep & valid
    if fault == "drop_last_row":
        take = take.copy()
        take[n - 1] = False
    if fault == "take_null_cells":
        take = keep
    with np.errstate(all="ignore"):
        x = values * take if fault == "multiply_by_mask" else np.where(take, values, 0.0)
        if fault == "flush_subnormals":
            x = np.where(np.abs(x) < 2.0 ** -1022, 0.0, x)
        dtype = np.float32 if fault == "accumulate_in_float32" else np.float64
        tile = lanes * rows_per_lane
        ntiles = (n + tile - 1) // tile
        x = np.concatenate([x, np.zeros(ntiles * tile - n)]).astype(dtype).reshape(ntiles, rows_per_lane, lanes)
        partials = []
        for b in range(min(grid, ntiles)):
            acc = np.zeros(lanes, dtype)
            for t in range(b, ntiles, grid):
                for j in range(rows_per_lane):
                    acc = acc + x[t, j]
            s = lanes // 2
            while s:
                acc = acc + acc[np.arange(lanes) ^ s]
                s //= 2
            partials.append(acc[0])
        partials = np.array(partials, np.float64)
        if fault == "low_32_bits_of_one_partial":
            partials.view(np.uint64)[0] &= np.uint64(0xFFFFFFFF)
        total = dtype(0)
        for p in partials.astype(dtype):
            total = total + p
    return float(total)


def _model_input(scale, n=1500):
    """1500 rows: six tiles over three workgroups, the last one ragged."""
    k, values, valid = dyadic_cells(11, n, scale, 0.2)
    keep = np.random.default_rng(12).random(n) < 0.6
    k[n - 1], values[n - 1], valid[n - 1], keep[n - 1] = 12345, float(np.ldexp(12345.0, scale)), True, True  # the last row counts
    assert (~valid & keep).any() and (~keep & ~valid).any()
    return k, values, valid, keep


@pytest.mark.parametrize("scale", DYADIC_SCALES)
def test_correct_blocked_reduction_passes_in_any_geometry(scale):
    k, values, valid, keep = _model_input(scale)
    want = dyadic_sum(k, scale, keep & valid)
    for lanes, rows_per_lane, grid in [(64, 4, 3), (64, 16, 1), (16, 1, 7), (64, 4, 1000)]:
        assert same_float(blocked_sum(values, valid, keep, None, lanes, rows_per_lane, grid), want)


@pytest.mark.parametrize("fault", list(FAULTS))
def test_wrong_blocked_reduction_is_flagged(fault):
    for scale in FAULTS[fault]:
        # float32 holds the mixed-sign sums of a few hundred 20-bit integers exactly: that fault needs sums past 2^24
        k, values, valid, keep = _model_input(scale, 40_000 if fault == "accumulate_in_float32" else 1500)
        want = dyadic_sum(k, scale, keep & valid)
        got = blocked_sum(values, valid, keep, fault)
        assert not same_float(got, want), f"{fault} at scale {scale} went unnoticed: {got!r}"
