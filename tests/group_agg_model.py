"""Model of group_by(key).agg(count / sum / min / max) as include/rivulus_gpu.h defines it (rv_hash_aggregate, rv_group_ids): pure
Python / numpy, nothing of the library.  The reference has no aggregate operator, so this file IS the specification the device is
compared with: groups by first occurrence (all null keys one group), integer sums exact mod 2^64, MIN / MAX on an order-preserving
map of the bits with the NaN rule, math.fsum for Float64 sums.

A column is (dtype, values, valid): dtype one of "i64", "f64", "other" (String / Boolean / Null: only COUNT looks at it), values a
numpy array (int64 / float64; anything for "other"), valid a bool array or None (no nulls).  An aggregate is (op, column index) with op
one of "count_rows", "count", "sum", "min", "max".
"""
import math
from fractions import Fraction

import numpy as np

SIGN = np.uint64(1 << 63)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
CANONICAL_NAN = 0x7FF8000000000000
U = Fraction(1, 2 ** 53)


def group_positions(key_values, key_valid):
    """(gids[n], first_row[G]): groups in the order of their first rows; null keys are one group."""
    n = len(key_values)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    valid = np.ones(n, bool) if key_valid is None else np.asarray(key_valid, bool)
    rows = np.arange(n)
    firsts, inverse = np.zeros(0, np.int64), np.zeros(0, np.int64)
    if valid.any():
        _, firsts, inverse = np.unique(np.asarray(key_values)[valid], return_index=True, return_inverse=True)
        firsts = rows[valid][firsts]  # np.unique's index is the first occurrence
    group_of_row = np.empty(n, np.int64)
    group_of_row[valid] = inverse
    if not valid.all():
        group_of_row[~valid] = len(firsts)
        firsts = np.append(firsts, rows[~valid][0])
    order = np.argsort(firsts, kind="stable")
    rank = np.empty(len(firsts), np.int64)
    rank[order] = np.arange(len(firsts))
    return rank[group_of_row], firsts[order].astype(np.int64)


def order_key(bits, is_float, is_max):
    """uint64 keys whose unsigned order is the order of the cells: Int64 with the sign flipped; Float64 -inf < .. < -0.0 < +0.0 < ..
    < +inf, every NaN at the end that wins."""
    bits = np.asarray(bits, np.uint64)
    if not is_float:
        return bits ^ SIGN
    nan = (bits & ~SIGN) > np.uint64(0x7FF0000000000000)
    neg = (bits & SIGN) != 0
    key = np.where(neg, ~bits, bits | SIGN)
    return np.where(nan, ALL if is_max else np.uint64(0), key)


def order_value(key, is_float):
    key = int(key)
    if not is_float:
        return key ^ (1 << 63)
    if key == 0 or key == 0xFFFFFFFFFFFFFFFF:
        return CANONICAL_NAN
    return key & 0x7FFFFFFFFFFFFFFF if key >> 63 else key ^ 0xFFFFFFFFFFFFFFFF


def float_sum(cells):
    """The correctly rounded sum of Float64 cells, + 0.0 (a sum is never -0.0; no cells: +0.0); inf and NaN as IEEE has them."""
    cells = [float(x) for x in cells]
    if any(math.isnan(x) for x in cells) or (math.inf in cells and -math.inf in cells):
        return math.nan
    if math.inf in cells:
        return math.inf
    if -math.inf in cells:
        return -math.inf
    try:
        return math.fsum(cells) + 0.0
    except OverflowError:  # the exact sum is past the largest double
        return math.inf if sum(Fraction(x) for x in cells) > 0 else -math.inf


def gamma_bound(cells):
    """gamma_{n-1} x sum|x| as a Fraction: the bound on |any summation order - the exact sum| for n finite cells."""
    n = len(cells)
    if n < 2:
        return Fraction(0)
    k = (n - 1) * U
    return k / (1 - k) * sum(abs(Fraction(float(x))) for x in cells)


def aggregate(key, columns, specs, exact_float=False):
    """key: (values, valid).  Returns a dict: groups, gids, first_row, key_valid[G] (False for the null group), key_values[G], and
    aggs: one (dtype, bits[G] as Python ints -- uint64 patterns --, valid[G] bools or None, cells) per aggregate, where `cells` is, for
    a Float64 SUM, the list of each group's non-null cells (for the gamma bound) and None otherwise.  exact_float: the caller knows
    every partial sum of every Float64 SUM to be representable (cells k * 2^s): the sums are then exact in any order and numpy adds them."""
    key_values, key_valid = key
    gids, first_row = group_positions(key_values, key_valid)
    G, n = len(first_row), len(gids)
    out = {"groups": G, "gids": gids, "first_row": first_row}
    kv = np.ones(n, bool) if key_valid is None else np.asarray(key_valid, bool)
    out["key_valid"] = kv[first_row] if G else np.zeros(0, bool)
    out["key_values"] = np.asarray(key_values)[first_row] if G and len(np.asarray(key_values)) else np.zeros(G, np.int64)
    order = np.argsort(gids, kind="stable")
    starts = np.searchsorted(gids[order], np.arange(G)) if G else np.zeros(0, np.int64)
    aggs = []
    for op, ci in specs:
        if op == "count_rows":
            aggs.append(("i64", [int(x) for x in np.bincount(gids, minlength=G)] if G else [], None, None))
            continue
        dtype, values, valid = columns[ci]
        valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
        if dtype == "other" and values is None:
            values = np.zeros(n, np.int64)
        counts = np.bincount(gids[valid], minlength=G) if G else np.zeros(0, np.int64)
        if op == "count":
            aggs.append(("i64", [int(x) for x in counts], None, None))
            continue
        assert dtype in ("i64", "f64"), "SUM / MIN / MAX take an Int64 or Float64 column"
        if G == 0:
            aggs.append((dtype, [], None, [] if (op == "sum" and dtype == "f64") else None))
            continue
        bits = np.asarray(values).view(np.uint64)
        if op == "sum" and dtype == "i64":
            s = np.add.reduceat(np.where(valid, bits, np.uint64(0))[order], starts)  # uint64 adds wrap: mod 2^64
            aggs.append(("i64", [int(x) for x in s], None, None))
        elif op == "sum":
            fv, fo = np.asarray(values, np.float64)[order], valid[order]
            ends = list(starts[1:]) + [n]
            if exact_float:
                s = np.add.reduceat(np.where(fo, fv, 0.0), starts) + 0.0
                aggs.append(("f64", [int(x) for x in s.view(np.uint64)], None, None))
            else:
                cells = [fv[b:e][fo[b:e]].tolist() for b, e in zip(starts, ends)]
                s = np.array([float_sum(c) for c in cells], np.float64)
                aggs.append(("f64", [int(x) for x in s.view(np.uint64)], None, cells))
        else:
            is_max, is_float = op == "max", dtype == "f64"
            identity = np.uint64(0) if is_max else ALL
            keys = np.where(valid, order_key(bits, is_float, is_max), identity)[order]
            red = (np.maximum if is_max else np.minimum).reduceat(keys, starts)
            has = counts > 0
            aggs.append((dtype, [order_value(k, is_float) if h else 0 for k, h in zip(red, has)], None if has.all() else [bool(h) for h in has], None))
    out["aggs"] = aggs
    return out


# ---- cells as tests/golden/group_agg_cases.json writes them ------------------------------------------------------------------------
def float_bits(x):
    """uint64 pattern of a Float64 cell (a number or "nan" / "inf" / "-inf" / "-0.0"), every NaN canonical."""
    v = float(x)
    return CANONICAL_NAN if math.isnan(v) else int(np.array([v], np.float64).view(np.uint64)[0])


def canonical(dtype, bits):
    """a cell's bits as tests compare them: Int64 as the signed value, Float64 with every NaN canonical (payloads are not specified)"""
    bits = int(bits) & 0xFFFFFFFFFFFFFFFF
    if dtype == "f64":
        return CANONICAL_NAN if (bits & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000 else bits
    return bits - (1 << 64) if bits >> 63 else bits


def column_of(dtype, cells):
    """(dtype, values, valid) of a JSON cell list; valid is None when no cell is null"""
    valid = np.array([c is not None for c in cells], bool)
    if dtype == "i64":
        values = np.array([0 if c is None else c for c in cells], np.int64)
    elif dtype == "f64":
        values = np.array([float_bits(0.0 if c is None else c) for c in cells], np.uint64).view(np.float64)
    else:
        values = None
    return dtype, values, (None if valid.all() else valid)


def expected_cells(dtype, cells):
    return [None if c is None else canonical(dtype, float_bits(c) if dtype == "f64" else c) for c in cells]


def agg_cells(agg):
    """[None | canonical cell] of one aggregate of aggregate()'s result"""
    dtype, bits, valid, _ = agg
    return [None if valid is not None and not valid[g] else canonical(dtype, b) for g, b in enumerate(bits)]
