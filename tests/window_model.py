"""Window functions in numpy / Python: the executable statement of include/rivulus_gpu.h's rv_window comment (K12).  Nothing of the
library.  The order is tests/sort_model.py's, the partition equality tests/group_keys_model.py's, MIN / MAX and their NaN rule
tests/group_agg_model.py's.

A column is (dtype, values, valid): dtype "i64" / "f64" / "bool" / "str" / "null"; values a numpy array of int64 / float64 / bool, a list of
str for "str", anything of the frame's length for "null"; valid a bool array or None (no nulls).  An expression is (op, column index) or
(op, column index, offset) with op "row_number", "rank", "dense_rank", "cum_count", "cum_sum", "cum_min", "cum_max", "lag" or "lead".
partition_by is a list of column indices, order_by a list of (column index, flags) with sort_model's flags.

window() returns one (dtype, values, valid) per expression IN ROW ORDER: values int64 for "i64", uint64 bit patterns for "f64" (every NaN
canonical), bool for "bool", a list for "str", None for "null"; valid a bool array (all True when no cell is null); 0 / False / "" lies
under a null.  The numbering and the integer aggregates are written with cumulative sums over the sequence; Float64 CUM_SUM, MIN / MAX and
LAG / LEAD are per partition a sequential loop over its rows in window order -- the statement of the semantics as it reads.
"""
import numpy as np

import group_agg_model as A
import group_keys_model as K
import sort_model as S


def rows_of(cols):
    return len(cols[0][1])


def valid_of(col):
    dtype, values, valid = col
    n = len(values)
    if dtype == "null":
        return np.zeros(n, bool)
    return np.ones(n, bool) if valid is None else np.asarray(valid, bool)


def partition_codes(cols, partition_by):
    n = rows_of(cols)
    if not partition_by or n == 0:
        return np.zeros(n, np.int64)
    keys = []
    for c in partition_by:
        dtype, values, valid = cols[c]
        assert dtype != "str", "String partition keys go through the dictionary (the host layer)"
        keys.append(("null", None, n) if dtype == "null" else (dtype, values, valid))
    return K.codes(keys)[0]


def sequence(cols, partition_by, order_by):
    """(seq, part_head, peer_head): the rows with every partition's side by side (partitions by first occurrence), each partition in the
    order rv_sort over order_by gives it, and per position whether a partition / a peer group starts there."""
    n = rows_of(cols)
    codes = partition_codes(cols, partition_by)
    perm = S.sort_frame(cols_for_sort(cols), order_by) if order_by else np.arange(n, dtype=np.int64)
    seq = perm[np.argsort(codes[perm], kind="stable")]
    part_head = np.ones(n, bool)
    part_head[1:] = codes[seq][1:] != codes[seq][:-1]
    peer_head = part_head.copy()
    for c, flags in order_by:
        cls, key = S.working_keys(cols_for_sort(cols)[c], flags)
        cls, key = cls[seq], key[seq]
        peer_head[1:] |= (cls[1:] != cls[:-1]) | (key[1:] != key[:-1])
    return seq, part_head, peer_head


def cols_for_sort(cols):
    """the frame as sort_model takes it (only the order keys are looked at: anything else becomes a placeholder)"""
    out = []
    for dtype, values, valid in cols:
        if dtype in ("i64", "f64"):
            out.append((dtype, values, valid))
        else:
            out.append(("null", np.zeros(len(values), np.int64), None))
    return out


def window(cols, partition_by, order_by, exprs, exact_float=False):
    """exact_float: the caller knows every partial sum of every Float64 CUM_SUM to be representable (integer-valued cells): the sums are
    then exact in any order and numpy's cumulative sum stands for the loop."""
    n = rows_of(cols)
    for c, _ in order_by:
        assert cols[c][0] in ("i64", "f64", "null"), "Boolean and String order keys are refused"
    seq, part_head, peer_head = sequence(cols, partition_by, order_by)
    pos = np.arange(n, dtype=np.int64)
    start = np.maximum.accumulate(np.where(part_head, pos, 0)) if n else pos  # the position of the partition's head
    heads = np.flatnonzero(part_head)
    ends = np.append(heads[1:], n)  # one past each partition
    end = np.repeat(ends, ends - heads) if n else pos
    out = []
    for e in exprs:
        op, ci = e[0], e[1]
        k = int(e[2]) if len(e) > 2 else 0
        dtype, values, _ = cols[ci]
        valid = valid_of(cols[ci])[seq]
        res_valid = np.ones(n, bool)
        if op == "row_number":
            res, rdtype = pos - start + 1, "i64"
        elif op == "rank":
            res, rdtype = (np.maximum.accumulate(np.where(peer_head, pos, 0)) if n else pos) - start + 1, "i64"
        elif op == "dense_rank":
            c = np.cumsum(peer_head.astype(np.int64))
            res, rdtype = (c - c[start] + 1) if n else pos, "i64"
        elif op == "cum_count":
            c = np.cumsum(valid.astype(np.int64))
            res, rdtype = (c - c[start] + valid[start]) if n else pos, "i64"
        elif op == "cum_sum" and dtype == "i64":
            x = np.where(valid, np.asarray(values, np.int64)[seq].view(np.uint64), np.uint64(0))
            c = np.cumsum(x, dtype=np.uint64)  # wraps: mod 2^64
            res, rdtype = ((c - c[start] + x[start]) if n else x).view(np.int64), "i64"
        elif op == "cum_sum":
            assert dtype == "f64", "CUM_SUM takes an Int64 or Float64 column"
            x = np.where(valid, np.asarray(values, np.float64)[seq], 0.0)
            if exact_float:
                c = np.cumsum(x)
                s = (c - c[start] + x[start]) + 0.0 if n else x
            else:
                s = np.zeros(n, np.float64)
                with np.errstate(all="ignore"):
                    for b, t in zip(heads, ends):
                        acc = 0.0
                        for j in range(b, t):
                            acc = acc + (x[j] if x[j] != 0 else 0.0)
                            s[j] = acc
            res, rdtype = canonical_bits(s), "f64"
        elif op in ("cum_min", "cum_max"):
            assert dtype in ("i64", "f64"), "CUM_MIN / CUM_MAX take an Int64 or Float64 column"
            is_max, is_float = op == "cum_max", dtype == "f64"
            bits = np.ascontiguousarray(np.asarray(values)[seq]).view(np.uint64)
            keys = np.where(valid, A.order_key(bits, is_float, is_max), np.uint64(0) if is_max else A.ALL)
            res = np.zeros(n, np.uint64)
            for b, t in zip(heads, ends):
                run = (np.maximum if is_max else np.minimum).accumulate(keys[b:t])
                seen = np.cumsum(valid[b:t]) > 0
                res_valid[b:t] = seen
                res[b:t] = [A.order_value(q, is_float) if h else 0 for q, h in zip(run, seen)]
            rdtype = dtype
            if dtype == "i64":
                res = res.view(np.int64)
        else:
            assert op in ("lag", "lead")
            src = pos - k if op == "lag" else pos + k
            there = (src >= start) & (src < end)
            src = np.where(there, src, 0)
            res_valid = there & (valid[src] if n else there)
            rdtype = dtype
            if dtype == "null":
                res, res_valid = None, np.zeros(n, bool)
            elif dtype == "str":
                res = [values[seq[s]] if v else "" for s, v in zip(src, res_valid)]
            elif dtype == "bool":
                res = np.where(res_valid, np.asarray(values, bool)[seq][src] if n else False, False)
            else:
                bits = np.ascontiguousarray(np.asarray(values)[seq]).view(np.uint64)
                res = np.where(res_valid, bits[src] if n else bits, np.uint64(0))
                res = res.view(np.int64) if dtype == "i64" else res
        # back to row order
        back_valid = np.empty(n, bool)
        back_valid[seq] = res_valid
        if res is None:
            out.append((rdtype, None, back_valid))
        elif isinstance(res, list):
            back = [""] * n
            for j, r in enumerate(seq):
                back[r] = res[j]
            out.append((rdtype, back, back_valid))
        else:
            res = np.asarray(res)
            back = np.empty(n, res.dtype)
            back[seq] = res
            out.append((rdtype, back, back_valid))
    return out


def canonical_bits(x):
    """uint64 patterns of Float64 cells, every NaN canonical (payloads are not specified)"""
    bits = np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64).copy()
    bits[(bits & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000)] = np.uint64(A.CANONICAL_NAN)
    return bits


def frames(cols, partition_by, order_by, ci):
    """per ROW the list of the non-null Float64 cells of column ci in the row's frame, in window order: what the gamma bound of a
    CUM_SUM is worked out from (small inputs only: quadratic)"""
    n = rows_of(cols)
    seq, part_head, _ = sequence(cols, partition_by, order_by)
    valid = valid_of(cols[ci])[seq]
    x = np.asarray(cols[ci][1], np.float64)[seq]
    out = [None] * n
    cur = []
    for j in range(n):
        if part_head[j]:
            cur = []
        if valid[j]:
            cur = cur + [float(x[j])]
        out[seq[j]] = cur
    return out


# ---- cells as tests/golden/window_cases.json writes them ----------------------------------------------------------------------------
def column_of(dtype, cells):
    """(dtype, values, valid) of a JSON cell list: null -> a null cell; Float64 cells are numbers or "nan" / "-nan" / "inf" / "-inf" /
    "-0.0" (sort_model.column_of); Boolean cells true / false; String cells strings."""
    n = len(cells)
    if dtype in ("i64", "f64", "null"):
        return S.column_of(dtype, cells)
    valid = np.array([c is not None for c in cells], bool)
    if dtype == "bool":
        return dtype, np.array([bool(c) for c in cells], bool), (None if valid.all() else valid)
    assert dtype == "str"
    return dtype, ["" if c is None else c for c in cells], (None if valid.all() else valid)


def cells_of(result):
    """a result column as a JSON-like cell list: None for a null, Int64 as int, Float64 as float (nan compares through repr), Boolean as
    bool, String as str"""
    dtype, values, valid = result
    out = []
    for i in range(len(valid)):
        if not valid[i]:
            out.append(None)
        elif dtype == "i64":
            out.append(int(values[i]))
        elif dtype == "f64":
            out.append(float(np.array([values[i]], np.uint64).view(np.float64)[0]))
        elif dtype == "bool":
            out.append(bool(values[i]))
        else:
            out.append(values[i])
    return out


def expected_cells(dtype, cells):
    """the canonical form of a JSON list of expected cells, comparable with cells_of through same_cells"""
    if dtype != "f64":
        return list(cells)
    return [None if c is None else float(c) for c in cells]


def same_cells(a, b):
    """cell lists equal, Float64 by bit pattern with every NaN equal to every NaN"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if isinstance(x, float) and isinstance(y, float):
            if x != x and y != y:
                continue
            if np.array([x]).view(np.uint64)[0] != np.array([y]).view(np.uint64)[0]:
                return False
        elif x != y or type(x) is not type(y):
            return False
    return True
