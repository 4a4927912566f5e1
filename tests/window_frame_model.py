"""Window frames in numpy / Python: the executable statement of include/rivulus_gpu.h's rv_window_frames comment (K12a).  Nothing of the
library.  The partition, the order and the peers are tests/window_model.py's; MIN / MAX and their NaN rule tests/group_agg_model.py's.

Columns and results are window_model's (dtype, values, valid) triples.  An expression is one of
  (op, column index, preceding, following)   op "count", "sum", "min", "max", "avg", "first_value", "last_value"; offsets signed ints,
                                             UNBOUNDED (or None) for the partition's edge
  ("ntile", column index, buckets)
  (op, column index[, offset])               window_model's ops, computed HERE from the frame sentences (ROW_NUMBER is the size of the frame
                                             (UNBOUNDED, 0), CUM_x is x over it, LAG(k) is FIRST_VALUE over (k, -k), LEAD(k) over (-k, k))

window_frames() is a sequential loop per row over the cells of its frame: the header's sentences as they read, not the block method.  A
Float64 SUM is the left fold of the frame's non-null cells in window order, from +0.0, a zero of either sign entering as +0.0; frame_cells()
hands out the cells themselves for math.fsum and the gamma bound.  fast=True computes the same results with cumulative sums and slices
(exact for integers mod 2^64; Float64 sums only with exact_float, i.e. integer-valued cells whose every partial sum is representable) so
that the GPU suite's larger shapes take milliseconds; the CPU suite holds the two against each other.
"""
import numpy as np

import group_agg_model as A
import window_model as M

UNBOUNDED = (1 << 63) - 1
FRAME_OPS = ("count", "sum", "min", "max", "avg", "first_value", "last_value")
OFFSET_MOST = 1 << 62


def frame_ok(preceding, following):
    pu, fu = preceding == UNBOUNDED, following == UNBOUNDED
    if (not pu and abs(preceding) > OFFSET_MOST) or (not fu and abs(following) > OFFSET_MOST):
        return False
    return pu or fu or preceding + following >= 0


def edge(v):
    return UNBOUNDED if v is None else int(v)


def geometry(cols, partition_by, order_by):
    """(seq, part_head, peer_head, start, end): window_model's sequence, and per position the position of its partition's head and one
    past its partition's last row"""
    n = M.rows_of(cols)
    seq, part_head, peer_head = M.sequence(cols, partition_by, order_by)
    pos = np.arange(n, dtype=np.int64)
    start = np.maximum.accumulate(np.where(part_head, pos, 0)) if n else pos
    heads = np.flatnonzero(part_head)
    ends = np.append(heads[1:], n)
    end = np.repeat(ends, ends - heads) if n else pos
    return seq, part_head, peer_head, start, end


def bounds(j, start, end, preceding, following):
    """the frame of sequence position j as sequence positions lo .. hi inclusive; lo > hi: empty"""
    lo = start if preceding == UNBOUNDED else max(start, j - preceding)
    hi = end - 1 if following == UNBOUNDED else min(end - 1, j + following)
    return lo, hi


def normalise(e):
    """an expression as (kind, column, preceding, following, buckets) with kind a FRAME_OPS name, "ntile", "rank" or "dense_rank" """
    op, ci = e[0], e[1]
    k = int(e[2]) if len(e) > 2 and e[2] is not None else 0
    if op in FRAME_OPS:
        return op, ci, edge(e[2]), edge(e[3]), 0
    if op == "ntile":
        return op, ci, 0, 0, k
    if op == "row_number":
        return "rows", ci, UNBOUNDED, 0, 0
    if op in ("rank", "dense_rank"):
        return op, ci, 0, 0, 0
    if op.startswith("cum_"):
        return op[4:], ci, UNBOUNDED, 0, 0
    assert op in ("lag", "lead"), op
    return ("first_value", ci, k, -k, 0) if op == "lag" else ("first_value", ci, -k, k, 0)


def result_dtype(kind, dtype):
    if kind in ("count", "rows", "ntile", "rank", "dense_rank"):
        return "i64"
    return "f64" if kind == "avg" else dtype


def wrap(s):
    s %= 1 << 64
    return s - (1 << 64) if s >> 63 else s


def window_frames(cols, partition_by, order_by, exprs, exact_float=False, fast=False):
    n = M.rows_of(cols)
    for c, _ in order_by:
        assert cols[c][0] in ("i64", "f64", "null"), "Boolean and String order keys are refused"
    seq, part_head, peer_head, start, end = geometry(cols, partition_by, order_by)
    out = []
    for e in exprs:
        kind, ci, p, f, buckets = normalise(e)
        dtype, values, _ = cols[ci]
        if kind in FRAME_OPS:
            assert frame_ok(p, f), "a frame's finite offsets are at most 2^62 and preceding + following >= 0"
        if kind in ("sum", "min", "max", "avg"):
            assert dtype in ("i64", "f64"), "SUM / MIN / MAX / AVG take an Int64 or Float64 column"
        if kind == "ntile":
            assert buckets >= 1, "NTILE of 0 buckets"
        valid = M.valid_of(cols[ci])[seq]
        rdtype = result_dtype(kind, dtype)
        work = (_fast if fast else _loop)(kind, dtype, values, valid, seq, part_head, peer_head, start, end, p, f, buckets, exact_float)
        out.append(_to_rows(seq, rdtype, *work))
    return out


def _to_rows(seq, rdtype, res, res_valid):
    n = len(seq)
    back_valid = np.empty(n, bool)
    back_valid[seq] = res_valid
    if rdtype == "null":
        return rdtype, None, np.zeros(n, bool)
    if rdtype == "str":
        back = [""] * n
        for j, r in enumerate(seq):
            back[r] = res[j]
        return rdtype, back, back_valid
    res = np.asarray(res, {"i64": np.int64, "f64": np.uint64, "bool": bool}[rdtype])
    if rdtype == "f64":
        res = M.canonical_bits(res.view(np.float64))  # NaN payloads are not specified
    back = np.empty(n, res.dtype)
    back[seq] = res
    return rdtype, back, back_valid


def _cells_in_order(dtype, values, seq):
    if dtype == "null":
        return [None] * len(seq)
    if dtype == "str":
        return [values[r] for r in seq]
    return np.asarray(values)[seq]


def _fold(kind, dtype, x, ok):
    """(bits or value, valid) of SUM / MIN / MAX / AVG / COUNT over the frame's cells x (window order) with validity ok: the sentences"""
    cells = [x[t] for t in range(len(x)) if ok[t]]
    if kind == "count":
        return len(cells), True
    if kind in ("sum", "avg"):
        if dtype == "i64":
            s = wrap(sum(int(c) for c in cells))
        else:
            s = 0.0
            with np.errstate(all="ignore"):
                for c in cells:
                    s = s + (float(c) if c != 0 else 0.0)
        if kind == "sum":
            return (s if dtype == "i64" else int(M.canonical_bits([s])[0])), True
        if not cells:
            return 0, False
        with np.errstate(all="ignore"):
            return int(M.canonical_bits([np.float64(s) / np.float64(len(cells))])[0]), True
    if not cells:
        return 0, False
    is_float, is_max = dtype == "f64", kind == "max"
    keys = A.order_key(np.ascontiguousarray(np.asarray(cells)).view(np.uint64), is_float, is_max)
    v = A.order_value(max(keys) if is_max else min(keys), is_float)
    return (wrap(v) if dtype == "i64" else v), True


def _loop(kind, dtype, values, valid, seq, part_head, peer_head, start, end, p, f, buckets, exact_float):
    n = len(seq)
    x = _cells_in_order(dtype, values, seq)
    res_valid = np.ones(n, bool)
    rdtype = result_dtype(kind, dtype)
    res = [("" if rdtype == "str" else 0)] * n
    for j in range(n):
        b, t = int(start[j]), int(end[j])
        pos, length = j - b + 1, t - b
        if kind == "ntile":
            q, r = divmod(length, buckets)
            bucket, left = 0, pos
            while left > 0:  # deal the rows out: the first r buckets take q + 1, the rest q
                bucket += 1
                left -= q + 1 if bucket <= r else q
            res[j] = bucket
        elif kind == "rank":
            s = j
            while not peer_head[s]:
                s -= 1
            res[j] = s - b + 1
        elif kind == "dense_rank":
            res[j] = int(np.count_nonzero(peer_head[b:j + 1]))
        else:
            lo, hi = bounds(j, b, t, p, f)
            if kind == "rows":
                res[j] = max(0, hi - lo + 1)
            elif kind in ("first_value", "last_value"):
                at = lo if kind == "first_value" else hi
                ok = lo <= hi and bool(valid[at])
                res_valid[j] = ok
                if ok and dtype not in ("null",):
                    c = x[at]
                    res[j] = c if dtype in ("str", "bool") else int(np.array([c]).view(np.uint64)[0]) if dtype == "f64" else int(c)
            else:
                frame = range(lo, hi + 1)
                res[j], res_valid[j] = _fold(kind, dtype, [x[s] for s in frame], [valid[s] for s in frame])
    if dtype == "null" and kind in ("first_value", "last_value"):
        res_valid[:] = False
    return res, res_valid


def _fast(kind, dtype, values, valid, seq, part_head, peer_head, start, end, p, f, buckets, exact_float):
    n = len(seq)
    if n == 0 or kind in ("rank", "dense_rank") or (dtype in ("str", "null") and kind in ("first_value", "last_value")):
        return _loop(kind, dtype, values, valid, seq, part_head, peer_head, start, end, p, f, buckets, exact_float)
    j = np.arange(n, dtype=np.int64)
    res_valid = np.ones(n, bool)
    if kind == "ntile":
        pos, length = j - start + 1, end - start
        q, r = length // buckets, length % buckets
        big = r * (q + 1)
        return np.where(pos <= big, (pos - 1) // (q + 1) + 1, r + (pos - 1 - big) // np.maximum(q, 1) + 1), res_valid
    big = 1 << 40  # offsets beyond every position reach the same rows
    lo = start if p == UNBOUNDED else np.maximum(start, j - max(-big, min(big, p)))
    hi = end - 1 if f == UNBOUNDED else np.minimum(end - 1, j + max(-big, min(big, f)))
    empty = lo > hi
    lo_c, hi_c = np.where(empty, 0, lo), np.where(empty, 0, hi)
    if kind == "rows":
        return np.where(empty, 0, hi - lo + 1), res_valid
    if kind in ("first_value", "last_value"):
        at = lo_c if kind == "first_value" else hi_c
        res_valid = ~empty & valid[at]
        x = np.ascontiguousarray(np.asarray(values)[seq])
        if dtype == "bool":
            return np.where(res_valid, x[at], False), res_valid
        return np.where(res_valid, x.view(np.uint64)[at], np.uint64(0)).view(np.int64 if dtype == "i64" else np.uint64), res_valid
    between = lambda c: np.where(empty, c.dtype.type(0), c[hi_c + 1] - c[lo_c])  # c: exclusive cumulative sums, n + 1 of them
    count = between(np.concatenate([np.zeros(1, np.int64), np.cumsum(valid.astype(np.int64))]))
    if kind == "count":
        return count, res_valid
    x = np.ascontiguousarray(np.asarray(values)[seq])
    if kind in ("sum", "avg"):
        if dtype == "f64":
            assert exact_float, "the fast path sums Float64 cells only when they are integer-valued"
            ints = np.where(valid, x, 0.0).astype(np.int64)
        else:
            ints = np.where(valid, x, 0)
        s = between(np.concatenate([np.zeros(1, np.uint64), np.cumsum(ints.view(np.uint64), dtype=np.uint64)])).view(np.int64)  # wraps: mod 2^64
        if kind == "sum":
            return (s if dtype == "i64" else M.canonical_bits(s.astype(np.float64) + 0.0)), res_valid
        res_valid = count > 0
        with np.errstate(all="ignore"):
            avg = s.astype(np.float64) / np.where(res_valid, count, 1).astype(np.float64)
        return np.where(res_valid, M.canonical_bits(avg), np.uint64(0)), res_valid
    is_float, is_max = dtype == "f64", kind == "max"
    keys = np.where(valid, A.order_key(x.view(np.uint64), is_float, is_max), np.uint64(0) if is_max else A.ALL)
    res_valid = count > 0
    res = np.zeros(n, np.uint64)
    reduce = np.max if is_max else np.min
    for t in np.flatnonzero(res_valid):
        res[t] = A.order_value(reduce(keys[lo[t]:hi[t] + 1]), is_float)
    return (res.view(np.int64) if dtype == "i64" else res), res_valid


def frame_cells(cols, partition_by, order_by, ci, preceding, following):
    """per ROW the list of the non-null Float64 cells of column ci in the row's frame, in window order: what math.fsum and the gamma bound
    of a SUM are worked out from (small inputs only: rows x width)"""
    n = M.rows_of(cols)
    seq, _, _, start, end = geometry(cols, partition_by, order_by)
    valid = M.valid_of(cols[ci])[seq]
    x = np.asarray(cols[ci][1], np.float64)[seq]
    out = [None] * n
    for j in range(n):
        lo, hi = bounds(j, int(start[j]), int(end[j]), edge(preceding), edge(following))
        out[seq[j]] = [float(x[s]) for s in range(lo, hi + 1) if valid[s]]
    return out
