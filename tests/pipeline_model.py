"""Operator pipelines in plain Python: one frame type and one pure function per step kind, each a thin adapter over the model the
operator already has (helpers.host_survivors, arith_model, join_model, group_agg_model, sort_model).  No rule is restated here, with
one exception: string_ids() states rv_string_dict_build's id rule (the row of a string's first occurrence), which no model file has.

A frame is a list of columns (dtype, values, valid), the representation sort_model and group_agg_model share:
  dtype   "i64" | "f64" | "bool" | "str" | "null"
  values  numpy int64 / float64 / bool array; a Python list with None under a null for "str"; zeros for "null"
  valid   a bool array, or None when no cell is null (a "null" column is all null whatever it says)
What lies under a null cell of `values` is never compared and never read by a step.

A step is a dict (JSON can hold it; trees may arrive as lists):
  {"kind": "filter",  "terms": [(col, op, literal)], "nulls": "drops" | "least", "expr": tree | None, "via": "project" | "selection"}
  {"kind": "mask",    "terms": [(col, op, literal)], "expr": tree | None}                       compare -> and / or / not -> filter
  {"kind": "arith",   "tree": arithmetic tree}                                                   the result is appended as a new column
  {"kind": "join",    "probe_key": c, "build_key": c, "chunked": bool, "side": "probe" | "build"}  the frame's key, the second frame's key
  {"kind": "group",   "key": c, "specs": [(op, col | None)]}                                    -> [key cells, aggregate 0, ...]
  {"kind": "sort",    "keys": [(col, flags)], "via": "sort" | "chain"}
  {"kind": "reshape", "how": "slice", "offset": o, "tail": t}                                   rows [min(o, n // 2), n - t)
  {"kind": "reshape", "how": "concat", "eighths": e}                                            rows [h, n) then [0, h), h = n * e // 8
  {"kind": "reshape", "how": "take_first", "col": c}                                            take by the group first rows of column c
  {"kind": "reshape", "how": "take_sorted", "col": c, "flags": f}                               take by the sort indices of column c
and, adapters over window_model, topk_model / sort_model, outer_join_model and group_keys_model (KINDS_ALL; KINDS is the older set):
  {"kind": "window",  "partition_by": [c], "order_by": [(c, flags)], "exprs": [(op, c[, k])]}   the results are appended, as arith's is
  {"kind": "topk",    "keys": [(c, flags)], "k": ["abs", K] | ["of", num, den[, add]], "via": "frame" | "indices", "select": bool}
                      k = K, or max(0, rows * num // den + add) of the rows the step receives; "indices": rv_top_k_indices over the first
                      key alone, then take_device; "select": option top_k_select_from_rows = 1 around the call
  {"kind": "outer_join", "how": "outer" | "full" | "semi" | "anti", and the fields of "join"}   rv_hash_join_kind's columns
  {"kind": "group_keys", "keys": [c1, c2[, c3]], "specs": [(op, col | None)]}                   -> [key cells of every key, aggregate 0, ...]

Beside every frame runs its `meta`, one dict per column: what include/rivulus_gpu.h lets a caller expect of the device column --
  bitmap  a validity bitmap is attached (None: the header states no rule)
  known   null_count is known without a device pass (None: no rule)
  offset  the column's element offset (None: no rule)
  made    an operator wrote the column's buffers (False: an upload or a CSV batch, or a slice of one)
"""
import numpy as np

import arith_model
import group_agg_model
import group_keys_model
import join_model
import outer_join_model
import sort_model
import topk_model
import window_model
from helpers import host_survivors
from rivulus_amd.capi import RV_BOOLEAN, RV_FLOAT64, RV_INT64, RV_NULL, RV_STRING, Column, Predicate, Term

RV = {"i64": RV_INT64, "f64": RV_FLOAT64, "bool": RV_BOOLEAN, "str": RV_STRING, "null": RV_NULL}
DTYPE_OF_RV = {v: k for k, v in RV.items()}
KINDS = ("filter", "mask", "arith", "join", "group", "sort", "reshape")
NEW_KINDS = ("window", "topk", "outer_join", "group_keys")
KINDS_ALL = KINDS + NEW_KINDS
JOINS = ("join", "outer_join")  # the kinds that read a second frame
HOW = {"outer": outer_join_model.PROBE_OUTER, "full": outer_join_model.FULL_OUTER, "semi": outer_join_model.PROBE_SEMI, "anti": outer_join_model.PROBE_ANTI}
CANONICAL_NAN = np.uint64(group_agg_model.CANONICAL_NAN)
JOIN_CHUNK = 1024


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def rows(frame):
    return len(frame[0][1])


def dtypes(frame):
    return [c[0] for c in frame]


def valid_of(col):
    dtype, values, valid = col
    if dtype == "null":
        return np.zeros(len(values), bool)
    return np.ones(len(values), bool) if valid is None else np.asarray(valid, bool)


def null_count(col):
    return int((~valid_of(col)).sum())


def cells(col):
    """The column as a list of Python cells, None under a null (what arith_model and join_model take)."""
    dtype, values, _ = col
    ok = valid_of(col)
    raw = values if dtype == "str" else np.asarray(values).tolist()
    return [x if v else None for x, v in zip(raw, ok)]


def column_of(dtype, cell_list):
    """A column from a list of cells (None: null); Float64 cells may be spelled "nan", "inf", "-inf", "-0.0" as in the golden files."""
    n = len(cell_list)
    if dtype == "null":
        return "null", np.zeros(n, np.int64), None
    valid = np.array([c is not None for c in cell_list], bool)
    if dtype == "str":
        return "str", list(cell_list), (None if valid.all() else valid)
    if dtype == "i64":
        values = np.array([0 if c is None else int(c) for c in cell_list], np.int64)
    elif dtype == "f64":
        values = np.array([0.0 if c is None else float(c) for c in cell_list], np.float64)
    else:
        values = np.array([bool(c) for c in cell_list], bool)
    return dtype, values, (None if valid.all() else valid)


def take_col(col, idx):
    dtype, values, valid = col
    idx = np.asarray(idx, np.int64)
    out = [values[i] for i in idx] if dtype == "str" else np.asarray(values)[idx]
    return dtype, out, (None if valid is None else np.asarray(valid, bool)[idx])


def take_frame(frame, idx):
    return [take_col(c, idx) for c in frame]


def to_host(col):
    """The capi.Column an upload takes."""
    dtype, values, valid = col
    if dtype == "null":
        return Column.nulls(len(values))
    if dtype == "str":
        return Column.from_strings(values)
    return Column.from_numpy(values, valid)


def from_host(c):
    """A downloaded capi.Column as a model column."""
    dtype = DTYPE_OF_RV[c.dtype]
    if dtype == "null":
        return "null", np.zeros(c.length, np.int64), None
    if dtype == "str":
        return "str", c.to_strings(), c.logical_valid()
    return dtype, np.array(c.logical_values()), c.logical_valid()


def payload(col):
    """What two equal columns agree on, cell by cell: the 64 bits of a valid cell with every NaN one value, 0 under a null."""
    dtype, values, _ = col
    ok = valid_of(col)
    if dtype == "str":
        return [x if v else None for x, v in zip(values, ok)]
    if dtype == "null":
        return np.zeros(len(values), np.uint64)
    if dtype == "f64":
        bits = np.ascontiguousarray(values, np.float64).view(np.uint64).copy()
        bits[np.isnan(np.asarray(values, np.float64))] = CANONICAL_NAN
    elif dtype == "i64":
        bits = np.ascontiguousarray(values, np.int64).view(np.uint64).copy()
    else:
        bits = np.asarray(values, bool).astype(np.uint64)
    bits[~ok] = 0
    return bits


def column_diff(got, want):
    """None when `got` is `want` -- dtype, length, valid flags, bits of valid cells, strings -- else a text naming the first rows."""
    if got[0] != want[0]:
        return f"dtype {got[0]} != {want[0]}"
    if len(got[1]) != len(want[1]):
        return f"length {len(got[1])} != {len(want[1])}"
    gv, wv = valid_of(got), valid_of(want)
    bad = np.flatnonzero(gv != wv)
    if len(bad):
        return f"valid flags differ first at rows {bad[:5].tolist()}: got {gv[bad[:5]].tolist()}"
    a, b = payload(got), payload(want)
    if got[0] == "str":
        bad = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
        return None if not bad else f"strings differ first at rows {bad[:5]}: {[a[i] for i in bad[:5]]} != {[b[i] for i in bad[:5]]}"
    bad = np.flatnonzero(a != b)
    return None if not len(bad) else f"cells differ first at rows {bad[:5].tolist()}: bits {[hex(int(x)) for x in a[bad[:5]]]} != {[hex(int(x)) for x in b[bad[:5]]]}"


def frame_diff(got, want):
    if len(got) != len(want):
        return f"{len(got)} columns != {len(want)}"
    for j, (g, w) in enumerate(zip(got, want)):
        d = column_diff(g, w)
        if d:
            return f"column {j} ({w[0]}): {d}"
    return None


def tup(x):
    """Lists of a JSON file back into the tuples trees and terms are written as."""
    return tuple(tup(y) for y in x) if isinstance(x, (list, tuple)) else x


# ---- steps ---------------------------------------------------------------------------------------------------------------------------
def predicate_of(step):
    expr = step.get("expr")
    return Predicate([Term(int(c), op, lit) for c, op, lit in step["terms"]], step.get("nulls", "drops"), None if expr is None else tup(expr))


def predicate_columns(frame):
    """The frame as the capi.Columns helpers.host_survivors reads (String / Null columns are no predicate columns: a length alone)."""
    n = rows(frame)
    return [Column.from_numpy(c[1], c[2]) if c[0] in ("i64", "f64", "bool") else Column.nulls(n) for c in frame]


def survivors(frame, step):
    if rows(frame) == 0:
        return np.zeros(0, bool)
    return host_survivors(predicate_columns(frame), predicate_of(step))


def step_filter(frame, step):
    """filter_project over every column, and the mask path: both keep helpers.host_survivors' rows (a mask is policy "drops")."""
    return take_frame(frame, np.flatnonzero(survivors(frame, step)))


def compact_tree(tree, used):
    op, *args = tree
    if op == "col":
        return ("col", used.index(args[0]))
    if op == "lit":
        return ("lit", args[0])
    return (op, compact_tree(args[0], used), compact_tree(args[1], used))


def step_arith(frame, step):
    tree = tup(step["tree"])
    used = sorted(arith_model.columns_read(tree))
    dtype, out = arith_model.evaluate(compact_tree(tree, used), [RV[frame[k][0]] for k in used], [cells(frame[k]) for k in used])
    name = DTYPE_OF_RV[dtype]
    if name == "f64":  # (column_of would read a Python float cell the same way; this keeps a NaN's payload out of the question)
        col = ("f64", np.array([0.0 if x is None else x for x in out], np.float64), np.array([x is not None for x in out], bool))
    else:
        col = column_of(name, out)
    return list(frame) + [col]


def join_sides(frame, step, other):
    """(probe frame, its key, build frame, its key): the frame is the probe side unless the step says "side": "build".  Either way
    probe_key names the frame's key column and build_key the second frame's."""
    if step.get("side") == "build":
        return other, step["build_key"], frame, step["probe_key"]
    return frame, step["probe_key"], other, step["build_key"]


def join_pairs(probe, pk, build, bk):
    pairs = join_model.inner_join_pairs(RV[build[bk][0]], cells(build[bk]), RV[probe[pk][0]], cells(probe[pk]))
    out = join_model.materialize([("p", RV_INT64, range(rows(probe)))], [("k", RV_NULL, None), ("b", RV_INT64, range(rows(build)))], "k", pairs)
    return np.array(out[0][2], np.int64), np.array(out[1][2], np.int64)


def step_join(frame, step, other):
    probe, pk, build, bk = join_sides(frame, step, other)
    pi, bi = join_pairs(probe, pk, build, bk)
    return take_frame(probe, pi) + [take_col(c, bi) for j, c in enumerate(build) if j != bk]


def string_ids(col):
    """rv_string_dict_build's ids: the row of a string's first occurrence, null under a null."""
    first, ids = {}, np.zeros(len(col[1]), np.int64)
    ok = valid_of(col)
    for i, (x, v) in enumerate(zip(col[1], ok)):
        if v:
            ids[i] = first.setdefault(x, i)
    return "i64", ids, (None if ok.all() else ok)


def group_key(col):
    if col[0] == "str":
        col = string_ids(col)
    if col[0] == "null":
        return np.zeros(len(col[1]), np.int64), np.zeros(len(col[1]), bool)
    return col[1], col[2]


def group_result(frame, step):
    """group_agg_model.aggregate's dict for the step (gids and first_row included)."""
    columns = [(c[0] if c[0] in ("i64", "f64") else "other", c[1] if c[0] in ("i64", "f64") else None, valid_of(c)) for c in frame]
    return group_agg_model.aggregate(group_key(frame[step["key"]]), columns, [(op, c) for op, c in step["specs"]], exact_float=True)


def step_group(frame, step):
    res = group_result(frame, step)
    out = [take_col(frame[step["key"]], res["first_row"])]
    for dtype, bits, valid, _ in res["aggs"]:
        raw = np.array(bits, np.uint64) if len(bits) else np.zeros(0, np.uint64)
        out.append((dtype, raw.view(np.int64 if dtype == "i64" else np.float64), None if valid is None else np.array(valid, bool)))
    return out


def sort_columns(frame):
    return [(c[0], c[1], c[2]) if c[0] in ("i64", "f64", "null") else None for c in frame]


def step_sort(frame, step):
    return take_frame(frame, sort_model.sort_frame(sort_columns(frame), [(int(c), int(f)) for c, f in step["keys"]]))


def slice_bounds(n, step):
    off = min(step["offset"], n // 2)
    return off, max(0, n - off - step["tail"])


def reshape_indices(frame, step):
    n = rows(frame)
    how = step["how"]
    if how == "slice":
        off, length = slice_bounds(n, step)
        return np.arange(off, off + length)
    if how == "concat":
        h = n * step["eighths"] // 8
        return np.concatenate([np.arange(h, n), np.arange(0, h)])
    if how == "take_first":
        return group_agg_model.group_positions(*group_key(frame[step["col"]]))[1]
    assert how == "take_sorted"
    return sort_model.sort_indices(sort_columns(frame)[step["col"]], step["flags"])


def step_reshape(frame, step):
    return take_frame(frame, reshape_indices(frame, step))


def window_args(frame, step):
    """(columns, partition_by) as window_model.window takes them: a String partition key stands as its dictionary ids in an extra
    column behind the frame (the device runner appends the same column), every other column as it is."""
    cols = [(c[0], c[1], c[2]) for c in frame]
    part = []
    for c in step["partition_by"]:
        if frame[c][0] == "str":
            cols.append(string_ids(frame[c]))
            c = len(cols) - 1
        part.append(c)
    return cols, part


def model_column(dtype, values, valid):
    """A result column of window_model (Float64 as bit patterns, None for a Null column) as a frame column."""
    n = len(valid)
    if dtype == "null":
        return "null", np.zeros(n, np.int64), None
    if dtype == "f64":
        values = np.ascontiguousarray(values, np.uint64).view(np.float64)
    return dtype, values, (None if valid.all() else np.asarray(valid, bool))


def step_window(frame, step):
    cols, part = window_args(frame, step)
    out = window_model.window(cols, part, [(int(c), int(f)) for c, f in step["order_by"]], [tuple(e) for e in step["exprs"]], exact_float=True)
    return list(frame) + [model_column(*c) for c in out]


def topk_k(step, n):
    k = step["k"]
    if k[0] == "abs":
        return int(k[1])
    return max(0, n * k[1] // k[2] + (k[3] if len(k) > 3 else 0))


def topk_keys(step):
    keys = [(int(c), int(f)) for c, f in step["keys"]]
    return keys[:1] if step.get("via") == "indices" else keys


def topk_select(step, frame, select_from_rows, divisor):
    """topk_model.Select of the step's call: which path it takes over the first key, its passes and candidates."""
    c, flags = topk_keys(step)[0]
    return topk_model.select(sort_columns(frame)[c], flags, topk_k(step, rows(frame)), 1 if step.get("select") else select_from_rows, divisor)


def step_topk(frame, step):
    return take_frame(frame, topk_model.top_k_frame(sort_columns(frame), topk_keys(step), topk_k(step, rows(frame))))


def take_col_nullable(col, idx):
    """take_col with -1 for "no row": a null cell (rv_take_device_nullable)."""
    idx = np.asarray(idx, np.int64)
    there = idx >= 0
    if col[0] == "null":
        return "null", np.zeros(len(idx), np.int64), None
    if there.all():
        return take_col(col, idx)
    if len(col[1]) == 0:
        return column_of(col[0], [None] * len(idx))
    dtype, values, _ = take_col(col, np.where(there, idx, 0))
    return dtype, values, valid_of(col)[np.where(there, idx, 0)] & there


def outer_join_indices(probe, pk, build, bk, how):
    """outer_join_model.join_pairs as two index arrays, -1 for "no partner" """
    pairs = outer_join_model.join_pairs(HOW[how], RV[build[bk][0]], cells(build[bk]), RV[probe[pk][0]], cells(probe[pk]))
    pi = np.array([-1 if p is None else p for p, _ in pairs], np.int64)
    bi = np.array([-1 if b is None else b for _, b in pairs], np.int64)
    return pi, bi


def step_outer_join(frame, step, other):
    probe, pk, build, bk = join_sides(frame, step, other)
    how = step["how"]
    pi, bi = outer_join_indices(probe, pk, build, bk, how)
    out = [take_col_nullable(c, pi) for c in probe]
    if how in ("semi", "anti"):
        return out
    return out + [take_col_nullable(c, bi) for j, c in enumerate(build) if j != bk or how == "full"]


def group_keys_result(frame, step):
    """group_keys_model.aggregate's dict for the step"""
    n = rows(frame)
    keys = []
    for c in step["keys"]:
        col = string_ids(frame[c]) if frame[c][0] == "str" else frame[c]
        keys.append(("null", None, n) if col[0] == "null" else (col[0], col[1], col[2]))
    columns = [(c[0] if c[0] in ("i64", "f64") else "other", c[1] if c[0] in ("i64", "f64") else None, valid_of(c)) for c in frame]
    return group_keys_model.aggregate(keys, columns, [(op, c) for op, c in step["specs"]], exact_float=True)


def agg_columns(aggs):
    out = []
    for dtype, bits, valid, _ in aggs:
        raw = np.array(bits, np.uint64) if len(bits) else np.zeros(0, np.uint64)
        out.append((dtype, raw.view(np.int64 if dtype == "i64" else np.float64), None if valid is None else np.array(valid, bool)))
    return out


def step_group_keys(frame, step):
    res = group_keys_result(frame, step)
    return [take_col(frame[c], res["first_row"]) for c in step["keys"]] + agg_columns(res["aggs"])


def apply(step, frame, build=None):
    kind = step["kind"]
    if kind == "window":
        return step_window(frame, step)
    if kind == "topk":
        return step_topk(frame, step)
    if kind == "outer_join":
        return step_outer_join(frame, step, build)
    if kind == "group_keys":
        return step_group_keys(frame, step)
    if kind in ("filter", "mask"):
        return step_filter(frame, step)
    if kind == "arith":
        return step_arith(frame, step)
    if kind == "join":
        return step_join(frame, step, build)
    if kind == "group":
        return step_group(frame, step)
    if kind == "sort":
        return step_sort(frame, step)
    assert kind == "reshape", kind
    return step_reshape(frame, step)


# ---- what the header promises of a device column ---------------------------------------------------------------------------------------
def source_meta(frame, how="upload", offset=0):
    """upload / slice: the bitmap is attached exactly when the host had one (`valid` is not None, all True included), the null count is
    known only without one.  csv: a batch's column carries a bitmap iff the batch holds a null in it."""
    out = []
    for c in frame:
        if c[0] == "null":
            out.append({"bitmap": False, "known": True, "offset": None, "made": False})
        elif how == "csv":
            out.append({"bitmap": c[2] is not None, "known": None, "offset": None, "made": False})
        else:
            out.append({"bitmap": c[2] is not None, "known": c[2] is None, "offset": offset, "made": False})
    return out


def gathered_meta(col):
    """take / filter / concat / join / sort outputs: the builder drops a bitmap without nulls; null_count known; offset 0."""
    return {"bitmap": col[0] != "null" and null_count(col) > 0, "known": True, "offset": None if col[0] == "null" else 0, "made": True}


def meta_after(step, frame_in, meta_in, frame_out):
    kind = step["kind"]
    if kind == "arith":
        tree = tup(step["tree"])
        used = sorted(arith_model.columns_read(tree))
        has = [meta_in[k]["bitmap"] for k in used]
        bitmap = None
        if rows(frame_in) and None not in has:
            bitmap = arith_model.bitmap_expected(compact_tree(tree, used), [RV[frame_in[k][0]] for k in used], has)
        return list(meta_in) + [{"bitmap": bitmap, "known": True, "offset": None if frame_out[-1][0] == "null" else 0, "made": True}]
    if kind == "reshape" and step["how"] == "slice":
        off, _ = slice_bounds(rows(frame_in), step)
        out = []
        for c, m in zip(frame_in, meta_in):
            if c[0] == "null":
                out.append({"bitmap": False, "known": True, "offset": None, "made": m["made"]})
            else:
                out.append({"bitmap": m["bitmap"], "known": None if m["bitmap"] is None else not m["bitmap"],
                            "offset": None if m["offset"] is None else m["offset"] + off, "made": m["made"]})
        return out
    if kind == "window":  # rv_window, "Outputs": a bitmap iff some output cell is null, null_count known; passed-on columns as they were
        return list(meta_in) + [gathered_meta(c) for c in frame_out[len(meta_in):]]
    if kind in ("group", "group_keys"):
        nkeys = len(step["keys"]) if kind == "group_keys" else 1
        out = [gathered_meta(c) for c in frame_out[:nkeys]]
        for (op, _), col in zip(step["specs"], frame_out[nkeys:]):
            out.append({"bitmap": op in ("min", "max") and null_count(col) > 0, "known": True, "offset": 0, "made": True})  # attached iff some cell is null
        return out
    return [gathered_meta(c) for c in frame_out]


def touched(step, frame):
    """The input columns the step's device calls read."""
    kind = step["kind"]
    if kind == "arith":
        return sorted(arith_model.columns_read(tup(step["tree"])))
    if kind == "group":
        return sorted({step["key"]} | {c for _, c in step["specs"] if c is not None})
    if kind == "group_keys":
        return sorted(set(step["keys"]) | {c for _, c in step["specs"] if c is not None})
    if kind == "window":  # (the numbering ops ignore their column)
        read = {e[1] for e in step["exprs"] if e[0] not in ("row_number", "rank", "dense_rank")}
        return sorted(set(step["partition_by"]) | {c for c, _ in step["order_by"]} | read)
    return list(range(len(frame)))


def padded_after(step, frame, pads, build=None, build_pads=None):
    """Per output column the cells that are null because an "outer" / "full" join found no partner for the row, carried through every
    step that moves cells (a computed column starts without any).  pads: one bool array per input column; the index lists are the ones
    the step functions above use."""
    kind = step["kind"]
    n = rows(frame)
    none = lambda m: np.zeros(m, bool)
    if kind in ("arith", "window"):
        return list(pads) + [none(n) for _ in range(len(step["exprs"]) if kind == "window" else 1)]
    if kind == "group":
        first = group_result(frame, step)["first_row"]
        return [pads[step["key"]][first]] + [none(len(first)) for _ in step["specs"]]
    if kind == "group_keys":
        first = group_keys_result(frame, step)["first_row"]
        return [pads[c][first] for c in step["keys"]] + [none(len(first)) for _ in step["specs"]]
    if kind in JOINS:
        other = build_pads if build_pads is not None else [none(rows(build)) for _ in build]
        probe, pk, bcols, bk = join_sides(frame, step, build)
        ppads, bpads = (other, pads) if step.get("side") == "build" else (pads, other)
        how = step.get("how", "inner")
        pi, bi = join_pairs(probe, pk, bcols, bk) if kind == "join" else outer_join_indices(probe, pk, bcols, bk, how)
        pad = how in ("outer", "full")
        gather = lambda p, idx: np.where(idx >= 0, p[np.maximum(idx, 0)] if len(p) else False, pad)
        out = [gather(p, pi) for p in ppads]
        if how in ("semi", "anti"):
            return out
        return out + [gather(p, bi) for j, p in enumerate(bpads) if j != bk or how == "full"]
    if kind in ("filter", "mask"):
        idx = np.flatnonzero(survivors(frame, step))
    elif kind == "sort":
        idx = sort_model.sort_frame(sort_columns(frame), [(int(c), int(f)) for c, f in step["keys"]])
    elif kind == "topk":
        idx = topk_model.top_k_frame(sort_columns(frame), topk_keys(step), topk_k(step, n))
    else:
        idx = reshape_indices(frame, step)
    return [p[idx] for p in pads]


def padded_run(case, inter, builds):
    """[pads of every intermediate] of a case whose model intermediates are (inter, builds); the sources hold no padded cell."""
    def walk(steps, frames, seconds):
        pads = [np.zeros(rows(frames[0][0]), bool) for _ in frames[0][0]]
        out = [pads]
        for k, step in enumerate(steps):
            b = seconds.get(k) if step["kind"] in JOINS else None
            pads = padded_after(step, frames[k][0], pads, None if b is None else b[0], None if b is None else b[1])
            assert [len(p) for p in pads] == [rows(frames[k + 1][0])] * len(frames[k + 1][0])
            out.append(pads)
        return out
    seconds = {k: (builds[k][-1][0], walk(case["builds"][k]["steps"], builds[k], {})[-1]) for k in builds}
    return walk(case["steps"], inter, seconds)


def column_states(col, meta):
    """Which of the irregular states the issue lists a consumer's input column is in."""
    n = len(col[1])
    out = set()
    if n == 0:
        out.add("zero_rows")
    elif null_count(col) == n:
        out.add("all_null")
    if meta["known"] is False:
        out.add("null_count_unknown")
    if meta["bitmap"] is True and null_count(col) == 0 and n > 0:
        out.add("bitmap_no_nulls")
    return out


def run(sources, steps, builds=None):
    """Every intermediate of a pipeline: [(frame, meta)] with entry 0 the source and entry k + 1 the output of steps[k].
    sources: (frame, meta) of the main input; builds[k]: the run() of join step k's second frame."""
    frame, meta = sources
    out = [(frame, meta)]
    for k, step in enumerate(steps):
        build = builds[k][-1][0] if step["kind"] in JOINS else None
        nxt = apply(step, frame, build)
        if step["kind"] in JOINS:
            meta = [gathered_meta(c) for c in nxt]
        else:
            meta = meta_after(step, frame, meta, nxt)
        frame = nxt
        out.append((frame, meta))
    return out


def source_of(src):
    """(frame, meta) of a source of tests/pipeline_cases.py"""
    return src["frame"], source_meta(src["frame"], src["how"], src["pad"])


def run_case(case):
    """run() of a generated case, and of the second frames of its joins: (intermediates, {step index: intermediates of the build side})"""
    builds = {k: run(source_of(b["source"]), b["steps"]) for k, b in case["builds"].items()}
    return run(source_of(case["source"]), case["steps"], builds), builds
