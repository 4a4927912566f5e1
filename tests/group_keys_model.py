"""Model of group_by([k_0 .. k_{m-1}]).agg(...) as include/rivulus_gpu.h defines it (K9a: rv_hash_aggregate_keys, rv_group_ids_keys):
pure Python / numpy, nothing of the library.  A row's key is the tuple of its cells; this file only says when two cells are EQUAL and
turns every row's tuple into a dense code by first occurrence.  The aggregates and every numeric rule are tests/group_agg_model.py's:
aggregate() hands it the codes as a single Int64 key without nulls.

A key column is (dtype, values, valid): dtype one of "i64", "f64", "bool", "null"; values a numpy array (int64 / float64 / bool; None
for "null"); valid a bool array or None (no nulls).  For "null" give the row count in place of valid: ("null", None, n).
"""
import numpy as np

import group_agg_model as M

CANONICAL_NAN = M.CANONICAL_NAN


def cells(dtype, values, valid, n):
    """(word[n] uint64, null[n] bool): what equality looks at.  A null has no word (0 here: what lies under it is never read); Int64:
    the bits; Float64: the bits, every NaN the canonical pattern (so -0.0 and +0.0 stay apart); Boolean: 0 or 1."""
    if dtype == "null":
        return np.zeros(n, np.uint64), np.ones(n, bool)
    null = np.zeros(n, bool) if valid is None else ~np.asarray(valid, bool)
    if dtype == "bool":
        word = np.asarray(values, bool).astype(np.uint64)
    else:
        word = np.ascontiguousarray(values).view(np.uint64).copy()
        if dtype == "f64":
            word[(word & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000)] = np.uint64(CANONICAL_NAN)
    word[null] = 0
    return word, null


def cell(dtype, values, valid, i):
    """one cell: None for a null, else its word as an int"""
    n = int(valid) if dtype == "null" else len(values)
    word, null = cells(dtype, values, None if dtype == "null" else valid, n)
    return None if null[i] else int(word[i])


def rows_of(keys):
    dtype, values, valid = keys[0]
    return int(valid) if dtype == "null" else len(values)


def codes(keys):
    """(codes[n] int64, first_row[G]): every row's tuple as a dense code by first occurrence."""
    n = rows_of(keys)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    table = np.empty((n, 2 * len(keys)), np.uint64)
    for k, (dtype, values, valid) in enumerate(keys):
        word, null = cells(dtype, values, None if dtype == "null" else valid, n)
        table[:, 2 * k], table[:, 2 * k + 1] = word, null
    _, first, inverse = np.unique(table, axis=0, return_index=True, return_inverse=True)  # index: the first occurrence
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    return rank[np.asarray(inverse).reshape(-1)], first[order].astype(np.int64)


def aggregate(keys, columns, specs, exact_float=False):
    """group_agg_model.aggregate over the codes, plus key_cells: per key column the cells AS STORED at the groups' first rows -- None
    for a null, else the bits (a NaN keeps the first row's own bits; compare through M.canonical)."""
    c, first = codes(keys)
    out = M.aggregate((c, None), columns, specs, exact_float=exact_float)
    assert np.array_equal(out["first_row"], first) and np.array_equal(out["gids"], c)  # codes by first occurrence ARE the positions
    out["key_cells"] = []
    for dtype, values, valid in keys:
        if dtype == "null":
            out["key_cells"].append([None] * len(first))
            continue
        stored = np.asarray(values, bool).astype(np.uint64) if dtype == "bool" else np.ascontiguousarray(values).view(np.uint64)
        ok = np.ones(len(first), bool) if valid is None else np.asarray(valid, bool)[first]
        out["key_cells"].append([int(b) if v else None for b, v in zip(stored[first].tolist(), ok.tolist())])
    return out


# ---- cells as tests/golden/group_keys_cases.json writes them ----------------------------------------------------------------------
def key_column_of(dtype, cells, rows):
    """(dtype, values, valid) of a JSON cell list: null -> None; Float64 cells are numbers, "nan" / "inf" / "-inf" / "-0.0" or
    "bits:0x..." (a pattern typed out, for NaN payloads); Boolean cells true / false; a "null" column has no cell list."""
    if dtype == "null":
        return "null", None, rows
    valid = np.array([c is not None for c in cells], bool)
    if dtype == "i64":
        values = np.array([0 if c is None else c for c in cells], np.int64)
    elif dtype == "bool":
        values = np.array([bool(c) for c in cells], bool)
    else:
        bits = [0 if c is None else int(c[5:], 16) if isinstance(c, str) and c.startswith("bits:") else int(np.array([float(c)], np.float64).view(np.uint64)[0])
                for c in cells]
        values = np.array(bits, np.uint64).view(np.float64)
    return dtype, values, (None if valid.all() else valid)


def expected_key_cells(dtype, cells):
    """the canonical form of a JSON list of expected key cells"""
    out = []
    for c in cells:
        if c is None:
            out.append(None)
        elif dtype == "bool":
            out.append(int(bool(c)))
        elif dtype == "f64":
            out.append(M.canonical("f64", int(c[5:], 16) if isinstance(c, str) and c.startswith("bits:") else M.float_bits(c)))
        else:
            out.append(int(c))
    return out


def canonical_key_cells(dtype, cells):
    """aggregate()'s key_cells of one column as tests compare them: Int64 signed, Float64 with every NaN canonical"""
    if dtype in ("i64", "f64"):
        return [None if c is None else M.canonical(dtype, c) for c in cells]
    return cells
