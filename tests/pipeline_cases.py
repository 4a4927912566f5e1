"""Deterministic generator of operator pipelines: case(seed) -> the source frames and 2 to 5 steps (tests/pipeline_model.py's step dicts).

The step list follows from the seed and the schema alone -- dtypes and the per-column hints below, never the cells -- so the cases can be
listed, counted and run through the model on a machine without a device.  The first two step kinds walk through all 49 ordered pairs
(seed % 49); the rest is drawn.  Every frame keeps an Int64 column, so every step kind type-checks after every other.

A schema is one dict per column:
  dtype    "i64" | "f64" | "bool" | "str" | "null"
  dom      (lo, hi): the non-null cells lie in [lo, hi), which is how a predicate aims at a selectivity; None: unknown
  sum      Float64: every cell is k * 2^-10 with |k| < 2^20 (helpers.dyadic_cells), or a sum of such: a SUM over it is exact in any order
  special  Float64 that may hold +-inf / NaN / -0.0: a sort key and a MIN / MAX input, never summed, never read by a predicate
  dead     every cell of the source column was drawn null: predicates and join keys mostly look elsewhere (a cap on empty results)
  full     the column carries a bitmap and no null (an upload with an all-valid bitmap, what arith computes from such, slices of both)
  fresh    full, and rv_eval_arith wrote it: arith operands and group keys / arguments lean towards these, so that the state "bitmap
           attached, zero nulls" reaches consumers on columns an operator made
"""
import collections
import math

import numpy as np

import arith_model
from helpers import const, dyadic_cells
import pipeline_model
from pipeline_model import KINDS, RV

TILE = 256 * const("kSortRowsPerLane")
SIZES = (0, 1, 63, 64, 65, TILE - 1, TILE + 1, 2 * TILE + 1, 4096, 20_011)
SIZE_P = (0.03, 0.07, 0.08, 0.08, 0.08, 0.14, 0.13, 0.13, 0.13, 0.13)
LARGE = 70_003
NULL_SHARES = (0.0, 0.05, 0.5, 1.0)
SELECTIVITIES = (0.0, 0.1, 0.5, 0.9, 1.0)
SELECTIVITY_P = (0.03, 0.17, 0.3, 0.3, 0.2)
PAD = (1, 63, 65)
WORDS = ["a", "ab", "Bob", "Ünï", "zz", "名前", "x" * 40, "q"]
SPECIALS = (0.0, -0.0, math.inf, -math.inf, math.nan)
SCALE = -10


def _col(dtype, dom=None, summable=False, special=False, dead=False):
    return {"dtype": dtype, "dom": dom, "sum": summable, "special": special, "dead": dead, "full": False, "fresh": False}


# ---- source frames -----------------------------------------------------------------------------------------------------------------
def _valid(rng, total, share, csv, whole=False):
    if share == 0.0:
        return np.ones(total, bool) if (not csv and (rng.random() < 0.6 or whole)) else None  # a bitmap without a null: attached all the same
    return rng.random(total) >= share


def _make_column(rng, dtype, total, n, csv, whole=False):
    """(schema entry, column of `total` rows); whole: no null, and a bitmap attached all the same"""
    share = float(rng.choice(NULL_SHARES, p=(0.4, 0.25, 0.2, 0.15)))
    if whole:
        share = 0.0
    if dtype == "null":
        return _col("null"), ("null", np.zeros(total, np.int64), None)
    if dtype == "i64":
        card = int(rng.choice([1, 2, 7, 100, max(1, n)]))
        return _col("i64", (0, card)), ("i64", rng.integers(0, card, total, dtype=np.int64), _valid(rng, total, share, csv, whole))
    if dtype == "f64":
        _, values, valid = dyadic_cells(int(rng.integers(0, 1 << 30)), total, SCALE, 0.0 if csv else share)
        if csv and share:
            valid = rng.random(total) >= share
        if valid is None:
            valid = _valid(rng, total, 0.0, csv, whole)
        if rng.random() < 0.5 and not csv:
            hit = rng.random(total) < 0.1
            values[hit] = np.array(SPECIALS)[rng.integers(0, len(SPECIALS), int(hit.sum()))]
            return _col("f64", None, False, True), ("f64", values, valid)
        return _col("f64", (-1024.0, 1024.0), True), ("f64", values, valid)
    if dtype == "bool":
        return _col("bool"), ("bool", rng.random(total) < float(rng.choice([0.1, 0.5, 0.9])), _valid(rng, total, share, csv))
    card = int(rng.choice([1, 3, 50, max(1, n)]))
    valid = _valid(rng, total, share, csv)
    ids = rng.integers(0, card, total)
    words = [WORDS[k % len(WORDS)] + (str(k // len(WORDS)) if k >= len(WORDS) else "") for k in ids]
    if not csv:
        words = ["" if k == 1 and card > 2 else w for k, w in zip(ids, words)]  # "" is a value, not a null (a CSV cell "" is a null)
    if valid is not None:
        words = [w if v else None for w, v in zip(words, valid)]
    return _col("str"), ("str", words, valid)


def _cut(col, a, n):
    dtype, values, valid = col
    return dtype, values[a:a + n], (None if valid is None else valid[a:a + n])


def _csv_text(frame):
    lines = [",".join(f"c{j}" for j in range(len(frame)))]
    cols = []
    for dtype, values, valid in frame:
        ok = np.ones(len(values), bool) if valid is None else valid
        if dtype == "bool":
            cols.append([("true" if x else "false") if v else "" for x, v in zip(values, ok)])
        elif dtype == "str":
            cols.append([x if v else "null" for x, v in zip(values, ok)])
        else:
            cols.append([repr(x) if v else "" for x, v in zip(values.tolist(), ok)])
    lines += [",".join(row) for row in zip(*cols)]
    return "\n".join(lines) + "\n"


def _csv_frame(frame, as_reference):
    """The batch the reader hands out: no bitmap without a null, 0 under a null, and with nulls_as_reference the reference's defect:
    an Int64 / Float64 column that holds a null comes out with every validity bit inverted (include/rivulus_gpu.h, rv_csv_open)."""
    out = []
    for dtype, values, valid in frame:
        if valid is None or valid.all():
            out.append((dtype, values, None))
        elif dtype in ("i64", "f64"):
            zeroed = np.where(valid, values, 0).astype(values.dtype)
            out.append((dtype, zeroed, ~valid if as_reference else valid))
        else:
            out.append((dtype, values, valid))
    return out


def _source(rng, dtypes, n, how, whole=()):
    """{"how", "frame": the logical n rows, "padded": what is uploaded before the slice, "pad", "ref", "text"} and its schema."""
    pad = int(rng.choice(PAD)) if how == "slice" else 0
    total = n + (pad + int(rng.integers(1, 9)) if how == "slice" else 0)
    schema, padded = [], []
    for dtype in dtypes:
        s, c = _make_column(rng, dtype, total, n, how == "csv", len(schema) in whole)
        s["dead"] = c[0] != "null" and c[2] is not None and not c[2].any()
        s["full"] = how != "csv" and c[0] != "null" and c[2] is not None and bool(c[2].all())
        schema.append(s)
        padded.append(c)
    frame = [_cut(c, pad, n) for c in padded]
    src = {"how": how, "frame": frame, "padded": padded, "pad": pad, "ref": False, "text": None}
    if how == "csv":
        src["ref"] = bool(rng.random() < 0.5)
        src["text"] = _csv_text(frame)
        src["frame"] = _csv_frame(frame, src["ref"])
        for s, c in zip(schema, src["frame"]):
            if s["dtype"] == "i64" and src["ref"] and c[2] is not None:
                s["dom"] = None  # (the cells that are valid now all hold 0)
    return src, schema


# ---- steps -------------------------------------------------------------------------------------------------------------------------
def _pick(rng, items):
    return items[int(rng.integers(0, len(items)))]


def _term(rng, schema, sel, allow_bool):
    cand = [j for j, c in enumerate(schema) if c["dtype"] in ("i64", "f64") and not c["special"]]
    if rng.random() < 0.9:
        cand = [j for j in cand if not schema[j]["dead"]] or cand
    known = [j for j in cand if schema[j]["dom"] is not None]
    if known and rng.random() < 0.8:
        cand = known
    if allow_bool and rng.random() < 0.25:
        cand = [j for j, c in enumerate(schema) if c["dtype"] == "bool"] or cand
    j = _pick(rng, cand)
    c = schema[j]
    if c["dtype"] == "bool":
        return (j, "is_true", None)
    is_float = c["dtype"] == "f64"
    if c["dom"] is None:
        if sel == 0.0:
            return (j, "<", -1e300 if is_float else -(1 << 62))
        return (j, "!=", 3.0 if is_float else 3)
    lo, hi = c["dom"]
    if sel == 1.0:
        return (j, ">=", lo)
    thr = lo + sel * (hi - lo)
    return (j, "<", float(thr) if is_float else int(math.ceil(thr)))


def _predicate(rng, schema, mask):
    sel = float(rng.choice(SELECTIVITIES, p=SELECTIVITY_P))
    terms = [_term(rng, schema, sel, not mask)]
    expr = None
    r = rng.random()
    if r < 0.35:
        terms.append(_term(rng, schema, 0.9, not mask))
        expr = None if r < 0.2 else ("or", 0, 1)
    elif r < 0.45 and sel not in (0.0, 1.0):
        terms[0] = _term(rng, schema, 1.0 - sel, not mask)  # NOT turns the share round
        dom = schema[terms[0][0]]["dom"]
        if dom is not None and dom[1] - dom[0] >= 7:  # (a domain of one or two values has no 10 % to aim at)
            expr = ("not", 0)
        else:
            terms[0] = _term(rng, schema, sel, not mask)
    return terms, expr


def _step_filter(rng, schema):
    terms, expr = _predicate(rng, schema, False)
    nulls = "least" if rng.random() < 0.3 and all(t[1] != "is_true" for t in terms) else "drops"
    step = {"kind": "filter", "terms": terms, "nulls": nulls, "expr": expr, "via": "selection" if rng.random() < 0.3 else "project"}
    return step, [dict(c) for c in schema]


def _step_mask(rng, schema):
    terms, expr = _predicate(rng, schema, True)
    return {"kind": "mask", "terms": terms, "expr": expr}, [dict(c) for c in schema]


def _literal(rng, dtype):
    return _pick(rng, [0.5, -2.0, 0.0]) if dtype == "f64" else _pick(rng, [3, -2, 0, 7])


def _step_arith(rng, schema, plain=False):
    """plain: an expression over columns with a bitmap and no null, without an Int64 division or a Null leaf -- its result is `fresh`"""
    num = [j for j, c in enumerate(schema) if c["dtype"] in ("i64", "f64")]
    nul = [j for j, c in enumerate(schema) if c["dtype"] == "null"]
    lean = [j for j in num if schema[j]["fresh"]] if rng.random() < 0.85 else []
    lean = lean or ([j for j in num if schema[j]["full"]] if rng.random() < 0.6 or plain else [])
    a, b = ("col", _pick(rng, lean or num)), ("col", _pick(rng, lean or num))
    lit = ("lit", _literal(rng, schema[a[1]]["dtype"]))
    t = int(rng.integers(1, 4) if plain else rng.integers(0, 6))
    if t == 0:
        tree = ("/", a, b)
    elif t == 1:
        tree = ("+", ("*", a, lit), b)
    elif t == 2:
        tree = ("-", a, lit)
    elif t == 3:
        tree = ("*", a, b)
    elif t == 4:
        tree = ("/", a, lit)
    else:
        tree = ("+", a, ("col", _pick(rng, nul)) if nul else ("lit", None))
    dtype = {v: k for k, v in RV.items()}[arith_model.tree_dtype(tree, [RV[c["dtype"]] for c in schema])]
    new = _col(dtype, None, False, dtype == "f64")
    whole = all(schema[j]["full"] for j in arith_model.columns_read(tree))
    new["full"] = new["fresh"] = whole and dtype != "null" and not arith_model.has_null_leaf(tree, [RV[c["dtype"]] for c in schema]) \
        and not arith_model.has_int_div(tree, [RV[c["dtype"]] for c in schema])
    return {"kind": "arith", "tree": tree}, [dict(c) for c in schema] + [new]


def _step_group(rng, schema):
    keys = [j for j, c in enumerate(schema) if c["dtype"] == "i64"]
    keys = [j for j in keys if schema[j]["dom"] is not None] or keys
    strs = [j for j, c in enumerate(schema) if c["dtype"] == "str"]
    key = _pick(rng, strs) if strs and rng.random() < 0.3 else _pick(rng, keys)
    fresh = [j for j, c in enumerate(schema) if c["fresh"]]
    if fresh and schema[fresh[-1]]["dtype"] == "i64" and rng.random() < 0.6:
        key = fresh[-1]
    options = [("count_rows", None)] + [("count", j) for j in range(len(schema))]
    for j, c in enumerate(schema):
        if c["dtype"] == "i64" or (c["dtype"] == "f64" and c["sum"]):
            options.append(("sum", j))
        if c["dtype"] in ("i64", "f64"):
            options += [("min", j), ("max", j)] * 2
    specs = [_pick(rng, options) for _ in range(int(rng.integers(1, 4)))]
    if fresh:
        specs[0] = (_pick(rng, ["min", "max"] + (["sum"] if schema[fresh[-1]]["dtype"] == "i64" else [])), fresh[-1])
    if schema[key]["dtype"] == "str":
        specs = [("count_rows", None)] + specs[:2]  # every frame keeps an Int64 column
    out = [dict(schema[key])]
    for op, j in specs:
        if op in ("count_rows", "count"):
            out.append(_col("i64"))
        elif op == "sum":
            out.append(_col(schema[j]["dtype"], None, schema[j]["sum"]))
        else:
            out.append(dict(schema[j]))
    return {"kind": "group", "key": key, "specs": specs}, out


def _sortable(schema):
    return [j for j, c in enumerate(schema) if c["dtype"] in ("i64", "f64", "null")]


def _step_sort(rng, schema):
    cand = _sortable(schema)
    keys = [(_pick(rng, cand), int(rng.integers(0, 4))) for _ in range(int(rng.integers(1, 3)))]
    return {"kind": "sort", "keys": keys, "via": "chain" if rng.random() < 0.4 else "sort"}, [dict(c) for c in schema]


def _step_reshape(rng, schema):
    how = _pick(rng, ["slice", "slice", "slice", "concat", "take_first", "take_sorted"])
    if how == "slice":
        step = {"kind": "reshape", "how": how, "offset": int(rng.choice(PAD)), "tail": int(rng.integers(0, 2))}
    elif how == "concat":
        step = {"kind": "reshape", "how": how, "eighths": int(rng.choice([1, 3, 4, 7]))}
    elif how == "take_first":
        step = {"kind": "reshape", "how": how, "col": _pick(rng, [j for j, c in enumerate(schema) if c["dtype"] in ("i64", "null")])}
    else:
        step = {"kind": "reshape", "how": how, "col": _pick(rng, _sortable(schema)), "flags": int(rng.integers(0, 4))}
    return step, [dict(c) for c in schema]


def _step_join(rng, schema):
    """The frame probes a small second frame whose keys are drawn from the probe key's domain, every key at most three times and at most
    two null keys: a join multiplies the rows by three at the most.  Three times in ten the sides are swapped: the frame -- columns an
    operator wrote -- is the side that is hashed."""
    keys = [j for j, c in enumerate(schema) if c["dtype"] == "i64"]
    keys = [j for j in keys if schema[j]["dom"] is not None] or keys
    if rng.random() < 0.9:
        keys = [j for j in keys if not schema[j]["dead"]] or keys
    pk = _pick(rng, keys)
    lo, hi = schema[pk]["dom"] or (0, 8)
    card = max(1, hi - lo)
    side = "build" if rng.random() < 0.3 else "probe"
    m = min(int(rng.choice([0, 1, 5, 64, 300], p=(0.02, 0.08, 0.2, 0.3, 0.4))), 3 * card)
    if side == "build":
        m = min(max(m, 1), 5)  # the frame is hashed and the second frame probes it: at most five times the frame's rows come out
    dts = ["i64"] + [str(rng.choice(["i64", "f64", "bool", "str", "null"])) for _ in range(int(rng.integers(1, 4)))]
    src, bschema = _source(rng, dts, m, "slice" if rng.random() < 0.3 else "upload")
    keyvals = lo + rng.permutation(m) % card
    valid = None
    if (m >= 3 and rng.random() < 0.4) or (m and schema[pk]["dead"]):  # (an all-null probe key meets the null build keys)
        valid = np.ones(m, bool)
        valid[rng.integers(0, m, 2)] = False
    full = src["padded"][0]
    kfull = np.array(full[1])
    kfull[src["pad"]:src["pad"] + m] = keyvals
    vfull = None
    if valid is not None:
        vfull = np.ones(len(kfull), bool)
        vfull[src["pad"]:src["pad"] + m] = valid
    src["padded"][0] = ("i64", kfull, vfull)
    src["frame"][0] = _cut(src["padded"][0], src["pad"], m)
    bschema[0] = _col("i64", (lo, hi))
    bsteps = []
    r = rng.random()
    if r < 0.2:
        bsteps.append({"kind": "filter", "terms": [(0, "<", lo + int(math.ceil(0.9 * card)))], "nulls": "least", "expr": None, "via": "project"})
    elif r < 0.35:
        step, bschema = _step_sort(rng, bschema)
        bsteps.append(step)
    elif r < 0.5:
        step, bschema = _step_arith(rng, bschema)
        bsteps.append(step)
    step = {"kind": "join", "probe_key": pk, "build_key": 0, "chunked": bool(rng.random() < 0.4), "side": side}
    if side == "build":
        return step, [dict(c) for c in bschema] + [dict(c) for j, c in enumerate(schema) if j != pk], {"source": src, "steps": bsteps}
    return step, [dict(c) for c in schema] + [dict(c) for c in bschema[1:]], {"source": src, "steps": bsteps}


MAKERS = {"filter": _step_filter, "mask": _step_mask, "arith": _step_arith, "group": _step_group, "sort": _step_sort, "reshape": _step_reshape}


EMPTY_SEEDS = (50, 56)  # filter -> mask and mask -> filter over a table without rows


def case(seed):
    """{"seed", "n", "source", "steps", "builds": {step index: {"source", "steps"}}}"""
    rng = np.random.default_rng(424_200 + seed)
    how = "csv" if seed % 10 == 3 else "slice" if seed % 10 in (1, 5, 8) else "upload"
    n = int(rng.choice(SIZES, p=SIZE_P))
    if seed % 40 == 7:
        n = LARGE
    if how == "csv":
        n = int(rng.choice([257, 300, 511]))
    a, b = divmod(seed % 49, 7)
    steer = KINDS[a] == "arith"  # arith -> every kind: the first step computes a column with a bitmap and no null for the second
    if steer and how == "csv":
        how = "upload"
    if seed in EMPTY_SEEDS:
        n = 0
    pool = ["i64", "f64", "bool", "str"] + ([] if how == "csv" else ["null"])
    dts = ["i64"] + [str(rng.choice(pool)) for _ in range(int(rng.integers(1, 6)))]
    if steer:
        dts[1] = ("i64", "f64")[seed % 2]
    source, schema = _source(rng, dts, n, how, (0, 1) if steer else ())
    kinds = [KINDS[a], KINDS[b]] + [str(rng.choice(KINDS)) for _ in range(int(rng.integers(0, 4)))]
    steps, builds, joins = [], {}, 0
    for kind in kinds:
        if kind == "join" and joins == 2:
            kind = "sort"
        if kind == "arith" and n == LARGE and any(s["kind"] == "arith" for s in steps):
            kind = "sort"  # the Python cell loop of arith_model: one large arith step per case
        if kind == "join":
            joins += 1
            step, schema, build = _step_join(rng, schema)
            builds[len(steps)] = build
        elif kind == "arith":
            step, schema = _step_arith(rng, schema, steer and not steps)
        else:
            step, schema = MAKERS[kind](rng, schema)
        if kind != "arith" and not (kind == "reshape" and step["how"] == "slice"):
            for c in schema:  # every other producer gathers: a bitmap without nulls is dropped
                c["full"] = c["fresh"] = False
        steps.append(step)
    return {"seed": seed, "n": n, "source": source, "steps": steps, "builds": builds}


# ---- the second generator: window, top-k, outer / semi / anti joins and multi-key grouping among the older kinds ---------------------
# case() above and everything it calls stay as they are (tests/golden/pipeline_cases_digest.json pins the 200 default cases); the makers
# below read three more schema hints, set by them alone:
#   padded  an "outer" / "full" join may have put nulls into the column (the side that can lack a partner)
#   holes   an operator wrote the column and it may hold nulls (a quotient, a padded column, a MIN / MAX, a LAG / LEAD): top-k first
#           keys lean towards these
#   far     a LAG / LEAD beyond every partition wrote the column: every cell is null
NEW_KINDS = pipeline_model.NEW_KINDS
KINDS_ALL = pipeline_model.KINDS_ALL
PAIRS_OPS = [(a, b) for a in KINDS_ALL for b in KINDS_ALL if a in NEW_KINDS or b in NEW_KINDS]  # 72 ordered pairs
HOWS = ("outer", "full", "semi", "anti")
FAR = 1 << 20  # a LAG / LEAD offset larger than any partition (the largest frame is LARGE rows times two joins)
TOPK_K = (["abs", 1], ["abs", 7], ["of", 1, 8, 1], ["of", 1, 2, -1], ["of", 1, 2], ["of", 1, 1], ["of", 1, 1, 5])  # (rows / 8 + 1: a small frame keeps a row)
TOPK_K_P = (0.17, 0.2, 0.25, 0.1, 0.08, 0.1, 0.1)


def _lean(rng, cand, schema, hints, p=0.85):
    """cand, or with probability p those of it that carry one of `hints` (if any does)"""
    if rng.random() < p:
        for h in hints:
            sub = [j for j in cand if schema[j].get(h)]
            if sub:
                return sub
    return cand


def _passed_on(c, **hints):
    out = dict(c)
    out.update({"full": False, "fresh": False}, **hints)
    return out


def _step_window(rng, schema):
    hints = ("padded", "fresh", "full")
    parts = [j for j, c in enumerate(schema) if c["dtype"] in ("i64", "f64", "bool", "null", "str")]
    order = _sortable(schema)
    small = [j for j in parts if schema[j]["dtype"] != "i64" or (schema[j]["dom"] is not None and schema[j]["dom"][1] - schema[j]["dom"][0] <= 100)]
    partition_by = [_pick(rng, _lean(rng, small or parts, schema, hints, 0.6)) for _ in range(int(rng.choice([0, 1, 1, 1, 2])))]
    order_by = [(_pick(rng, _lean(rng, order, schema, hints, 0.6)), int(rng.integers(0, 4))) for _ in range(int(rng.choice([0, 1, 1, 2])))]
    options = [("row_number", 0), ("rank", 0), ("dense_rank", 0)]
    for j, c in enumerate(schema):
        options.append(("cum_count", j))
        options += [(_pick(rng, ["lag", "lead"]), j, int(rng.choice([0, 1, 2, FAR])))]
        if c["dtype"] == "i64" or (c["dtype"] == "f64" and c["sum"]):
            options.append(("cum_sum", j))
        if c["dtype"] in ("i64", "f64"):
            options += [("cum_min", j), ("cum_max", j)]
    exprs = [_pick(rng, options) for _ in range(int(rng.integers(1, 5)))]
    reads = _lean(rng, list(range(len(schema))), schema, hints, 1.0)
    if reads != list(range(len(schema))):  # one expression over a column in a state worth meeting
        j = _pick(rng, reads)
        ops = ["cum_count", "lag", "lead"] + (["cum_min", "cum_max", "cum_sum"] if schema[j]["dtype"] == "i64" else ["cum_min", "cum_max"] if schema[j]["dtype"] == "f64" else [])
        op = _pick(rng, ops)
        exprs[0] = (op, j, int(rng.choice([0, 1, 2, FAR]))) if op in ("lag", "lead") else (op, j)
    out = [dict(c) for c in schema]  # the frame's columns are passed on untouched
    for e in exprs:
        src = schema[e[1]]
        if e[0] in ("row_number", "rank", "dense_rank", "cum_count"):
            out.append(_col("i64"))
        elif e[0] == "cum_sum":
            out.append(_col(src["dtype"]))  # not summable: no later SUM or CUM_SUM reads it
        else:
            out.append(_passed_on(src, sum=False, holes=True, padded=False, far=len(e) > 2 and e[2] == FAR))
    return {"kind": "window", "partition_by": partition_by, "order_by": order_by, "exprs": exprs}, out


def _step_topk(rng, schema, tiny=False, none=False, holes=False):
    """tiny: the source has at most two rows -- no k that rounds to 0; none: k = 0 (two of the default seeds); holes: the select, forced,
    over a first key an operator wrote nulls into if the frame has one -- nulls last and a small k, so that it runs whatever their number"""
    cand = _sortable(schema)
    wide = [j for j in cand if schema[j]["dtype"] == "f64" or (schema[j]["dtype"] == "i64" and (schema[j]["dom"] is None or schema[j]["dom"][1] - schema[j]["dom"][0] >= 100))]
    first = _pick(rng, _lean(rng, _lean(rng, cand, schema, ("holes",), 0.7), schema, ("padded", "fresh", "full"), 0.5)) if rng.random() < 0.6 else _pick(rng, wide or cand)
    keys = [(first, int(rng.integers(0, 4)))]
    via = "indices" if rng.random() < 0.3 else "frame"
    if via == "frame" and rng.random() < 0.5:
        keys.append((_pick(rng, cand), int(rng.integers(0, 4))))
    k = list(TOPK_K[int(rng.choice(len(TOPK_K), p=TOPK_K_P))])
    if tiny and k[0] == "of" and k[2] == 2:
        k = ["abs", 1]
    if none:
        k = ["abs", 0]
    made = [j for j in cand if schema[j].get("holes")]
    if holes and made and not none:
        keys[0] = (_pick(rng, made), 2 + int(rng.integers(0, 2)))
        first, k = keys[0][0], [["abs", 1], ["abs", 7]][int(rng.integers(0, 2))]
    step = {"kind": "topk", "keys": keys, "k": k, "via": via, "select": bool(rng.random() < 0.7) or (holes and bool(made))}
    out = [_passed_on(c) for c in schema]
    out[first]["dom"] = None  # the rows that stay are one end of the key's domain
    return step, out


def _step_outer_join(rng, schema, how=None, side=None, least=0):
    """_step_join for the other kinds.  The second frame's keys cover the upper half of the probe key's domain and as much again above it:
    whatever `how`, some probe rows find a partner and some do not, and some rows of the second frame meet nobody (what FULL appends)."""
    how = how or str(rng.choice(HOWS))
    keys = [j for j, c in enumerate(schema) if c["dtype"] == "i64"]
    keys = [j for j in keys if schema[j]["dom"] is not None] or keys
    if rng.random() < 0.9:
        keys = [j for j in keys if not schema[j]["dead"]] or keys
        keys = [j for j in keys if schema[j]["dom"] is not None and schema[j]["dom"][1] - schema[j]["dom"][0] >= 2] or keys  # one value: every row matches
    pk = _pick(rng, _lean(rng, keys, schema, ("padded", "fresh"), 0.5))
    lo, hi = schema[pk]["dom"] or (0, 8)
    card = max(1, hi - lo)
    side = side or ("build" if rng.random() < 0.3 else "probe")
    m = min(int(rng.choice([0, 1, 5, 64, 300], p=(0.02, 0.04, 0.1, 0.34, 0.5))), 3 * card)
    m = max(m, min(least, 3 * card))
    if side == "build":
        m = min(max(m, 2), 5)
    dts = ["i64", str(rng.choice(["i64", "f64"]))] + [str(rng.choice(["i64", "f64", "bool", "str", "null"])) for _ in range(int(rng.integers(0, 3)))]
    src, bschema = _source(rng, dts, m, "slice" if rng.random() < 0.3 else "upload")
    first = hi - (m + 1) // 2 if side == "build" else lo + card // 2  # (the few rows that probe the frame straddle its domain's end)
    keyvals = first + rng.permutation(m) % card
    valid = None
    if m >= 3 and rng.random() < 0.4:
        valid = np.ones(m, bool)
        valid[rng.integers(0, m, 2)] = False
    kfull = np.array(src["padded"][0][1])
    kfull[src["pad"]:src["pad"] + m] = keyvals
    vfull = None
    if valid is not None:
        vfull = np.ones(len(kfull), bool)
        vfull[src["pad"]:src["pad"] + m] = valid
    src["padded"][0] = ("i64", kfull, vfull)
    src["frame"][0] = _cut(src["padded"][0], src["pad"], m)
    bschema[0] = _col("i64", (first, first + card))
    bsteps = []
    r = rng.random()
    if r < 0.15:
        step, bschema = _step_sort(rng, bschema)
        bsteps.append(step)
    elif r < 0.3:
        step, bschema = _step_arith(rng, bschema)
        bsteps.append(step)
    step = {"kind": "outer_join", "how": how, "probe_key": pk, "build_key": 0, "chunked": bool(how != "full" and rng.random() < 0.4), "side": side}
    mine, other = [dict(c) for c in schema], [dict(c) for c in bschema]
    probe, build, bk = (other, mine, pk) if side == "build" else (mine, other, 0)
    if how in ("semi", "anti"):
        return step, [_passed_on(c) for c in probe], {"source": src, "steps": bsteps}
    pads = how in ("outer", "full")
    out = [_passed_on(c, padded=c.get("padded", False) or how == "full", holes=c.get("holes", False) or how == "full") for c in probe]
    out += [_passed_on(c, padded=pads, holes=pads) for j, c in enumerate(build) if j != bk or how == "full"]
    if how == "full":
        for c in out:
            if c["dtype"] == "i64" and c["dom"] is not None:
                c["dom"] = (min(c["dom"][0], lo, first), max(c["dom"][1], first + card))
    return step, out, {"source": src, "steps": bsteps}


def _step_group_keys(rng, schema):
    hints = ("padded", "fresh", "full")
    cand = [j for j, c in enumerate(schema) if c["dtype"] in ("i64", "f64", "bool", "null", "str")]
    nkeys = min(len(cand), int(rng.choice([2, 2, 3])))
    keys = []
    while len(keys) < nkeys:
        j = _pick(rng, _lean(rng, [c for c in cand if c not in keys], schema, hints, 0.7))
        keys.append(j)
    if len(keys) == 1:  # a frame of one column: the tuple of the same column twice
        keys.append(keys[0])
    options = [("count_rows", None)] + [("count", j) for j in range(len(schema))]
    for j, c in enumerate(schema):
        if c["dtype"] == "i64" or (c["dtype"] == "f64" and c["sum"]):
            options.append(("sum", j))
        if c["dtype"] in ("i64", "f64"):
            options += [("min", j), ("max", j)] * 2
    specs = [_pick(rng, options) for _ in range(int(rng.integers(1, 4)))]
    numeric = _lean(rng, [j for j, c in enumerate(schema) if c["dtype"] in ("i64", "f64")], schema, hints, 1.0)
    if any(schema[j].get(h) for j in numeric for h in hints):
        j = _pick(rng, numeric)
        specs[0] = (_pick(rng, ["min", "max"] + (["sum"] if schema[j]["dtype"] == "i64" else [])), j)
    if not any(schema[j]["dtype"] == "i64" for j in keys):
        specs = [("count_rows", None)] + specs[:2]  # every frame keeps an Int64 column
    out = [_passed_on(schema[j]) for j in keys]
    for op, j in specs:
        if op in ("count_rows", "count"):
            out.append(_col("i64"))
        elif op == "sum":
            out.append(_col(schema[j]["dtype"], None, schema[j]["sum"]))
        else:
            out.append(_passed_on(schema[j], holes=True, padded=False))
    return {"kind": "group_keys", "keys": keys, "specs": specs}, out


def _step_arith_ops(rng, schema, plain=False):
    """_step_arith; over a frame with padded numeric columns mostly an expression that reads one (a sum or a quotient, as the nulls an
    outer join wrote meet the operators)."""
    padded = [j for j, c in enumerate(schema) if c.get("padded") and c["dtype"] in ("i64", "f64")]
    if plain or not padded or rng.random() < 0.1:
        step, out = _step_arith(rng, schema, plain)
    else:
        num = [j for j, c in enumerate(schema) if c["dtype"] in ("i64", "f64")]
        a, b = ("col", _pick(rng, padded)), ("col", _pick(rng, num))
        tree = (_pick(rng, ["+", "/", "*"]), a, b) if rng.random() < 0.5 else ("/", b, a)
        dtype = {v: k for k, v in RV.items()}[arith_model.tree_dtype(tree, [RV[c["dtype"]] for c in schema])]
        step, out = {"kind": "arith", "tree": tree}, [dict(c) for c in schema] + [_col(dtype, None, False, dtype == "f64")]
    out[-1]["holes"] = True
    return step, out


def _step_group_ops(rng, schema):
    """_step_group; over a frame with padded numeric columns the last aggregate is mostly a MIN / MAX of one"""
    step, out = _step_group(rng, schema)
    padded = [j for j, c in enumerate(schema) if c.get("padded") and c["dtype"] in ("i64", "f64")]
    if padded and rng.random() < 0.9:
        j = _pick(rng, padded)
        step["specs"][-1] = (_pick(rng, ["min", "max"]), j)
        out[-1] = dict(schema[j])
    for c, (op, _) in zip(out[1:], step["specs"]):
        if op in ("min", "max"):
            c["holes"], c["padded"] = True, False
    return step, out


MAKERS_OPS = dict(MAKERS, window=_step_window, group_keys=_step_group_keys)  # (case_ops calls the makers of joins, arith, group and topk itself)
EMPTY_SEEDS_OPS = (4, 5, 7)  # mask -> a new kind over a table without rows, then the other three new kinds
TOPK_NONE_SEEDS = (25, 72 + 58)  # reshape -> topk and outer_join -> topk with k = 0
JOIN_CONSUMERS = [i for i, (_, b) in enumerate(PAIRS_OPS) if b == "outer_join"]
N_CASES_OPS = 216  # three walks through PAIRS_OPS


def case_ops(seed):
    """case() over KINDS_ALL: the first two kinds walk through PAIRS_OPS (seed % 72), then 0 to 3 drawn steps; sizes, sources and null
    shares as case() has them."""
    rng = np.random.default_rng(848_400 + seed)
    how = "csv" if seed % 10 == 3 else "slice" if seed % 10 in (1, 5, 8) else "upload"
    n = int(rng.choice(SIZES, p=SIZE_P))
    if seed % 40 == 7:
        n = LARGE
    if how == "csv":
        n = int(rng.choice([257, 300, 511]))
    a, b = PAIRS_OPS[seed % len(PAIRS_OPS)]
    steer = a == "arith"
    if steer and how == "csv":
        how = "upload"
    if seed in EMPTY_SEEDS_OPS:
        n = 0
    elif "outer_join" in (a, b) and n < 63:
        n = 65  # the walk's consumer is to meet padded cells, every kind of join rows with and rows without a partner
    walk = seed // len(PAIRS_OPS)
    pool = ["i64", "f64", "bool", "str"] + ([] if how == "csv" else ["null"])
    dts = ["i64"] + [str(rng.choice(pool)) for _ in range(int(rng.integers(1, 6)))]
    if steer:
        dts[1] = ("i64", "f64")[seed % 2]
    source, schema = _source(rng, dts, n, how, (0, 1) if steer else ())
    kinds = [a, b] + [str(rng.choice(KINDS_ALL)) for _ in range(int(rng.integers(0, 4)))]
    if seed in EMPTY_SEEDS_OPS:
        kinds = [a, b] + sorted((k for k in NEW_KINDS if k != b), key=lambda k: k == "outer_join")  # (a FULL join brings rows back: last)
    steps, builds, joins = [], {}, 0
    for pos, kind in enumerate(kinds):
        if kind in ("join", "outer_join") and joins == 2:
            kind = "sort"
        if kind == "arith" and n == LARGE and any(s["kind"] == "arith" for s in steps):
            kind = "sort"
        if kind in ("filter", "mask", "join"):
            # predicates and inner-join keys mostly look past the columns that may well be all null by now (what `dead` is for)
            for c in schema:
                c["was_dead"], c["dead"] = c["dead"], c["dead"] or c.get("padded", False) or c.get("far", False)
        if kind == "join":
            joins += 1
            step, schema, build = _step_join(rng, schema)
            builds[len(steps)] = build
        elif kind == "outer_join":
            joins += 1
            # as a walk's producer the join pads (its consumer is to meet the padded columns); as its consumer every kind takes its turn
            how_join = str(rng.choice(HOWS[:2]))  # (a drawn join sits late, over what is often a small frame: "semi" / "anti" are the walk's)
            if pos == 0:
                how_join = HOWS[(walk + seed) % 2]
            elif pos == 1:
                how_join = HOWS[(walk + JOIN_CONSUMERS.index(seed % len(PAIRS_OPS))) % 4]
            step, schema, build = _step_outer_join(rng, schema, how_join, "probe" if pos == 0 else None, 5 if pos == 0 else 0)
            builds[len(steps)] = build
        elif kind == "arith":
            step, schema = _step_arith_ops(rng, schema, steer and not steps)
        elif kind == "group":
            step, schema = _step_group_ops(rng, schema)
        elif kind == "topk":
            step, schema = _step_topk(rng, schema, n <= 2, seed in TOPK_NONE_SEEDS and pos == 1, pos == 1 and a in ("outer_join", "window"))
        else:
            step, schema = MAKERS_OPS[kind](rng, schema)
        for c in schema:
            if "was_dead" in c:
                c["dead"] = c.pop("was_dead")
        if kind not in ("arith", "window") and not (kind == "reshape" and step["how"] == "slice"):
            for c in schema:  # every other producer gathers: a bitmap without nulls is dropped
                c["full"] = c["fresh"] = False
        steps.append(step)
    return {"seed": seed, "n": n, "source": source, "steps": steps, "builds": builds}


# ---- directed pipelines: the edges by name, at any size (tests/golden/pipeline_cases.json holds each at toy size) --------------------------
def upload_of(frame):
    return {"how": "upload", "frame": frame, "padded": frame, "pad": 0, "ref": False, "text": None}


def _div_frame(n, seed):
    """a / b with zeros in b: a null quotient has 0 underneath, next to genuine quotients 0 (a = 0, or |a| < |b|)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-6, 7, n, dtype=np.int64)
    b = rng.integers(-2, 3, n, dtype=np.int64)
    _, v, _ = dyadic_cells(seed + 1, n, SCALE)
    return [("i64", a, None), ("i64", b, None), ("f64", v, None)]


DIV = {"kind": "arith", "tree": ("/", ("col", 0), ("col", 1))}


def _null_groups_frame(n, seed):
    """key k in [0, 8): the groups 2 and 5 hold null cells only, so MIN / MAX are null there with 0 underneath; specials elsewhere."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 8, n, dtype=np.int64)
    x = np.ldexp(rng.integers(-50, 50, n).astype(np.float64), -3)
    hit = rng.random(n) < 0.2
    x[hit] = np.array(SPECIALS)[rng.integers(0, len(SPECIALS), int(hit.sum()))]
    valid = ~np.isin(k, (2, 5)) & (rng.random(n) > 0.1)
    return [("i64", k, None), ("f64", x, valid), ("i64", rng.integers(-9, 9, n, dtype=np.int64), None)]


def directed(name, n, seed=5):
    """(frame, steps, {step index: (build frame, build steps)}) of the directed pipeline `name` over n rows."""
    rng = np.random.default_rng(seed)
    if name == "div_probe_key":  # the build side holds key 0 (and a null key: the null quotients meet that one, never key 0)
        build = [("i64", np.array([0, 3, 0, -2, 7], np.int64), np.array([1, 1, 1, 1, 0], bool)), ("str", ["zero", "three", "zero2", "minus", "null"], None)]
        return _div_frame(n, seed), [DIV, {"kind": "join", "probe_key": 3, "build_key": 0, "chunked": False}], {1: (build, [])}
    if name == "div_build_key":  # the same quotients HASHED: the null rows must land in the null group, not in the list of key 0
        probe = [("i64", np.array([0, 3, 0, -2, 7], np.int64), np.array([1, 1, 0, 1, 1], bool)), ("str", ["zero", "three", "null", "minus", "seven"], None)]
        return _div_frame(n, seed), [DIV, {"kind": "join", "probe_key": 3, "build_key": 0, "chunked": True, "side": "build"}], {1: (probe, [])}
    if name == "div_group_key":
        return _div_frame(n, seed), [DIV, {"kind": "group", "key": 3, "specs": [("count_rows", None), ("sum", 2), ("min", 0)]}], {}
    if name.startswith("div_sort_key_"):
        return _div_frame(n, seed), [DIV, {"kind": "sort", "keys": [(3, int(name[-1]))], "via": "sort"}], {}
    if name == "minmax_null_groups":  # MIN / MAX with empty groups -> sort by that aggregate -> take_device by a device-made index
        steps = [{"kind": "group", "key": 0, "specs": [("min", 1), ("max", 1), ("count", 1), ("sum", 2)]},
                 {"kind": "sort", "keys": [(1, 1), (2, 2)], "via": "chain"},
                 {"kind": "reshape", "how": "take_sorted", "col": 2, "flags": 3}]
        return _null_groups_frame(n, seed), steps, {}
    if name.startswith("bitmap_without_nulls_"):
        # Columns uploaded with an all-valid bitmap; rv_eval_arith keeps the bitmap on what it computes from them: columns 2 (Int64) and
        # 3 (Float64) are attached-bitmap, zero-null columns an operator wrote.  The last step hands them to one consumer each -- as
        # operands, as sort key and payload, as group key and SUM / MIN argument, as join key on either side (the other side's key made
        # the same way).  tests/test_pipeline_gpu.py asserts through pipeline_model.column_states that the consumer met the state.
        frame = [("i64", rng.integers(0, 5, n, dtype=np.int64), np.ones(n, bool)), ("f64", dyadic_cells(seed, n, SCALE)[1], np.ones(n, bool))]
        made = [{"kind": "arith", "tree": ("+", ("col", 0), ("lit", 1))}, {"kind": "arith", "tree": ("*", ("col", 1), ("lit", 0.5))}]
        other = [("i64", np.array([2, 3, 2, 9], np.int64), np.ones(4, bool)), ("f64", np.array([0.5, -1.0, 2.0, 4.0]), None)]
        other_steps = [{"kind": "arith", "tree": ("-", ("col", 0), ("lit", 0))}]
        tail = {"arith": {"kind": "arith", "tree": ("*", ("col", 2), ("col", 3))},
                "sort": {"kind": "sort", "keys": [(2, 1)], "via": "sort"},
                "group": {"kind": "group", "key": 2, "specs": [("sum", 3), ("min", 3), ("count", 2)]},
                "join_probe": {"kind": "join", "probe_key": 2, "build_key": 2, "chunked": True},
                "join_build": {"kind": "join", "probe_key": 2, "build_key": 2, "chunked": False, "side": "build"}}[name[len("bitmap_without_nulls_"):]]
        return frame, made + [tail], ({2: (other, other_steps)} if tail["kind"] == "join" else {})
    if name.startswith("empty_then_"):  # a filter that keeps nothing, then one consumer
        frame = [("i64", rng.integers(0, 9, n, dtype=np.int64), rng.random(n) > 0.2), ("f64", dyadic_cells(seed, n, SCALE)[1], rng.random(n) > 0.3),
                 ("str", [WORDS[i % 5] for i in range(n)], None), ("bool", rng.random(n) > 0.5, None), ("null", np.zeros(n, np.int64), None)]
        nothing = {"kind": "filter", "terms": [(0, "<", -1)], "nulls": "drops", "expr": None, "via": "project"}
        build = [("i64", np.array([0, 1, 2], np.int64), None), ("str", ["a", "b", "c"], None)]
        tail = {"arith": [{"kind": "arith", "tree": ("/", ("col", 0), ("col", 1))}],
                "group": [{"kind": "group", "key": 0, "specs": [("count_rows", None), ("sum", 1), ("min", 1), ("count", 2)]}],
                "group_str": [{"kind": "group", "key": 2, "specs": [("count_rows", None), ("max", 0)]}],
                "sort": [{"kind": "sort", "keys": [(1, 0), (0, 3)], "via": "sort"}],
                "sort_chain": [{"kind": "sort", "keys": [(1, 0), (4, 0)], "via": "chain"}],
                "join_probe": [{"kind": "join", "probe_key": 0, "build_key": 0, "chunked": False}],
                "join_chunked": [{"kind": "join", "probe_key": 0, "build_key": 0, "chunked": True}],
                "concat": [{"kind": "reshape", "how": "concat", "eighths": 4}],
                "mask": [{"kind": "mask", "terms": [(0, ">", 1), (1, "<", 0.0)], "expr": ("or", 0, ("not", 1))}]}[name[len("empty_then_"):]]
        return frame, [nothing] + tail, ({1: (build, [])} if tail[0]["kind"] == "join" else {})
    if name == "empty_build_side":  # the filter that keeps nothing on the BUILD side of a join
        frame = [("i64", rng.integers(0, 3, n, dtype=np.int64), None), ("f64", dyadic_cells(seed, n, SCALE)[1], None)]
        build = [("i64", np.array([0, 1, 2], np.int64), None), ("str", ["a", "b", "c"], None), ("null", np.zeros(3, np.int64), None)]
        nothing = {"kind": "filter", "terms": [(0, ">", 99)], "nulls": "least", "expr": None, "via": "selection"}
        return frame, [{"kind": "join", "probe_key": 0, "build_key": 0, "chunked": False}], {0: (build, [nothing])}
    if name == "null_columns_ride_along":  # Null-dtype columns through take, sort, join payloads and as a COUNT argument
        frame = [("i64", rng.integers(0, 4, n, dtype=np.int64), rng.random(n) > 0.1), ("null", np.zeros(n, np.int64), None),
                 ("f64", dyadic_cells(seed, n, SCALE)[1], rng.random(n) > 0.2)]
        build = [("i64", np.array([3, 1, 1], np.int64), np.array([1, 1, 1], bool)), ("null", np.zeros(3, np.int64), None), ("bool", np.array([1, 0, 1], bool), None)]
        steps = [{"kind": "reshape", "how": "take_sorted", "col": 1, "flags": 1},
                 {"kind": "sort", "keys": [(1, 2), (0, 1)], "via": "sort"},
                 {"kind": "join", "probe_key": 0, "build_key": 0, "chunked": False},
                 {"kind": "group", "key": 0, "specs": [("count", 1), ("count", 3), ("count_rows", None), ("sum", 2)]}]
        return frame, steps, {2: (build, [])}
    raise KeyError(name)


DIRECTED = (["div_probe_key", "div_build_key", "div_group_key"] + [f"div_sort_key_{f}" for f in range(4)] + ["minmax_null_groups"]
            + [f"bitmap_without_nulls_{c}" for c in ("arith", "sort", "group", "join_probe", "join_build")]
            + [f"empty_then_{c}" for c in ("arith", "group", "group_str", "sort", "sort_chain", "join_probe", "join_chunked", "concat", "mask")]
            + ["empty_build_side", "null_columns_ride_along"])


def directed_case(name, n, seed=5):
    """directed() in the shape of case(): sources are plain uploads."""
    frame, steps, builds = directed(name, n, seed)
    return {"seed": name, "n": n, "source": upload_of(frame), "steps": steps,
            "builds": {k: {"source": upload_of(b), "steps": s} for k, (b, s) in builds.items()}}


def assert_consumer_met_bitmap_without_nulls(case):
    """The last step of a bitmap_without_nulls_* pipeline reads columns 2 and 3, which an operator wrote, and both are in the state
    "bitmap attached, zero nulls" (the inspected run has compared the model's `bitmap` with has_validity on the device); a join's
    other side brings its key in the same state."""
    model, builds = pipeline_model.run_case(case)
    k = len(case["steps"]) - 1
    step, (frame, meta) = case["steps"][k], model[k]
    read = [j for j in pipeline_model.touched(step, frame) if j in (2, 3)]
    assert read == [2, 3], read
    for j in read:
        assert meta[j]["made"] and "bitmap_no_nulls" in pipeline_model.column_states(frame[j], meta[j]), f"{step['kind']} input column {j}: {meta[j]}"
    if step["kind"] in pipeline_model.JOINS:
        bframe, bmeta = builds[k][-1]
        j = step["build_key"]
        assert bmeta[j]["made"] and "bitmap_no_nulls" in pipeline_model.column_states(bframe[j], bmeta[j]), f"join, other side's key: {bmeta[j]}"


# ---- directed pipelines over the newer operators (tests/golden/pipeline_ops_cases.json holds a hand-written toy version of each) -------
SLICE_AT = (1, 63, 65)
NOTHING = {"kind": "filter", "terms": [(0, "<", -1)], "nulls": "drops", "expr": None, "via": "project"}


def _outer_frames(n, rng, seed):
    """Probe keys in [0, 10) and build keys in [3, 13), a null key on each side, payloads of every dtype: a FULL join pads both sides.
    Output columns of the FULL join: probe 0 key, 1 Float64, 2 String, 3 Boolean, 4 Null; build 5 key, 6 Float64, 7 String, 8 Boolean."""
    m = max(4, n // 8)
    probe = [("i64", rng.integers(0, 10, n, dtype=np.int64), rng.random(n) > 0.1), ("f64", dyadic_cells(seed, n, SCALE)[1], rng.random(n) > 0.2),
             ("str", [WORDS[i % 5] for i in range(n)], None), ("bool", rng.random(n) > 0.5, rng.random(n) > 0.1), ("null", np.zeros(n, np.int64), None)]
    bvalid = np.ones(m, bool)
    bvalid[m // 2] = False
    build = [("i64", 3 + np.arange(m, dtype=np.int64) % 10, bvalid), ("f64", dyadic_cells(seed + 1, m, SCALE)[1], rng.random(m) > 0.2),
             ("str", [WORDS[(i + 2) % 6] for i in range(m)], None), ("bool", rng.random(m) > 0.5, None)]
    if n:
        probe[0][2][0] = False  # a null key on the probe side whatever the draw
        probe[0][1][-1] = 1     # and a key no build row holds
    return probe, build


FULL = {"kind": "outer_join", "how": "full", "probe_key": 0, "build_key": 0, "chunked": False, "side": "probe"}


def _minmax_frame(n, rng, seed, nulls):
    """key k in [0, max(6, n / 8)) and an Int64 x whose first cells in every partition are null (nulls: else none is): CUM_MIN / CUM_MAX over the
    partitions in row order are null at every partition's start."""
    k = rng.integers(0, max(6, n // 8), n, dtype=np.int64)  # (partitions start all along the frame: a slice keeps null cells)
    x = rng.integers(-40, 40, n, dtype=np.int64)
    valid = np.ones(n, bool)
    if nulls:
        seen = collections.Counter()
        for i, key in enumerate(k.tolist()):
            seen[key] += 1
            valid[i] = seen[key] > 2 and rng.random() > 0.1
    return [("i64", k, None), ("i64", x, valid if nulls else None), ("f64", dyadic_cells(seed, n, SCALE)[1], None)]


def directed_ops(name, n, seed=5):
    """(frame, steps, {step index: (second frame, its steps)}) of the directed pipeline `name` over n rows."""
    rng = np.random.default_rng(seed)
    if name.startswith("full_outer_then_"):
        # The consumer reads the columns FULL_OUTER padded -- value 0 under the null -- as keys and operands.
        probe, build = _outer_frames(n, rng, seed)
        c = name[len("full_outer_then_"):]
        builds = {0: (build, [])}
        if c == "window":  # partitions by the padded probe key, ordered by the padded build payload
            tail = [{"kind": "window", "partition_by": [0], "order_by": [(6, 2)],
                     "exprs": [("row_number", 0), ("dense_rank", 0), ("cum_count", 6), ("cum_min", 6), ("cum_max", 0), ("lag", 7, 1), ("lead", 3, 1), ("cum_sum", 5)]}]
        elif c.startswith("topk_"):  # the padded Float64 payload under flag word f, k below / above its null count, the select forced
            tail = [{"kind": "topk", "keys": [(6, int(c[5]))], "k": ["of", 1, 8] if c.endswith("lo") else ["of", 9, 20], "via": "frame", "select": True}]
        elif c == "group_keys":
            tail = [{"kind": "group_keys", "keys": [0, 5], "specs": [("count_rows", None), ("sum", 1), ("min", 6), ("count", 7)]}]
        elif c == "sort":
            tail = [{"kind": "sort", "keys": [(5, 0), (0, 3)], "via": "sort"}]
        elif c == "group":
            tail = [{"kind": "group", "key": 5, "specs": [("count", 0), ("min", 6), ("sum", 1)]}]
        elif c == "arith":
            tail = [{"kind": "arith", "tree": ("+", ("col", 0), ("col", 5))}, {"kind": "arith", "tree": ("/", ("col", 0), ("col", 5))}]
        else:  # the padded build key probes a second join whose build side holds key 0 (and a null key: the padded rows meet that one)
            assert c == "join", name
            second = [("i64", np.array([0, 4, 0, 7, 12], np.int64), np.array([1, 1, 1, 1, 0], bool)), ("str", ["zero", "four", "zero2", "seven", "null"], None)]
            tail = [{"kind": "join", "probe_key": 5, "build_key": 0, "chunked": False}]
            builds[1] = (second, [])
        return probe, [dict(FULL)] + tail, builds
    if name.startswith("window_minmax_"):  # window_minmax_<bitmap | plain>_then_<c>_<offset>
        _, _, state, _, c, off = name.split("_", 5)
        if c == "group":
            c, off = "group_keys", off.split("_")[-1]
        if c == "outer":
            c, off = "outer_join", off.split("_")[-1]
        frame = _minmax_frame(n, rng, seed, state == "bitmap")
        steps = [{"kind": "window", "partition_by": [0], "order_by": [], "exprs": [("cum_min", 1), ("cum_max", 1)]},
                 {"kind": "reshape", "how": "slice", "offset": int(off), "tail": 1}]
        second = [("i64", np.array([-5, 3, -5, 30, 0], np.int64), np.array([1, 1, 1, 1, 0], bool)), ("f64", np.array([0.5, 1.5, 2.5, 3.5, 4.5]), None)]
        tail = {"sort": {"kind": "sort", "keys": [(3, 1), (4, 2)], "via": "sort"},
                "topk": {"kind": "topk", "keys": [(3, 0), (4, 1)], "k": ["of", 1, 4], "via": "frame", "select": True},
                "group_keys": {"kind": "group_keys", "keys": [3, 0], "specs": [("count_rows", None), ("max", 4), ("sum", 2)]},
                "filter": {"kind": "filter", "terms": [(3, "<", 0)], "nulls": "least", "expr": None, "via": "project"},
                "outer_join": {"kind": "outer_join", "how": "outer", "probe_key": 3, "build_key": 0, "chunked": True, "side": "probe"}}[c]
        return frame, steps + [tail], ({2: (second, [])} if c == "outer_join" else {})
    if name.startswith("topk_indices_as_index_"):  # top_k_indices over a / b, select forced; take_device by it; a window over the k rows
        steps = [DIV, {"kind": "topk", "keys": [(3, int(name[-1]))], "k": ["of", 1, 4], "via": "indices", "select": True},
                 {"kind": "window", "partition_by": [1], "order_by": [(3, 0)], "exprs": [("rank", 0), ("cum_sum", 2), ("lag", 3, 1)]}]
        return _div_frame(n, seed), steps, {}
    if name.startswith("empty_then_"):
        frame = directed("empty_then_sort", n, seed)[0]
        build = [("i64", np.array([0, 1, 2], np.int64), None), ("str", ["a", "b", "c"], None)]
        c = name[len("empty_then_"):]
        if c in HOWS:
            return frame, [NOTHING, {"kind": "outer_join", "how": c, "probe_key": 0, "build_key": 0, "chunked": c == "semi", "side": "probe"}], {1: (build, [])}
        tail = {"window": {"kind": "window", "partition_by": [0, 3], "order_by": [(1, 1)], "exprs": [("row_number", 0), ("cum_sum", 1), ("cum_min", 0), ("lag", 2, 1), ("lead", 4, 0)]},
                "topk": {"kind": "topk", "keys": [(1, 0), (0, 3)], "k": ["abs", 7], "via": "frame", "select": True},
                "group_keys": {"kind": "group_keys", "keys": [0, 3, 2], "specs": [("count_rows", None), ("sum", 1), ("min", 1)]}}[c]
        return frame, [NOTHING, tail], {}
    if name.startswith("empty_build_side_") or name == "empty_probe_side_full":
        frame = [("i64", rng.integers(0, 3, n, dtype=np.int64), rng.random(n) > 0.1), ("f64", dyadic_cells(seed, n, SCALE)[1], None), ("str", [WORDS[i % 4] for i in range(n)], None)]
        other = [("i64", np.array([0, 1, 2], np.int64), None), ("str", ["a", "b", "c"], None), ("null", np.zeros(3, np.int64), None), ("bool", np.array([1, 0, 1], bool), None),
                 ("f64", np.array([0.5, -1.0, 2.0]), None)]
        nothing = {"kind": "filter", "terms": [(0, ">", 99)], "nulls": "least", "expr": None, "via": "selection"}
        if name == "empty_probe_side_full":
            return frame, [NOTHING, dict(FULL)], {1: (other, [])}
        return frame, [{"kind": "outer_join", "how": name.split("_")[-1], "probe_key": 0, "build_key": 0, "chunked": False, "side": "probe"}], {0: (other, [nothing])}
    if name.startswith("bitmap_without_nulls_"):
        frame, made, builds = directed("bitmap_without_nulls_join_probe", n, seed)
        made, other = made[:2], builds[2]
        tail = {"window": {"kind": "window", "partition_by": [2], "order_by": [(3, 0)], "exprs": [("cum_sum", 3), ("cum_max", 2), ("lag", 3, 1), ("rank", 0)]},
                "topk": {"kind": "topk", "keys": [(3, 1), (2, 0)], "k": ["of", 1, 8], "via": "frame", "select": True},
                "group_keys": {"kind": "group_keys", "keys": [2, 3], "specs": [("sum", 3), ("min", 2), ("count_rows", None)]},
                "outer_join_probe": {"kind": "outer_join", "how": "outer", "probe_key": 2, "build_key": 2, "chunked": True, "side": "probe"},
                "outer_join_build": {"kind": "outer_join", "how": "full", "probe_key": 2, "build_key": 2, "chunked": False, "side": "build"}}[name[len("bitmap_without_nulls_"):]]
        return frame, made + [tail], ({2: other} if tail["kind"] == "outer_join" else {})
    if name == "null_columns_ride_along_ops":
        # Null-dtype columns as window partition key and order key, LAG source, CUM_COUNT argument, top-k key, group_keys key and
        # FULL_OUTER payload (column 1 on the probe side, the second frame's column 1)
        frame = [("i64", rng.integers(0, 4, n, dtype=np.int64), rng.random(n) > 0.1), ("null", np.zeros(n, np.int64), None),
                 ("f64", dyadic_cells(seed, n, SCALE)[1], rng.random(n) > 0.2)]
        build = [("i64", np.array([3, 1, 1, 8], np.int64), None), ("null", np.zeros(4, np.int64), None), ("bool", np.array([1, 0, 1, 1], bool), None)]
        steps = [{"kind": "window", "partition_by": [1, 0], "order_by": [(1, 3), (2, 0)], "exprs": [("lag", 1, 1), ("cum_count", 1), ("row_number", 1)]},
                 dict(FULL),
                 {"kind": "topk", "keys": [(1, 1), (5, 0)], "k": ["of", 3, 4], "via": "frame", "select": True},
                 {"kind": "group_keys", "keys": [1, 0, 3], "specs": [("count", 7), ("count_rows", None), ("max", 5)]}]
        return frame, steps, {1: (build, [])}
    raise KeyError(name)


DIRECTED_OPS = ([f"full_outer_then_{c}" for c in ("window", "group_keys", "sort", "group", "arith", "join")]
                + [f"full_outer_then_topk_{f}_{side}" for f in range(4) for side in ("lo", "hi")]
                + [f"window_minmax_bitmap_then_{c}_{o}" for c in ("sort", "topk", "group_keys", "filter", "outer_join") for o in SLICE_AT]
                + [f"window_minmax_plain_then_{c}_1" for c in ("sort", "topk", "group_keys", "filter", "outer_join")]
                + [f"topk_indices_as_index_{f}" for f in range(4)]
                + [f"empty_then_{c}" for c in ("window", "topk", "group_keys") + HOWS]
                + [f"empty_build_side_{c}" for c in HOWS] + ["empty_probe_side_full"]
                + [f"bitmap_without_nulls_{c}" for c in ("window", "topk", "group_keys", "outer_join_probe", "outer_join_build")]
                + ["null_columns_ride_along_ops"])


def directed_ops_case(name, n, seed=5):
    """directed_ops() in the shape of case_ops(): sources are plain uploads."""
    frame, steps, builds = directed_ops(name, n, seed)
    return {"seed": name, "n": n, "source": upload_of(frame), "steps": steps,
            "builds": {k: {"source": upload_of(b), "steps": s} for k, (b, s) in builds.items()}}


def assert_point(name, case):
    """Where data could lose the point of a directed pipeline: assert that it is there (on the model alone)."""
    pm = pipeline_model
    model, builds = pm.run_case(case)
    pads = pm.padded_run(case, model, builds)
    steps = case["steps"]
    if name.startswith("full_outer_then_"):
        frame = model[1][0]
        for j in (0, 5, 6):  # both keys and the build payload hold padded nulls, and the probe key a genuine 0 beside them
            assert pads[1][j].any(), f"{name}: FULL_OUTER padded nothing into column {j}"
        assert (frame[0][1][pm.valid_of(frame[0])] == 0).any() and pm.null_count(frame[0]) > int(pads[1][0].sum()), name
        if "_topk_" in name and case["n"] >= 64:
            k, nulls = pm.topk_k(steps[1], pm.rows(frame)), pm.null_count(frame[6])
            assert (k < nulls) == name.endswith("lo"), f"{name}: k {k} against {nulls} nulls"
            assert pm.topk_select(steps[1], frame, 1, const("kTopKRefineDivisor")).passes >= 1, f"{name}: the select does not run"
    if name.startswith("window_minmax_"):
        frame, meta = model[2]  # what the consumer reads: the sliced window outputs
        for j in (3, 4):
            nulls = pm.null_count(frame[j])
            assert meta[j]["made"] and meta[j]["offset"] == min(steps[1]["offset"], pm.rows(model[1][0]) // 2) and meta[j]["bitmap"] == ("_bitmap_" in name)
            assert (nulls > 0) == ("_bitmap_" in name), f"{name}: {nulls} nulls in column {j}"
    if name.startswith("topk_indices_as_index_"):
        q = model[1][0][3]
        assert pm.null_count(q) > 0 and (q[1][pm.valid_of(q)] == 0).any(), "the case lost its point: no null quotient beside a genuine 0"
        if case["n"] >= 64:
            assert pm.topk_select(steps[1], model[1][0], 1, const("kTopKRefineDivisor")).passes >= 1, f"{name}: the select does not run"
    if name.startswith("empty_then_") or name == "empty_probe_side_full":
        assert pm.rows(model[1][0]) == 0
        assert pm.rows(model[-1][0]) == (3 if name.endswith("full") else 0)
    if name.startswith("empty_build_side_"):
        how = name.split("_")[-1]
        assert pm.rows(builds[0][-1][0]) == 0
        assert pm.rows(model[-1][0]) == (0 if how == "semi" else case["n"])
        if how == "anti":
            assert pm.frame_diff(model[-1][0], model[0][0]) is None
        if how in ("outer", "full"):
            assert pm.dtypes(model[-1][0])[3:] == (["i64"] if how == "full" else []) + ["str", "null", "bool", "f64"]
            assert all(pm.null_count(c) == case["n"] for c in model[-1][0][3:])
    if name.startswith("bitmap_without_nulls_"):
        assert_consumer_met_bitmap_without_nulls(case)
    if name == "null_columns_ride_along_ops":
        assert [model[k][0][j][0] for k, j in ((0, 1), (1, 3), (2, 1), (2, 7))] == ["null"] * 4
