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
    if step["kind"] == "join":
        bframe, bmeta = builds[k][-1]
        j = step["build_key"]
        assert bmeta[j]["made"] and "bitmap_no_nulls" in pipeline_model.column_states(bframe[j], bmeta[j]), f"join, other side's key: {bmeta[j]}"
