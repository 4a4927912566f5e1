"""Shared helpers: golden-case loading, column comparison, the constants of thresholds.hpp, the host layer's test programs."""
import json
import os
import re
import struct
import subprocess

import numpy as np

from rivulus_amd.capi import Column, Predicate, Term

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cases.json")
THRESHOLDS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rivulus_amd", "csrc", "thresholds.hpp")
_NP = {"i": np.int64, "f": np.float64, "b": np.bool_}


def _decode_col(c):
    if c["kind"] == "f":
        vals = np.array([float.fromhex(x) for x in c["values"]], np.float64)
    else:
        vals = np.array(c["values"], _NP[c["kind"]])
    valid = None if c["valid"] is None else np.array(c["valid"], bool)
    return Column.from_numpy(vals, valid)


def load_golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    out = []
    for case in doc["cases"]:
        terms = []
        for t in case["predicate"]["terms"]:
            lit = t["literal"]
            if t["literal_is_float"]:
                lit = float.fromhex(lit)
            terms.append(Term(t["column"], t["op"], lit))
        out.append({
            "name": case["name"],
            "columns": [_decode_col(c) for c in case["columns"]],
            "predicate": Predicate(terms, case["predicate"]["nulls"], case["predicate"].get("expr")),
            "projection": case["projection"],
            "rows": case["rows"],
            "expected": [_decode_col(c) for c in case["expected"]],
        })
    return out


def assert_columns_equal(got, expected, what=""):
    assert len(got) == len(expected), f"{what}: {len(got)} columns != {len(expected)}"
    for j, (g, e) in enumerate(zip(got, expected)):
        diff = g.same_as(e)
        assert diff is None, f"{what} column {j}: {diff}"


def const(name):
    """The value of constant `name` in rivulus_amd/csrc/thresholds.hpp (tests name a switch, never its value)."""
    with open(THRESHOLDS) as f:
        m = re.search(rf"\b{name} = ([^;,]+)[;,]", f.read())
    v = m.group(1).strip()
    if "<<" in v:
        a, b = re.findall(r"\d+", v)[-2:]
        return int(a) << int(b)
    return float(v) if "." in v else int(v)


# ---- Float64 sums that are exact in any order -----------------------------------------------------------------------------
# Every cell is k * 2^s with an integer |k| < 2^20.  As long as sum(|k|) < 2^53 every partial sum of any reduction tree is an
# integer multiple of 2^s below 2^53 * 2^s, hence exactly representable: a Float64 SUM over such cells has ONE correct bit
# pattern, whatever the launch geometry, and that pattern follows from integer arithmetic on the host.
DYADIC_SCALES = (-1074, -10, 960)  # subnormal cells throughout / ordinary / sums up to 2^1000 (no overflow below 2^40 * 2^960)
DYADIC_K_BITS = 20
NULL_FILL = (float("nan"), float("inf"), float("-inf"), 1e300)  # what lies under a null cell, in rotation


def dyadic_cells(seed, n, scale, null_fraction=0.0):
    """(k, values, valid): n Float64 cells k * 2^scale, k a random integer with |k| < 2^20 (both signs, one in twenty a zero).
    null_fraction > 0: a validity mask as well, and NULL_FILL in rotation under the null cells -- bit patterns that must never
    reach a sum."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-(1 << DYADIC_K_BITS) + 1, 1 << DYADIC_K_BITS, n, dtype=np.int64)
    k[rng.random(n) < 0.05] = 0
    values = np.ldexp(k.astype(np.float64), scale)
    valid = None
    if null_fraction > 0:
        valid = rng.random(n) >= null_fraction
        nulls = np.flatnonzero(~valid)
        values[nulls] = np.array(NULL_FILL)[np.arange(len(nulls)) % len(NULL_FILL)]
    return k, values, valid


def dyadic_sum(k, scale, take):
    """The one correct Float64 sum of the cells k[take] * 2^scale, from integer arithmetic."""
    return float(int(k[take].sum(dtype=np.int64))) * 2.0 ** scale


def float_bits(x):
    return struct.pack("<d", x)


def same_float(got, want):
    """Bit for bit the same double (so -0.0 is not +0.0), or both a NaN."""
    return float_bits(got) == float_bits(want) or (got != got and want != want)


# ---- the filter kernels' launch tables, read from the sources ---------------------------------------------------------------
CSRC = os.path.join(os.path.dirname(THRESHOLDS))
FUSED_SOURCES = ("fused_lean1.hip", "fused_valid1.hip", "fused_multi.hip", "fused_bool.hip", "fused_full.hip", "fused_expr.hip", "fused_roomy.hip")
NARROW_SOURCE = "fused_narrow.hip"  # passes over codes: RV_NARROW(R, FLAGS) is fused_filter_compact<1,R,2,16,FLAGS> and its plain twin
DIRECT_SOURCES = ("fused_direct.hip", "fused_direct2.hip")
REDO_SOURCE = "fused_full.hip"
_ENTRY = re.compile(r"\b(RV_FUSED|RV_NARROW|RV_DIRECT3|RV_DIRECT)\(([^()]*)\)")


def _table_text(name):
    """A table source without its comments and its #define lines (the macros' own definitions are no entries)."""
    with open(os.path.join(CSRC, name)) as f:
        src = f.read()
    src = re.sub(r"//[^\n]*", "", src)
    return "\n".join(line for line in src.splitlines() if not line.lstrip().startswith("#"))


def kernel_flags():
    """{name: value} of the FF_* feature flags of csrc/scan_frontend.hpp."""
    with open(os.path.join(CSRC, "scan_frontend.hpp")) as f:
        return {k: int(v) for k, v in re.findall(r"\b(FF_[A-Z0-9_]+) = (\d+)", f.read())}


def _flag_value(expr, names):
    """`FF_A | FF_B | 0` with the names of `names`: an OR of known constants, nothing else."""
    value = 0
    for part in expr.split("|"):
        part = part.strip()
        value |= int(part) if part.isdigit() else names[part]
    return value


def table_entries(name):
    """Every entry of table source `name`, in order, as (kernel, a, b, c, d, flags): fused_filter_compact<NC,R,V,W,F> or
    fused_direct_compact<NP,NQ,R,W,F>, the flags evaluated with the FF_* values and the file's own `constexpr int` aliases."""
    text = _table_text(name)
    names = kernel_flags()
    for decl in re.findall(r"constexpr int ([^;]+);", text):
        for alias, expr in re.findall(r"(\w+) = ([^,]+)", decl):
            names[alias] = _flag_value(expr, names)
    out = []
    for macro, args in _ENTRY.findall(text):
        args = [a.strip() for a in args.split(",")]
        if macro == "RV_DIRECT3":
            a, b, c, d = (int(v) for v in args)
            out += [("fused_direct_compact", a, b, c, d, f) for f in (0, names["FF_VALIDITY"], names["FF_VALIDITY"] | names["FF_BOOL"])]
        elif macro == "RV_NARROW":
            out.append(("fused_filter_compact", 1, int(args[0]), 2, 16, _flag_value(args[1], names)))
        else:
            a, b, c, d = (int(v) for v in args[:4])
            out.append(("fused_filter_compact" if macro == "RV_FUSED" else "fused_direct_compact", a, b, c, d, _flag_value(args[4], names)))
    return out


def redo_entries():
    """(ncols, rows per lane) of every fused_redo_waves instantiation behind a case label of redo_kernel()."""
    text = _table_text(REDO_SOURCE)
    body = text[text.index("redo_kernel("):]
    return [(int(a), int(b)) for a, b in re.findall(r"case \d+:\s*return &fused_redo_waves<(\d+), (\d+)>", body)]


def kernel_name(entry):
    """As rv_ctx_last_kernel spells it: fused_filter_compact<3,12,1,16,1>."""
    return f"{entry[0]}<{','.join(str(v) for v in entry[1:])}>"


def table_kernels():
    """The distinct kernel names of the nine tables, in table order (an entry listed in two tables is one kernel)."""
    seen = {}
    for src in FUSED_SOURCES + DIRECT_SOURCES:
        for e in table_entries(src):
            seen.setdefault(kernel_name(e), e)
    return seen


# (the aggregate's table is small enough to be listed by hand below; the filter kernels' tables are read by table_entries above:
#  either way every instantiation has a case, and tests/test_instantiation_table_cpu.py holds the filter tables to it)
# filter_agg_kernel<ncols, r, vec, 4, flags> (csrc/agg_table.hip): rows per lane by the number of 8-byte columns a pass reads,
# so a tile is 256 * r rows; flags 0 or FF_VALIDITY | FF_BOOL
AGG_R = {1: 16, 2: 8, 3: 4, 4: 4}
AGG_F = 3
# case name -> (8-byte columns of the launch, flags, Int64 predicate columns)
AGG_CASES = {"plain1": (1, 0, 0), "nullable1": (1, AGG_F, 0), "boolean1": (1, AGG_F, 0), "cols2": (2, AGG_F, 1),
             "cols3": (3, AGG_F, 2), "cols4": (4, AGG_F, 3), "cols5": (1, AGG_F, 4)}
_PRED_TERMS = [("<", 70), (">=", 15), ("!=", 3), (">", 8)]


def agg_kernel_name(ncols, vec, flags):
    return f"filter_agg_kernel<{ncols},{AGG_R[ncols]},{vec},4,{flags}>"


def agg_sizes(ncols):
    """Row counts round one lane, one wave and the tile of the ncols-column variant."""
    t = 256 * AGG_R[ncols]
    return [1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1]


def agg_case(case, n, scale, seed, nulls="drops"):
    """(cols, k, pred, agg_col) of one launch shape of the aggregate.  The aggregated dyadic Float64 column comes LAST, after the
    columns the predicate reads (nullable Int64 in [0, 100), or one nullable Boolean), so the predicate never reads it:
      plain1     no bitmap anywhere; the only column a one-column launch can test is the aggregated one (x != 3 * 2^scale)
      nullable1  the same over a nullable aggregated column
      boolean1   is_true(Boolean column), aggregated column without bitmap
      cols2..5   1..4 Int64 predicate columns + nullable aggregated column (cols5: one column more than a pass reads)"""
    _, _, npred = AGG_CASES[case]
    k, values, valid = dyadic_cells(seed, n, scale, 0.0 if case in ("plain1", "boolean1") else 0.2)
    rng = np.random.default_rng(seed + 7919)
    cols, terms = [], []
    for j in range(npred):
        cols.append(Column.from_numpy(rng.integers(0, 100, n, dtype=np.int64), rng.random(n) >= 0.15))
        terms.append(Term(j, *_PRED_TERMS[j]))
    if case == "boolean1":
        cols.append(Column.from_numpy(rng.random(n) < 0.6, rng.random(n) >= 0.15))
        terms.append(Term(0, "is_true"))
    cols.append(Column.from_numpy(values, valid))
    agg = len(cols) - 1
    if not terms:
        terms.append(Term(agg, "!=", float(np.ldexp(3.0, scale))))
    return cols, k, Predicate(terms, nulls), agg


def agg_expected(cols, k, scale, pred, agg):
    """(sum, count) of filter + SUM/COUNT from the host arrays: COUNT = surviving rows, SUM over the surviving non-null cells."""
    keep = host_survivors(cols, pred)
    valid = cols[agg].logical_valid()
    return dyadic_sum(k, scale, keep if valid is None else keep & valid), int(keep.sum())


_COMPARE = {"==": np.equal, "!=": np.not_equal, "<": np.less, ">": np.greater, "<=": np.less_equal, ">=": np.greater_equal}


def host_survivors(cols, pred):
    """The rows `pred` keeps, in numpy from the host columns (include/rivulus_gpu.h, rv_predicate; Int64 / Float64 compares with a
    literal of the column's type and Boolean is_true only).  "drops": a row survives iff every cell the expression reads is valid
    and the expression is true.  "least": a null cell orders below every value, so <, <= and != keep it."""
    n = cols[0].length
    truth, known = [], []
    for t in pred.terms:
        c = cols[t.column]
        v, ok = c.logical_values(), c.logical_valid()
        ok = np.ones(n, bool) if ok is None else ok
        x = v.astype(bool) if t.op == "is_true" else _COMPARE[t.op](v, t.literal)
        if pred.nulls == "least":
            assert t.op != "is_true"
            x = np.where(ok, x, t.op in ("<", "<=", "!="))
            ok = np.ones(n, bool)
        truth.append(x)
        known.append(ok)

    read = set()

    def ev(tree):
        if isinstance(tree, (int, np.integer)):
            read.add(int(tree))
            return truth[int(tree)]
        op, *args = tree
        if op == "not":
            return ~ev(args[0])
        vals = [ev(a) for a in args]
        return np.logical_and.reduce(vals) if op == "and" else np.logical_or.reduce(vals)

    keep = ev(pred.expr if pred.expr is not None else ("and", *range(len(pred.terms))))
    for i in read:
        keep = keep & known[i]
    return keep


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_host_runs = {}


def host_cases(binary):
    """(CPU case names, GPU case names) of tests/cpp/<binary>.cpp"""
    with open(os.path.join(ROOT, "tests", "cpp", binary + ".cpp")) as f:
        src = f.read()
    return re.findall(r"^CPU_TEST\((\w+)\)", src, re.M), re.findall(r"^GPU_TEST\((\w+)\)", src, re.M)


def assert_host_case(binary, case, cpu_only, arg=None, timeout=300):
    """`case` of the host test program `binary` printed "ok".  The library and the program are built, and the program run, once per
    mode (cpu_only: its --cpu cases alone); arg() gives the program's own argument, a directory, when it takes one."""
    import pytest

    if (binary, cpu_only) not in _host_runs:
        subprocess.run(["make", "-C", os.path.join(ROOT, "rivulus_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
        subprocess.run(["make", "-C", os.path.join(ROOT, "rivulus_amd", "host"), binary], check=True, stdout=subprocess.DEVNULL)
        cmd = [os.path.join(ROOT, "rivulus_amd", "host", binary)] + (["--cpu"] if cpu_only else []) + ([arg()] if arg else [])
        _host_runs[binary, cpu_only] = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    result = _host_runs[binary, cpu_only]
    for line in result.stdout.splitlines():
        if line.split()[1:2] == [case] or line.startswith(f"FAIL {case}:"):
            assert line.startswith("ok "), line
            return
    pytest.fail(f"case {case} produced no line; stdout: {result.stdout[-1000:]} stderr: {result.stderr[-1000:]}")
