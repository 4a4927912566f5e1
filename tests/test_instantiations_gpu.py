"""Every instantiation of the filter kernels' launch tables against the oracle (-m gpu): one item per entry of the fused_filter_compact
and fused_direct_compact tables, one per fused_redo_waves instantiation, one per (rows per lane, waves) geometry with many tiles per
workgroup.  The query of an entry is DERIVED from its template arguments (staged_query / direct_query below, after choose_launch and
find_direct in csrc/fused_launch.hip), the geometry is forced by the public options, and after every call the kernel that ran is
compared with the entry's name: a launch that quietly lands on a neighbour fails.  tests/test_instantiation_table_cpu.py holds the
lists below to the tables read from the sources, so an instantiation added without a case fails without a GPU."""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import pytest

from helpers import assert_columns_equal, kernel_flags
from rivulus_amd.capi import Column, Predicate, Term

FF = kernel_flags()
V, B, XS, SEL = FF["FF_VALIDITY"], FF["FF_BOOL"], FF["FF_XS"], FF["FF_SEL"]
I64, F64, A, N, E, OV = FF["FF_ONE_I64"], FF["FF_ONE_F64"], FF["FF_PROJALL"], FF["FF_NONULL"], FF["FF_EXPR"], FF["FF_OUTVALID"]

# fused_filter_compact<NC,R,V,W,F>: (NC, F) -> "R.V.W" of every geometry the tables hold for that shape
STAGED = {
    (1, I64): "16.2.16 16.1.16 24.2.16 32.2.8 32.1.8 16.2.8 8.2.16 4.2.16",
    (1, F64): "16.2.16 16.1.16 8.2.16 4.2.16",
    (1, I64 | SEL): "16.2.16 16.1.16 8.2.16 4.2.16",
    (1, F64 | SEL): "16.2.16 16.1.16 4.2.16",
    (1, 0): "16.2.16 16.1.16 32.2.8 8.2.16 4.2.16",
    (1, A): "16.2.16 16.1.16 8.2.16 4.2.16",
    (1, V): "16.2.16 16.1.16 8.2.16 8.1.16 4.2.16 4.1.16",
    (1, V | A): "16.2.16 16.1.16 8.2.16 4.2.16 4.1.16",
    (1, V | A | N): "16.2.16 16.1.16 8.2.16 8.1.16 4.2.16 4.1.16",
    (2, 0): "8.1.16 8.2.16 4.1.16",
    (2, V): "8.1.16 8.2.16 4.1.16",
    (2, A): "12.2.16 8.2.16 8.1.16 4.1.16",
    (2, V | A): "12.2.16 8.2.16 8.1.16 4.1.16",
    (2, V | A | N): "16.1.16 12.1.16 8.1.16 12.2.16 16.2.16 8.2.16 4.1.16",
    (3, V): "8.1.16 12.1.16 4.1.16 4.1.8",
    (4, V): "8.1.16 4.1.16 4.1.8",
    (3, 0): "8.1.16 8.2.16 4.1.16 4.1.8",
    (3, A): "8.2.16 8.1.16 4.1.16 4.1.8",
    (3, V | A): "8.2.16 12.1.16 8.1.16 4.1.16 4.1.8",
    (3, V | A | N): "8.2.16 8.1.16 4.1.16 4.1.8",
    (4, A): "4.1.16 4.1.8",
    (4, V | A): "8.1.16 4.1.16 4.1.8",
    (1, B | A): "16.2.16 16.1.16",
    (1, B | V | A): "16.2.16 16.1.16",
    (2, B | A): "8.2.16 8.1.16",
    (2, B | V | A): "8.2.16 8.1.16",
    (3, B | V | A): "4.1.16",
    (4, B | V | A): "4.1.16",
    (3, B | A): "8.1.16",
    (4, B | A): "4.1.16",
    (1, B | XS | A): "16.1.16",
    (1, B | XS | V | A): "16.1.16",
    (2, B | XS | V | A): "8.1.16",
    (1, XS | A): "16.1.16",
    (1, XS | V | A): "16.1.16",
    (2, XS | V | A): "8.1.16",
    (0, V | B | XS | SEL): "16.1.16",
    (1, V | B | XS | SEL): "8.1.16",
    (2, V | B | XS | SEL): "4.1.16",
    (3, V | B | XS | SEL): "4.1.16",
    (4, V | B | XS | SEL): "4.1.16",
    (0, V | B | SEL | E): "16.1.16",
    (1, V | B | SEL | E): "16.1.16 8.2.16",
    (2, V | B | SEL | E): "16.1.16 8.1.16 8.2.16",
    (3, V | B | SEL | E): "8.1.16 4.1.16",
    (4, V | B | SEL | E): "8.1.16 4.1.16",
    (1, V | A | N | E): "16.1.16",
    (2, V | A | N | E): "16.1.16",
    (3, V | A | N | E): "8.1.16",
    (1, A | E): "16.1.16",
    (2, A | E): "16.1.16",
    (3, A | E): "8.1.16",
    (2, V | E): "16.1.16",
    (3, V | E): "12.1.16 8.1.16",
    (4, V | E): "4.1.16",
    (2, V | N | E): "16.1.16",
    (3, V | N | E): "12.1.16 8.1.16",
    (4, V | N | E): "4.1.16",
}
# fused_direct_compact<NP,NQ,R,W,F>: (NP, NQ, F) -> "R.W"
DIRECT = {
    (1, 0, 0): "12.8 16.8 8.8 16.16 16.4",
    (1, 0, V): "12.8 16.8",
    (1, 0, V | B): "12.8 16.8",
    (1, 1, 0): "8.8",
    (1, 1, V): "8.8",
    (1, 1, V | B): "8.8",
    (1, 2, 0): "6.8 4.8 4.16 8.4",
    (1, 2, V): "6.8 4.8",
    (1, 2, V | B): "6.8 4.8",
    (1, 3, 0): "4.8",
    (1, 3, V): "4.8",
    (1, 3, V | B): "4.8",
    (2, 0, 0): "6.8 4.8",
    (2, 0, V): "6.8 4.8",
    (2, 0, V | B): "6.8 4.8",
    (1, 0, V | OV): "12.8 16.8",
    (1, 1, V | OV): "8.8",
    (1, 2, V | OV): "6.8 4.8",
    (1, 3, V | OV): "4.8",
    (2, 0, V | OV): "6.8",
    (2, 1, 0): "6.8 4.8",
    (2, 1, V): "6.8 4.8",
    (2, 1, V | B): "6.8 4.8",
    (2, 2, 0): "4.8",
    (2, 2, V): "4.8",
    (2, 2, V | B): "4.8",
    (3, 0, 0): "4.8",
    (3, 0, V): "4.8",
    (3, 0, V | B): "4.8",
    (3, 1, 0): "4.8",
    (3, 1, V): "4.8",
    (3, 1, V | B): "4.8",
    (4, 0, 0): "4.8",
    (4, 0, V): "4.8",
    (4, 0, V | B): "4.8",
    (0, 1, V | B): "16.8",
    (0, 2, V | B): "8.8",
    (0, 3, V | B): "4.8",
    (0, 4, V | B): "4.8",
    (2, 1, V | OV): "6.8 4.8",
    (2, 2, V | OV): "4.8",
}
# kernel name -> why no option and no table under 2e6 rows reaches it (at most six; an entry nothing can ever pick is deleted instead)
UNREACHED: Dict[str, str] = {}


def _dots(s):
    return [tuple(int(v) for v in g.split(".")) for g in s.split()]


STAGED_CASES = [f"fused_filter_compact<{nc},{r},{v},{w},{f}>" for (nc, f), gs in STAGED.items() for r, v, w in _dots(gs)]
DIRECT_CASES = [f"fused_direct_compact<{p},{q},{r},{w},{f}>" for (p, q, f), gs in DIRECT.items() for r, w in _dots(gs)]
CASES = STAGED_CASES + DIRECT_CASES
# fused_redo_waves<NC,RR>: the staged geometry whose wave ranges redo_rows_per_lane (csrc/fused_full.hip) maps to it
REDO_CASES = {
    (1, 16): "fused_filter_compact<1,16,2,16,32>", (1, 8): "fused_filter_compact<1,8,2,16,32>", (1, 4): "fused_filter_compact<1,4,2,16,32>",
    (2, 8): f"fused_filter_compact<2,8,1,16,{V | A}>", (2, 4): f"fused_filter_compact<2,4,1,16,{V | A}>",
    (3, 4): f"fused_filter_compact<3,4,1,16,{V | A}>", (4, 4): f"fused_filter_compact<4,4,1,16,{V | A}>",
    (0, 4): f"fused_filter_compact<0,16,1,16,{V | B | XS | SEL}>",
}
# one kernel per distinct (rows per lane, waves) geometry of either table: many tiles per workgroup
MANY_TILES = [
    "fused_filter_compact<1,16,2,16,32>", "fused_filter_compact<1,8,2,16,32>", "fused_filter_compact<1,4,2,16,32>",
    "fused_filter_compact<1,24,2,16,32>", "fused_filter_compact<1,32,2,8,32>", "fused_filter_compact<1,16,2,8,32>",
    f"fused_filter_compact<2,12,2,16,{A}>", f"fused_filter_compact<3,4,1,8,{A}>",
    "fused_direct_compact<1,0,12,8,0>", "fused_direct_compact<1,0,8,8,0>", "fused_direct_compact<2,0,6,8,0>", "fused_direct_compact<2,0,4,8,0>",
    "fused_direct_compact<1,0,16,8,0>", "fused_direct_compact<1,0,16,16,0>", "fused_direct_compact<1,0,16,4,0>",
    "fused_direct_compact<1,2,4,16,0>", "fused_direct_compact<1,2,8,4,0>",
]

LITERALS = (999, 989, 899, 499, 49, -1)  # x > lit over 0..999 keeps none, 1 %, 10 %, half, 95 %, all
RUNS = ("head", "tail")                  # the first half of the rows survives and the second does not; the reverse
NEUTRAL = {"sample": -1, "segments": -1, "skew": -1, "groups_by_ranges": -1}  # nothing moves columns or launches away from the entry
RESET = {"rows_per_lane": 0, "vec": 0, "direct": 0, "direct_r": 0, "direct_waves": 0, "bools_in_pass": 0, "cap_rows": 0, "wgs_per_cu": 0,
         "sample": 0, "segments": 0, "skew": 0, "groups_by_ranges": 0}


@dataclass
class Query:
    """A query as a recipe over named columns.  `driver` decides which rows survive: "gt" x > lit; "lt" x < 999 - lit under the
    "least" policy (the null cells of x survive: the only way a tested column keeps an output bitmap); "bool" `k is true` over the
    Boolean column k = (x > lit).  columns: (name, kind, nullable) with kind "i" / "f" (Int64 / Float64 values) or "b" (Boolean)."""
    columns: List[Tuple[str, str, bool]] = field(default_factory=list)
    driver: str = "gt"
    tests: List[str] = field(default_factory=list)   # ride-along columns tested by `>= 0`: all their valid cells pass, their nulls drop
    keeps: List[str] = field(default_factory=list)   # ... tested by `!= -5` under "least": every cell passes, nulls included
    is_true: Optional[str] = None                    # a further Boolean column required to be true
    second_term: bool = False                        # x != 1000 as well: two terms over the one column
    expr: bool = False                               # (driver OR never) AND the rest: an OR tree, strict under "drops"
    proj: List[str] = field(default_factory=list)
    selection: bool = False
    options: Dict[str, int] = field(default_factory=dict)
    offset: int = 67


def _rides(count, nullable):
    return [(f"r{k}", "if"[k % 2], nullable) for k in range(count)]


def staged_query(nc, r, vec, waves, f):
    """The query whose launch is fused_filter_compact<nc,r,vec,waves,f>: one feature per flag bit of f, none for a bit f lacks
    (choose_launch asks for the instantiation with exactly the shape flags and the fewest feature flags that cover the launch)."""
    q = Query(options={"rows_per_lane": r | waves << 8, "vec": vec, "direct": -1}, offset=66 if vec == 2 else 67)
    if nc == 0:  # a Boolean-only predicate; a projected Boolean column rides in the pass (FF_XS) or is compacted behind it (needs FF_SEL)
        q.columns, q.driver, q.proj = [("k", "b", True), ("bx", "b", True)], "bool", ["bx"]
        q.expr, q.selection = bool(f & E), bool(f & SEL)
        if f & XS:
            q.options["bools_in_pass"] = 1
        return q
    if f & (I64 | F64):  # one compare term over the only column, no nulls, projected
        q.columns, q.proj, q.selection = [("x", "i" if f & I64 else "f", False)], ["x"], bool(f & SEL)
        return q
    rides = _rides(nc - 1, bool(f & V))
    if nc == 1 and (f & V) and (f & A) and not (f & N):
        # the one loaded column keeps its bitmap: under a Boolean predicate it is a column no term tests, else the tested column under "least"
        if f & B:
            q.driver, rides = "bool", _rides(1, True)
            q.columns = [("k", "b", True)] + rides
        else:
            q.driver = "lt"
            q.columns = [("x", "i", True)]
    else:
        q.columns = [("x", "i", bool(f & V) and nc == 1)] + rides
    if f & N:
        q.tests = [name for name, _, _ in rides]
    if f & A:
        q.proj = [name for name, kind, _ in q.columns if kind != "b"]
    else:
        q.proj = [name for name, _, _ in rides]
    if (f & B) and q.driver != "bool":
        q.columns.append(("t", "b", True))
        q.is_true = "t"
    if f & XS:
        q.columns.append(("bx", "b", True))
        q.proj.append("bx")
        q.options["bools_in_pass"] = 1
    q.selection, q.expr = bool(f & SEL), bool(f & E)
    q.second_term = nc == 1 and not (f & (V | B | XS | E))  # (or the launch is the one-term kernel's)
    return q


def direct_query(np_, nq, r, waves, f):
    """The query whose launch is fused_direct_compact<np_,nq,r,waves,f>: np_ 8-byte columns the terms read, nq that are only
    projected; FF_VALIDITY a nullable tested column, FF_BOOL an `is true` term, FF_OUTVALID a projected column that keeps nulls."""
    q = Query(options={"direct": 1, "direct_r": r, "direct_waves": waves, "vec": 1})
    rides = _rides(nq, bool(f & OV))
    if np_ == 0:
        q.driver, q.columns = "bool", [("k", "b", True)] + rides
        q.proj = [name for name, _, _ in rides]
        return q
    tested = [(f"p{k}", "fi"[k % 2], False) for k in range(np_ - 1)]
    if (f & OV) and nq == 0:  # a TESTED column keeps its nulls: "least", where < and != keep them
        q.driver = "lt"
        if tested:
            tested[0] = (tested[0][0], tested[0][1], True)
            q.columns = [("x", "i", False)] + tested
            q.keeps = [name for name, _, _ in tested]
        else:
            q.columns = [("x", "i", True)]
    else:
        q.columns = [("x", "i", bool(f & V) and not (f & OV))] + tested + rides
        q.tests = [name for name, _, _ in tested]
    q.proj = [name for name, kind, _ in q.columns]
    if f & B:
        q.columns.append(("t", "b", True))
        q.is_true = "t"
    return q


def parse(kernel):
    name, args = kernel[:-1].split("<")
    return name, tuple(int(v) for v in args.split(","))


def query_of(kernel):
    name, args = parse(kernel)
    return staged_query(*args) if name == "fused_filter_compact" else direct_query(*args)


def tile_rows(kernel):
    name, args = parse(kernel)
    return args[3] * 64 * args[1] if name == "fused_filter_compact" else args[3] * 64 * args[2]


# ---- data -------------------------------------------------------------------------------------------------------------------
def _valid(rng, n, nullable):
    return rng.random(n) >= 0.2 if nullable else None


def make_table(q, n, variant, seed=11):
    """(host columns, Predicate, projection) of query q over n rows.  variant: a literal of LITERALS over independent x in 0..999, or
    "head" / "tail" (x in runs: one half of the rows all survives, the other not at all).  Every column is a slice at q.offset of a
    longer one: row 0 sits at bit 2 or 3 of its bitmaps' first byte (and, at offset 66, still on a 16-byte boundary)."""
    rng = np.random.default_rng(seed)
    full = n + q.offset + 5
    if variant in RUNS:
        lit = 499
        keep = np.zeros(full, bool)
        half = q.offset + n // 2
        keep[:half] = True
        if variant == "tail":
            keep = ~keep
        x = np.where(keep, 750, 250).astype(np.int64)
    else:
        lit = variant
        x = rng.integers(0, 1000, full, dtype=np.int64)
    if q.driver == "lt":
        x = 999 - x  # x < 999 - lit keeps what x > lit kept before
    names = [name for name, _, _ in q.columns]
    cols = []
    for name, kind, nullable in q.columns:
        valid = _valid(rng, full, nullable)
        if name == "x":
            values = x if kind == "i" else x.astype(np.float64)
        elif name == "k":
            values = x > lit
        elif kind == "b":
            values = rng.random(full) < (0.9 if name == "t" else 0.5)
        elif kind == "i":
            values = rng.integers(0, 1 << 40, full, dtype=np.int64)
        else:
            values = rng.random(full) * 1e6
        if valid is not None and kind in "if":  # a placeholder 0 under a null would hide a slot that kept the cell's bytes
            values = np.where(valid, values, np.array(-7, values.dtype))
        cols.append(Column.from_numpy(values, valid).slice(q.offset, n))
    at = names.index
    if q.driver == "gt":
        terms = [Term(at("x"), ">", lit if q.columns[at("x")][1] == "i" else float(lit))]
    elif q.driver == "lt":
        terms = [Term(at("x"), "<", 999 - lit)]
    else:
        terms = [Term(at("k"), "is_true")]
    tree = None
    if q.expr:  # (driver OR a term nothing satisfies) AND every other term
        if q.driver == "bool":
            cols.append(Column.from_numpy(np.zeros(full, bool)).slice(q.offset, n))
            terms.append(Term(len(cols) - 1, "is_true"))
        else:
            terms.append(Term(at("x"), "<", -5))
        tree = ("or", 0, 1)
    if q.second_term:
        terms.append(Term(at("x"), "!=", 1000))
    for name in q.tests:
        terms.append(Term(at(name), ">=", 0 if q.columns[at(name)][1] == "i" else 0.0))
    for name in q.keeps:
        terms.append(Term(at(name), "!=", -5 if q.columns[at(name)][1] == "i" else -5.0))
    if q.is_true:
        terms.append(Term(at(q.is_true), "is_true"))
    if tree is not None and len(terms) > 2:
        tree = ("and", tree, *range(2, len(terms)))
    pred = Predicate(terms, "least" if q.driver == "lt" else "drops", tree)
    return cols, pred, [at(name) for name in q.proj]


def run_and_check(ctx, oracle, kernel, q, n, variant, what, calls=2):
    """The query over n rows, `calls` times on the same device columns (the second launch is sized from the first one's selectivity):
    the kernel named, the outputs, the survivor count and the selection bitmap are the oracle's, bit for bit."""
    cols, pred, proj = make_table(q, n, variant)
    want = oracle.filter_project(cols, pred, proj)
    want_sel, want_rows = oracle.eval_predicate(cols, pred)
    dev = [ctx.upload(c) for c in cols]
    for call in range(calls):
        where = f"{what} n={n} variant={variant} call={call}"
        outs, rows, sel = ctx.filter_project(dev, pred, proj, q.selection)
        assert ctx.last_kernel() == kernel, f"{where}: ran {ctx.last_kernel()}"
        assert rows == want_rows, f"{where}: {rows} rows survive, the oracle keeps {want_rows}"
        assert_columns_equal([o.download() for o in outs], want, where)
        if sel is not None:
            assert_columns_equal([sel.download()], [want_sel], f"{where} selection")
            sel.free()
        [o.free() for o in outs]
    [d.free() for d in dev]
    return want_rows


class options:
    """The entry's options and the neutral ones set for the block, every one of them back at its default afterwards."""

    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, {**NEUTRAL, **opts}

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in RESET.items():
            self.ctx.set_option(k, v)


def sizes_of(kernel):
    t = tile_rows(kernel)
    return [1, 65, t - 1, t, t + 1, 5 * t + 67]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", CASES)
def test_instantiation_matches_oracle(gpu_ctx, oracle, kernel):
    """Every table entry at row counts round its tile's seams, from no survivor to all of them and in runs that straddle a tile."""
    q = query_of(kernel)
    what = f"{kernel} options={q.options}"
    with options(gpu_ctx, q.options):
        for n in sizes_of(kernel):
            for variant in LITERALS + RUNS:
                run_and_check(gpu_ctx, oracle, kernel, q, n, variant, what)


@pytest.mark.gpu
@pytest.mark.parametrize("redo", sorted(REDO_CASES), ids=lambda r: f"fused_redo_waves<{r[0]},{r[1]}>")
def test_redo_instantiation_matches_oracle(gpu_ctx, oracle, redo):
    """LDS slots of 64 rows (option cap_rows, rounded up to a chunk) under dense and run-shaped selections: the waves' ranges outgrow
    them and are re-read by the redo kernel of that (columns, rows per lane) pair."""
    kernel = REDO_CASES[redo]
    q = query_of(kernel)
    q.options["cap_rows"] = 32
    what = f"fused_redo_waves<{redo[0]},{redo[1]}> behind {kernel} options={q.options}"
    t = tile_rows(kernel)
    with options(gpu_ctx, q.options):
        for n in (t + 1, 5 * t + 67):
            for variant in (49, -1) + RUNS:
                run_and_check(gpu_ctx, oracle, kernel, q, n, variant, what)
                assert gpu_ctx.get_option("last_redo_ppm") > 0, f"{what} n={n} variant={variant}: no wave range was left to the redo kernel"


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", MANY_TILES)
def test_many_tiles_per_workgroup(gpu_ctx, oracle, kernel):
    """One workgroup per CU (option wgs_per_cu) and two tiles for each of them: the scanner wave and the look-back between a workgroup's
    own tiles in every (rows per lane, waves) geometry, at 10 %."""
    q = query_of(kernel)
    q.options["wgs_per_cu"] = 1
    cus = gpu_ctx.device_info()["compute_units"]
    n = (2 * (cus - 1) - 1) * tile_rows(kernel) + 1  # the first row count with 2 (CUs - 1) tiles: workgroup 0 is the scanner
    what = f"{kernel} options={q.options}"
    with options(gpu_ctx, q.options):
        run_and_check(gpu_ctx, oracle, kernel, q, n, 899, what)


@pytest.mark.gpu
def test_ranged_launch_takes_the_lean_power_of_two_entry(gpu_ctx, oracle):
    """No geometry forced: two tested columns and one projected, with a Boolean column compacted behind the pass at its wave offsets.
    Ranges of 6 x 64 rows do not tile the 4096-row steps of that kernel, so find_direct passes <2,1,6,8,0> over and takes the first listed
    entry of 4 rows per lane that covers the launch -- the one without validity staging, not the FF_OUTVALID one listed for nullable outputs."""
    kernel = "fused_direct_compact<2,1,4,8,0>"
    q = direct_query(2, 1, 4, 8, 0)
    q.options = {"direct": 1}
    q.columns.append(("bx", "b", True))
    q.proj.append("bx")
    with options(gpu_ctx, q.options):
        for variant in (499, 49):
            run_and_check(gpu_ctx, oracle, kernel, q, 5 * tile_rows(kernel) + 67, variant, f"{kernel} options={q.options}")
