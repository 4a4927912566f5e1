"""The staging loop of the pass over narrow codes (csrc/fused_kernel.hpp, the `kNarrow != 0` branch; -m gpu): the term as ONE interval
of codes (narrow_term.hpp, fold_negate), the loop without per-row tests of what is the same for a whole tile, ranks clamped to the slot
instead of compared with its capacity -- against the oracle row for row, a few tiles per case.  Every case reads the geometry and the
FF_NARROW* flag of the kernel that ran from last_kernel(): a fallback to the plain kernel fails."""
import numpy as np
import pytest

from rivulus_amd import capi
from rivulus_amd.capi import Column, Predicate, Term

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NARROW16, NARROW32 = 4096, 8192  # FF_NARROW16 / FF_NARROW32 (csrc/scan_frontend.hpp)
OPS = ("==", "!=", "<", ">", "<=", ">=")
WAVES = 16
TALL = 32  # kNarrowTallRows (csrc/fused_table.hpp)
T = WAVES * 64 * TALL
VEC = 2  # the narrow instantiations load pairs


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own, packing at the first whole scan whatever the size (option narrow_codes = 1)."""
    c = capi.Context(0)
    c.set_option("narrow_codes", 1)
    yield c
    c.close()


class option:
    def __init__(self, ctx, **values):
        self.ctx, self.values = ctx, values

    def __enter__(self):
        for k, v in self.values.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            self.ctx.set_option(k, 0)


def ran(ctx):
    """(rows per lane, waves, flags) of the kernel of the last pass."""
    name = ctx.last_kernel()
    assert name.startswith("fused_filter_compact<"), name
    _, r, _, w, f = (int(x) for x in name[name.index("<") + 1:-1].split(","))
    return r, w, f


def assert_ran(ctx, r, flag, what=""):
    got = ran(ctx)
    assert got[0] == r and got[1] == WAVES and got[2] & (NARROW16 | NARROW32) == flag, (what, ctx.last_kernel(), r, flag)


def uniform(lo, hi, n, seed):
    offs = np.random.default_rng(seed).integers(0, hi - lo + 1, n, dtype=np.uint64)
    return (offs + np.uint64(lo % (1 << 64))).view(np.int64)


def check(ctx, oracle, dcol, hcol, pred, what):
    outs, rows, _ = ctx.filter_project([dcol], pred, [0])
    want = oracle.filter_project([hcol], pred, [0])
    diff = outs[0].download().same_as(want[0])
    assert diff is None and rows == want[0].length, f"{what}: {diff} ({rows} rows, oracle {want[0].length}; {ctx.last_kernel()})"
    return rows


def packed(ctx, oracle, values, width):
    """The column uploaded and scanned once (the scan that builds its companion reads the 8-byte values)."""
    h = Column.from_numpy(values)
    d = ctx.upload(h)
    builds = ctx.get_option("narrow_builds")
    check(ctx, oracle, d, h, Predicate([Term(0, "==", int(values[0]))]), "the first scan")
    assert ran(ctx)[2] & (NARROW16 | NARROW32) == 0 and ctx.get_option("narrow_builds") == builds + 1
    assert ctx.get_option("narrow_bytes") >= width * len(values)
    return d, h


def empty_in_code_space(op, lit, base):
    """narrow_term.hpp's lowering, restated: does `x op lit` come out as the complement of ALL 2^32 codes of a column with this minimum?"""
    lt, gt = op in ("<", "<=", "!="), op in (">", ">=", "!=")
    if lit < base:
        return not gt
    d = lit - base
    if d > 0xFFFFFFFF:
        return not lt
    return (op == "<" and d == 0) or (op == ">" and d == 0xFFFFFFFF)


# ---- operators: every folded form, and the one query without one ---------------------------------------------------------------------
# (name, smallest value, largest value, code bytes, predicates of the 36 that lower to the complement of all 2^32 codes: x < lo and
#  x < / <= / == lo - 1 everywhere; x > hi where hi's code is 2^32 - 1; x == / > / >= hi + 1 where that lies above every code and Int64
#  has it.  Over 2-byte codes the fold turns it into an interval above them; over 4-byte codes it is the one term without an interval)
COLUMNS = [("2-byte codes", 100, 1099, 2, 4), ("2-byte codes, the whole width", -5, 65530, 2, 4), ("4-byte codes", -70000, 70000, 4, 4),
           ("4-byte codes, the whole width", 1000, 1000 + (1 << 32) - 1, 4, 8), ("4-byte codes, max INT64_MAX", I64_MAX - (1 << 32) + 1, I64_MAX, 4, 5)]


@pytest.mark.parametrize("name,lo,hi,width,none", COLUMNS, ids=[c[0] for c in COLUMNS])
def test_operators_against_literals_around_both_ends(ctx, oracle, name, lo, hi, width, none):
    n = 2 * T + 5
    v = uniform(lo, hi, n, seed=width * 7 + (hi - lo) % 5)
    v[3], v[T + 11], v[n - 1], v[n - 2] = lo, hi, lo, hi
    d, h = packed(ctx, oracle, v, width)
    r, flag = (TALL, NARROW16) if width == 2 else (16, NARROW32)
    literals = [x for x in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1) if I64_MIN <= x <= I64_MAX]
    empties = 0
    with option(ctx, grid_limit=1):
        for op in OPS:
            for lit in literals:
                rows = check(ctx, oracle, d, h, Predicate([Term(0, op, lit)]), f"{name}: x {op} {lit}")
                # (the pass over codes for every one of them: tests/test_narrow_codes_gpu.py and test_narrow_pipeline_gpu.py pin it for
                # the empty set over 4-byte codes too, which is no interval -- it keeps its negate flag and runs the loop's second form)
                assert_ran(ctx, r, flag, f"{name}: x {op} {lit}")
                if empty_in_code_space(op, lit, lo):
                    assert rows == 0, (name, op, lit, rows)
                    empties += 1
    assert empties == none, (name, empties)


# ---- the ragged last tile: the loop's other form ------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [1, 2])
@pytest.mark.parametrize("n", [1, 127, 129, T - 1, T + 1, 2 * T + 5], ids=["1", "127", "129", "T-1", "T+1", "2T+5"])
def test_ragged_tail(ctx, oracle, n, limit):
    """Odd n: the last dword holds one live and one dead code.  `x < 900` keeps code 0, which is what lies past the companion's end:
    a dead code that was not masked would be counted."""
    v = uniform(0, 999, n, seed=n)
    v[n - 1] = 950
    d, h = packed(ctx, oracle, v, 2)
    with option(ctx, grid_limit=limit):
        for pred in (Predicate([Term(0, ">", 899)]), Predicate([Term(0, "<", 900)]), Predicate([Term(0, "!=", 950)])):
            check(ctx, oracle, d, h, pred, f"{n} rows, grid_limit {limit}")
            assert_ran(ctx, TALL, NARROW16, f"{n} rows")


# ---- the slot boundary: ranks are clamped, not tested --------------------------------------------------------------------------------
# Option cap_rows = 64 asks for the smallest slot; size_staged (csrc/fused_launch.hip) keeps a slot at least one chunk of 64 * VEC rows,
# so a wave of these instantiations stages CAP = 128 survivors and is left to the redo kernel from 129.  The counts the boundary is
# walked with: 63 / 64 / 65 around the option's value, CAP - 1 / CAP / CAP + 1 around the slot, and a whole wave range.
CAP = 64 * VEC
FILLS = [("63, 64, 65", (63, 64, 65), False), ("CAP - 1, CAP", (CAP - 1, CAP), False), ("CAP + 1", (CAP + 1,), True),
         ("a whole range", (-1,), True), ("all of them", (63, 64, 65, CAP - 1, CAP, CAP + 1, -1), True)]


def boundary_column(r, fills, seed):
    """Two tiles at r rows per lane + 5 rows; in tile 0 the chosen waves hold exactly `fills` survivors (-1: every row), the others 0
    and 1 alternately; tile 1 holds one survivor in 97 rows."""
    rows_per_wave, tile = 64 * r, WAVES * 64 * r
    n = 2 * tile + 5
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 900, n, dtype=np.int64)
    v[tile::97] = 901
    held = []
    for w in range(WAVES):
        k = fills[w // 2] if w % 2 == 0 and w // 2 < len(fills) else (w // 2) % 2
        k = rows_per_wave if k < 0 else k
        at = w * rows_per_wave + rng.choice(rows_per_wave, k, replace=False)
        v[at] = 900 + rng.integers(0, 100, k)
        held.append(k)
    assert [int((v[w * rows_per_wave:(w + 1) * rows_per_wave] > 899).sum()) for w in range(WAVES)] == held
    return v, held


@pytest.mark.parametrize("name,fills,redo", FILLS, ids=[f[0] for f in FILLS])
def test_slot_boundary_at_the_tall_geometry(ctx, oracle, name, fills, redo):
    v, held = boundary_column(TALL, fills, seed=len(fills) + 31)
    d, h = packed(ctx, oracle, v, 2)
    pred = Predicate([Term(0, ">", 899)])
    reruns = ctx.get_option("overflow_reruns")
    with option(ctx, grid_limit=1, cap_rows=64, rows_per_lane=TALL | WAVES << 8):
        check(ctx, oracle, d, h, pred, name)
        assert_ran(ctx, TALL, NARROW16, name)
        assert (ctx.get_option("last_redo_ppm") != 0) == redo == any(k > CAP for k in held), (name, held, ctx.get_option("last_redo_ppm"))
    assert ctx.get_option("overflow_reruns") == reruns


@pytest.mark.parametrize("name,fills,redo", FILLS, ids=[f[0] for f in FILLS])
def test_slot_boundary_at_the_seam_geometry(ctx, oracle, name, fills, redo):
    """16 rows per lane through a chunked window with per-batch counts: a 1024-row batch is one wave range."""
    v, held = boundary_column(16, fills, seed=len(fills) + 57)
    n = len(v)
    d, h = packed(ctx, oracle, v, 2)
    pred = Predicate([Term(0, ">", 899)])
    reruns = ctx.get_option("overflow_reruns")
    with option(ctx, grid_limit=1, cap_rows=64, rows_per_lane=16 | WAVES << 8):
        outs, counts, _, total = ctx.filter_project_chunked([d], 1024, pred, [0])
        assert_ran(ctx, 16, NARROW16, name)
        assert (ctx.get_option("last_redo_ppm") != 0) == redo == any(k > CAP for k in held), (name, held, ctx.get_option("last_redo_ppm"))
    assert ctx.get_option("overflow_reruns") == reruns
    assert np.array_equal(np.array(counts, dtype=np.uint64), np.add.reduceat((v > 899).astype(np.uint64), np.arange(0, n, 1024)))
    assert list(np.array(counts[:WAVES], dtype=np.int64)) == held and total == int((v > 899).sum())
    assert outs[0].download().same_as(oracle.filter_project([h], pred, [0])[0]) is None


# ---- the dump cell: lanes without a survivor must write into no slot -----------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2])
def test_dump_cell_leaks_into_no_slot(ctx, oracle, depth):
    """A tile where nothing survives, one where every second row does (every wave outgrows its slot), one where a tenth does (every
    slot is flushed, with whatever the tiles before left in the LDS block), all walked by one workgroup."""
    n = 3 * T
    v = np.zeros(n, dtype=np.int64)
    v[T:2 * T:2] = 900 + (np.arange(T // 2) % 100)
    tenth = np.random.default_rng(depth).choice(T, T // 10, replace=False)
    v[2 * T + tenth] = 901 + (tenth % 90)
    d, h = packed(ctx, oracle, v, 2)
    with option(ctx, grid_limit=1, depth=depth, rows_per_lane=TALL | WAVES << 8):
        check(ctx, oracle, d, h, Predicate([Term(0, ">", 899)]), f"depth {depth}")
        assert_ran(ctx, TALL, NARROW16, f"depth {depth}")
        assert ctx.get_option("last_redo_ppm") > 0


# ---- nothing projected: the loop's other form counts and stores nothing ---------------------------------------------------------
def test_count_only(ctx, oracle):
    n = 2 * T + 5
    v = uniform(0, 999, n, seed=3)
    d, h = packed(ctx, oracle, v, 2)
    with option(ctx, grid_limit=1):
        outs, rows, _ = ctx.filter_project([d], Predicate([Term(0, ">", 899)]), [])
        assert_ran(ctx, TALL, NARROW16, "count only")
    assert outs == [] and rows == int((v > 899).sum())
