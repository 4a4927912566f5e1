"""The pass over PACKED narrow codes (csrc/narrow_rule.hpp: 10-bit codes, six per 8-byte word; FF_NARROW16 | FF_PACK10 of the lean filter
pass, 48 rows per lane; -m gpu) against the oracle, row for row, under option narrow_codes = 2: row counts around every boundary of the
layout and the geometry, value ranges on both sides of the packed width and at the ends of Int64, every operator and literal kind, the
slot boundary and the redo kernel, the overflow re-run at every packed geometry, a launch that projects nothing, views that can and
cannot read the packed codes with the second companion they end on, and the option's other values.  Every case reads the geometry and
the flags of the kernel that ran from last_kernel(): a fallback to another kernel fails."""
import numpy as np
import pytest

from helpers import const
from rivulus_amd import capi
from rivulus_amd.capi import RV_INT64, Column, Predicate, Term, synth_spec

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NARROW16, NARROW32, PACK10 = 4096, 8192, 16384  # FF_NARROW16 / FF_NARROW32 / FF_PACK10 (csrc/scan_frontend.hpp)
CODES = NARROW16 | NARROW32 | PACK10
PACKED = NARROW16 | PACK10
OPS = ("==", "!=", "<", ">", "<=", ">=")
WAVES = 16
TALL = 48        # kPackedTallRows (csrc/fused_table.hpp)
TALL16 = 32      # kNarrowTallRows: 2-byte codes
RANGE = 64 * TALL  # one wave range
T = WAVES * RANGE  # one tile
VEC = 2


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own, packing at the first whole scan whatever the size, packed where the rule allows."""
    c = capi.Context(0)
    c.set_option("narrow_codes", 2)
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


def assert_ran(ctx, r, codes, what=""):
    got = ran(ctx)
    assert got[0] == r and got[1] == WAVES and got[2] & CODES == codes, (what, ctx.last_kernel(), r, codes)


def uniform(lo, hi, n, seed):
    offs = np.random.default_rng(seed).integers(0, hi - lo + 1, n, dtype=np.uint64)
    return (offs + np.uint64(lo % (1 << 64))).view(np.int64)


def check(ctx, oracle, dcol, hcol, pred, what, proj=(0,)):
    outs, rows, _ = ctx.filter_project([dcol], pred, list(proj))
    want = oracle.filter_project([hcol], pred, [0])
    assert rows == want[0].length, f"{what}: {rows} rows, oracle {want[0].length}; {ctx.last_kernel()}"
    if proj:
        diff = outs[0].download().same_as(want[0])
        assert diff is None, f"{what}: {diff} ({ctx.last_kernel()})"
    return rows


def companion(ctx, oracle, values, nbytes):
    """The column uploaded and scanned whole once: the scan that builds its companion reads the 8-byte values.  nbytes: what the
    companion must take (the packed layout: whole super-groups of 384 elements in 512 bytes).  That scan keeps nothing: a case that
    runs the same predicate again finds a selectivity of 0 remembered for it, which sends no launch to the direct kernel."""
    h = Column.from_numpy(values)
    d = ctx.upload(h)
    builds, before = ctx.get_option("narrow_builds"), ctx.get_option("narrow_bytes")
    assert check(ctx, oracle, d, h, Predicate([Term(0, "<", int(values.min()))]), "the first scan") == 0
    assert ran(ctx)[2] & CODES == 0 and ctx.get_option("narrow_builds") == builds + 1
    assert ctx.get_option("narrow_bytes") == before + nbytes, (len(values), ctx.get_option("narrow_bytes") - before, nbytes)
    return d, h


def packed_bytes(n):
    return (n + 383) // 384 * 512


# ---- rows: every boundary of the layout (128-row group, 384-element super-group) and of the geometry (wave range, tile) ------------------
ROWS = [1, 383, 384, 385, RANGE - 1, RANGE, RANGE + 1, T - 1, T, T + 1, 3 * T + T // 5 + 7]


@pytest.mark.parametrize("limit", [1, 0], ids=["one workgroup", "several workgroups"])
@pytest.mark.parametrize("n", ROWS)
def test_row_counts(ctx, oracle, n, limit):
    """`x < 900` keeps code 0, which is what the padding of the last super-group holds and what lies past the companion: a dead code
    that was not masked would be counted.  The last row is a survivor of `x > 899`, the row before it is not."""
    v = uniform(0, 999, n, seed=n)
    v[n - 1] = 950
    if n >= 2:
        v[n - 2], v[0] = 0, 999
    d, h = companion(ctx, oracle, v, packed_bytes(n))
    with option(ctx, grid_limit=limit):
        for pred in (Predicate([Term(0, ">", 899)]), Predicate([Term(0, "<", 900)]), Predicate([Term(0, "!=", 950)]), Predicate([Term(0, "==", 999)])):
            check(ctx, oracle, d, h, pred, f"{n} rows, grid_limit {limit}")
            assert_ran(ctx, TALL, PACKED, f"{n} rows")


# ---- values: both sides of the packed width, both ends of Int64, every operator against literals around both ends -------------------------
# (name, smallest, largest, flags of the kernel, rows per lane, bytes per element or None: packed)
COLUMNS = [("range 1023", 100, 1123, PACKED, TALL, None), ("range 1024: 2-byte codes", 100, 1124, NARROW16, TALL16, 2), ("range 0", 41, 41, PACKED, TALL, None),
           ("negative base", -1000, -1, PACKED, TALL, None), ("base INT64_MIN", I64_MIN, I64_MIN + 1023, PACKED, TALL, None),
           ("top INT64_MAX", I64_MAX - 1023, I64_MAX, PACKED, TALL, None)]


@pytest.mark.parametrize("name,lo,hi,codes,r,width", COLUMNS, ids=[c[0] for c in COLUMNS])
def test_operators_against_literals_around_both_ends(ctx, oracle, name, lo, hi, codes, r, width):
    n = T + 2 * RANGE + 5
    v = uniform(lo, hi, n, seed=(hi - lo) % 7 + 3)
    v[3], v[T + 11], v[n - 1], v[n - 2] = lo, hi, lo, hi
    d, h = companion(ctx, oracle, v, packed_bytes(n) if width is None else width * n)
    mid = lo + (hi - lo) // 2
    literals = sorted({x for x in (lo - 1, lo, lo + 1, mid, hi - 1, hi, hi + 1, I64_MIN, I64_MAX) if I64_MIN <= x <= I64_MAX})
    empty = full = 0
    with option(ctx, grid_limit=1):
        for op in OPS:
            for lit in literals:
                rows = check(ctx, oracle, d, h, Predicate([Term(0, op, lit)]), f"{name}: x {op} {lit}")
                assert_ran(ctx, r, codes, f"{name}: x {op} {lit}")
                empty += rows == 0
                full += rows == n
    assert empty >= 4 and full >= 4, (name, empty, full)  # (x < lo, x > hi, ... and their complements)


# ---- the slot boundary: ranks are clamped, not tested -----------------------------------------------------------------------------
# Option cap_rows = 64 asks for the smallest slot; a slot holds at least one chunk of 64 * VEC rows, so a wave stages CAP = 128
# survivors and is left to the redo kernel from 129.
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


@pytest.mark.parametrize("r", [TALL, 24, 12])
@pytest.mark.parametrize("name,fills,redo", FILLS, ids=[f[0] for f in FILLS])
def test_slot_boundary(ctx, oracle, name, fills, redo, r):
    v, held = boundary_column(r, fills, seed=len(fills) + r)
    d, h = companion(ctx, oracle, v, packed_bytes(len(v)))
    pred = Predicate([Term(0, ">", 899)])
    reruns = ctx.get_option("overflow_reruns")
    with option(ctx, grid_limit=1, cap_rows=64, rows_per_lane=r | WAVES << 8):
        check(ctx, oracle, d, h, pred, name)
        assert_ran(ctx, r, PACKED, name)
        assert (ctx.get_option("last_redo_ppm") != 0) == redo == any(k > CAP for k in held), (name, held, ctx.get_option("last_redo_ppm"))
    assert ctx.get_option("overflow_reruns") == reruns


def test_values_are_the_plain_pass_s(ctx, oracle):
    """The same clustered column through a context that never builds codes: identical values, dense waves through the redo kernel."""
    v, held = boundary_column(TALL, (CAP + 1, -1, 64), seed=77)
    h = Column.from_numpy(v)
    pred = Predicate([Term(0, ">", 899)])
    plain = capi.Context(0)
    try:
        plain.set_option("narrow_codes", -1)
        pd = plain.upload(h)
        p_outs, p_rows, _ = plain.filter_project([pd], pred, [0])
        assert plain.get_option("narrow_builds") == 0 and ran(plain)[2] & CODES == 0
        p_values = p_outs[0].download()
    finally:
        plain.close()
    d, _ = companion(ctx, oracle, v, packed_bytes(len(v)))
    with option(ctx, grid_limit=1, cap_rows=64, rows_per_lane=TALL | WAVES << 8):
        outs, rows, _ = ctx.filter_project([d], pred, [0])
        assert_ran(ctx, TALL, PACKED)
        assert ctx.get_option("last_redo_ppm") > 0
    assert rows == p_rows and outs[0].download().same_as(p_values) is None


# ---- the dump cell: lanes without a survivor must write into no slot ----------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2])
def test_dump_cell_leaks_into_no_slot(ctx, oracle, depth):
    """A tile where nothing survives, one where every second row does (every wave outgrows its slot), one where a twentieth does (every
    slot is flushed, with whatever the tiles before left in the LDS block), all walked by one workgroup."""
    n = 3 * T
    v = np.zeros(n, dtype=np.int64)
    v[T:2 * T:2] = 900 + (np.arange(T // 2) % 100)
    some = np.random.default_rng(depth).choice(T, T // 20, replace=False)
    v[2 * T + some] = 901 + (some % 90)
    d, h = companion(ctx, oracle, v, packed_bytes(n))
    with option(ctx, grid_limit=1, depth=depth, rows_per_lane=TALL | WAVES << 8):
        check(ctx, oracle, d, h, Predicate([Term(0, ">", 899)]), f"depth {depth}")
        assert_ran(ctx, TALL, PACKED, f"depth {depth}")
        assert ctx.get_option("last_redo_ppm") > 0


# ---- output overflow: the re-run over the 8-byte values by the plain instantiation of the pass's geometry -------------------------------
@pytest.mark.parametrize("r", [TALL, 24, 12])
def test_overflow_rerun(ctx, oracle, r):
    tile = WAVES * 64 * r
    n = 2 * tile + 5
    v = uniform(0, 999, n, seed=r)  # ~10 % survive: far more than two rows per million + 1024
    d, h = companion(ctx, oracle, v, packed_bytes(n))
    pred = Predicate([Term(0, ">", 899)])
    reruns = ctx.get_option("overflow_reruns")
    with option(ctx, out_sizing=2, rows_per_lane=r | WAVES << 8):
        check(ctx, oracle, d, h, pred, f"overflow re-run at {r} rows per lane")
        assert_ran(ctx, r, PACKED, f"{r} rows per lane")
    assert ctx.get_option("overflow_reruns") == reruns + 1
    check(ctx, oracle, d, h, pred, "and without the overflow")
    assert ctx.get_option("overflow_reruns") == reruns + 1


# ---- nothing projected: the loop's other form counts and stores nothing ------------------------------------------------------------
def test_count_only(ctx, oracle):
    n = 2 * T + 5
    v = uniform(0, 999, n, seed=3)
    d, h = companion(ctx, oracle, v, packed_bytes(n))
    with option(ctx, grid_limit=1):
        outs, rows, _ = ctx.filter_project([d], Predicate([Term(0, ">", 899)]), [])
        assert_ran(ctx, TALL, PACKED, "count only")
    assert outs == [] and rows == int((v > 899).sum())


# ---- views: who reads the packed codes, and the second companion ------------------------------------------------------------------
def test_views_and_the_second_companion(ctx, oracle):
    n = 2 * T + 5
    v = uniform(0, 999, n, seed=21)
    d, h = companion(ctx, oracle, v, packed_bytes(n))
    pred = Predicate([Term(0, ">", 899)])
    want_counts = np.add.reduceat((v > 899).astype(np.uint64), np.arange(0, n, 1024))
    builds, nbytes = ctx.get_option("narrow_builds"), ctx.get_option("narrow_bytes")

    def sliced(off, length, codes, r):
        check(ctx, oracle, d.slice(off, length), h.slice(off, length), pred, f"slice {off}+{length}")
        got = ran(ctx)
        assert got[2] & CODES == codes and (r is None or got[0] == r), (off, length, ctx.last_kernel())

    for length in (n - 384, T, 17):
        sliced(384, length, PACKED, TALL)          # starts on a super-group: the packed codes
    sliced(768, n - 768, PACKED, TALL)
    for off in (2, 128, 3):
        for length in (n - off, 1024):
            sliced(off, length, 0, None)           # not on a super-group: the 8-byte values, the same result
    assert ctx.get_option("narrow_builds") == builds  # (slices read again and again complete no whole scan)
    # a launch with per-batch counts cannot read them either -- and completes a whole scan of its own: 2-byte codes beside the packed ones
    outs, counts, _, total = ctx.filter_project_chunked([d], 1024, pred, [0])
    assert ran(ctx)[2] & CODES == 0 and ran(ctx)[0] == 16
    assert np.array_equal(np.array(counts, dtype=np.uint64), want_counts) and total == int(want_counts.sum())
    assert outs[0].download().same_as(oracle.filter_project([h], pred, [0])[0]) is None
    assert ctx.get_option("narrow_builds") == builds + 1 and ctx.get_option("narrow_bytes") == nbytes + 2 * n
    # from here on every launch runs on the codes it can read
    outs, counts, _, total = ctx.filter_project_chunked([d], 1024, pred, [0])
    assert_ran(ctx, 16, NARROW16, "a window with per-batch counts")
    assert np.array_equal(np.array(counts, dtype=np.uint64), want_counts) and total == int(want_counts.sum())
    assert outs[0].download().same_as(oracle.filter_project([h], pred, [0])[0]) is None
    sliced(2, n - 2, NARROW16, TALL16)
    sliced(128, 1024, NARROW16, TALL16)
    sliced(3, n - 3, 0, None)                      # an odd element: neither layout
    sliced(384, n - 384, PACKED, TALL)
    sliced(0, n, PACKED, TALL)
    assert ctx.get_option("narrow_builds") == builds + 1


# ---- the option's other values ----------------------------------------------------------------------------------------------------
def test_option_1_builds_2_byte_codes_and_minus_1_nothing(oracle):
    n = 2 * T + 5
    v = uniform(0, 999, n, seed=9)
    h = Column.from_numpy(v)
    pred = Predicate([Term(0, ">", 899)])
    for value, codes, r, nbytes in ((1, NARROW16, TALL16, 2 * n), (-1, 0, 16, 0)):
        c = capi.Context(0)
        try:
            c.set_option("narrow_codes", value)
            d = c.upload(h)
            for _ in range(3):
                check(c, oracle, d, h, pred, f"narrow_codes = {value}")
            assert_ran(c, r, codes, f"narrow_codes = {value}")
            assert c.get_option("narrow_builds") == (1 if nbytes else 0) and c.get_option("narrow_bytes") == nbytes
        finally:
            c.close()


def test_auto_mode_ends_on_the_packed_kernel():
    """Option narrow_codes = 0 on the benchmark's own generator at kNarrowFromRows rows: whole-column launches trigger the packed layout."""
    rows = const("kNarrowFromRows")
    auto = capi.Context(0)
    try:
        x = auto.generate(synth_spec(RV_INT64, seed=42, length=rows))
        pred = Predicate([Term(0, ">", 899)])
        first = None
        for scan in range(1, const("kNarrowAfterWholeScans") + 3):
            outs, got, _ = auto.filter_project([x], pred, [0])
            if first is None:
                first, want = outs[0].download(), got
            else:
                assert got == want and outs[0].download().same_as(first) is None
            if scan <= const("kNarrowAfterWholeScans"):
                assert ran(auto)[2] & CODES == 0, (scan, auto.last_kernel())
            else:
                assert_ran(auto, TALL, PACKED, f"scan {scan}")
        assert auto.get_option("narrow_builds") == 1 and auto.get_option("narrow_bytes") == packed_bytes(rows)
    finally:
        auto.close()
