"""The pass over narrow codes as a pipeline (csrc/fused_kernel.hpp, the `kNarrow != 0` branches; -m gpu): raw code pairs requested a
tile ahead, the compare in code space (narrow_term.hpp) and survivors staged as codes and widened at the flush -- against the oracle
row for row.  Option grid_limit makes ONE or TWO workgroups walk every tile of a table of a few hundred thousand rows, so that the
prefetch, the slot stages and the ticket ring wrap; without it every workgroup of the persistent grid gets one tile at most.
Every case reads the geometry and the FF_NARROW* flag of the kernel that ran from last_kernel(): a fallback to the plain kernel fails."""
import math

import numpy as np
import pytest

from helpers import const
from rivulus_amd import capi
from rivulus_amd.capi import Column, Predicate, Term

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NARROW16, NARROW32 = 4096, 8192  # FF_NARROW16 / FF_NARROW32 (csrc/scan_frontend.hpp)
OPS = ("==", "!=", "<", ">", "<=", ">=")
WAVES = 16
TALL = 32  # kNarrowTallRows (csrc/fused_table.hpp): rows per lane of a pass over 2-byte codes without per-batch counts
T = WAVES * 64 * TALL  # its tile
STAGE_BUDGET, STAGES = 144 * 1024, 3  # size_staged (csrc/fused_launch.hip): LDS of a 16-wave launch, slot stages


def tile(r):
    return WAVES * 64 * r


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own, packing at the first whole scan whatever the size (option narrow_codes = 1)."""
    c = capi.Context(0)
    c.set_option("narrow_codes", 1)
    yield c
    c.close()


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
    """n Int64 values spread over [lo, hi] (Python integers: the range may be all of a code width at either end of Int64)."""
    offs = np.random.default_rng(seed).integers(0, hi - lo + 1, n, dtype=np.uint64)
    return (offs + np.uint64(lo % (1 << 64))).view(np.int64)


def check(ctx, oracle, dcol, hcol, pred, what):
    outs, rows, _ = ctx.filter_project([dcol], pred, [0])
    want = oracle.filter_project([hcol], pred, [0])
    diff = outs[0].download().same_as(want[0])
    assert diff is None and rows == want[0].length, f"{what}: {diff} ({rows} rows, oracle {want[0].length}; {ctx.last_kernel()})"
    return outs


def packed(ctx, oracle, values, width):
    """The column uploaded and scanned once (the scan that builds its companion reads the 8-byte values)."""
    h = Column.from_numpy(values)
    d = ctx.upload(h)
    builds = ctx.get_option("narrow_builds")
    check(ctx, oracle, d, h, Predicate([Term(0, "==", int(values[0]))]), "the first scan")
    assert ran(ctx)[2] & (NARROW16 | NARROW32) == 0 and ctx.get_option("narrow_builds") == builds + 1
    assert ctx.get_option("narrow_bytes") >= width * len(values)
    return d, h


def limited(ctx, k):
    class _Limit:
        def __enter__(self):
            ctx.set_option("grid_limit", k)

        def __exit__(self, *exc):
            ctx.set_option("grid_limit", 0)
    return _Limit()


# ---- pipeline edges: fewer tiles than the prefetch depth, exactly as many, and enough for sets and ring to wrap ----------------
@pytest.mark.parametrize("limit", [1, 2])
@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 5, 3 * T + 5, 4 * T + 5, 9 * T + 5], ids=["T-1", "T", "T+1", "2T+5", "3T+5", "4T+5", "9T+5"])
def test_pipeline_edges_at_the_tall_geometry(ctx, oracle, n, limit):
    d, h = packed(ctx, oracle, uniform(0, 999, n, seed=n), 2)
    with limited(ctx, limit):
        check(ctx, oracle, d, h, Predicate([Term(0, ">", 899)]), f"{n} rows, grid_limit {limit}")
        assert_ran(ctx, TALL, NARROW16)


def test_the_stamped_instantiations_compute_the_same(ctx, oracle):
    """Option stamp: the diagnostic instantiations of the pass over 2-byte codes (phase cycle sums), tall and at 16 rows per lane."""
    FF_STAMP = 16
    n = 4 * T + 5
    v = uniform(0, 999, n, seed=21)
    d, h = packed(ctx, oracle, v, 2)
    pred = Predicate([Term(0, ">", 899)])
    ctx.set_option("stamp", 1)
    try:
        with limited(ctx, 1):
            check(ctx, oracle, d, h, pred, "stamped, tall")
            assert_ran(ctx, TALL, NARROW16)
            assert ran(ctx)[2] & FF_STAMP
            outs, counts, _, total = ctx.filter_project_chunked([d], 1024, pred, [0])
            assert_ran(ctx, 16, NARROW16)
            assert ran(ctx)[2] & FF_STAMP and total == int((v > 899).sum())
            assert np.array_equal(np.array(counts, dtype=np.uint64), np.add.reduceat((v > 899).astype(np.uint64), np.arange(0, n, 1024)))
            assert outs[0].download().same_as(oracle.filter_project([h], pred, [0])[0]) is None
    finally:
        ctx.set_option("stamp", 0)


# ---- the other geometries: what the crowding rule of choose_launch walks down to ------------------------------------------------
def crowded(seen, r):
    """choose_launch's rule, from the constants: a wave's expected survivors (+ margin and sigmas) against its slot."""
    rows = 64 * r
    cap = min(rows, (STAGE_BUDGET // (STAGES * WAVES * 8)) & ~63)
    expect = seen * rows
    return cap < rows and expect * const("kCrowdedMargin") + const("kCrowdedSigmas") * math.sqrt(expect) > cap


def walked_to(seen, start):
    """The geometry a second call with a predicate that kept `seen` of the rows runs at: down the 16-wave list from `start`."""
    order = [r for r in (32, 16, 8, 4) if r <= start]
    for r in order:
        if not crowded(seen, r):
            return r
    return order[-1]


def chunked_reference(h, pred):
    """Values and per-batch counts of the plain path: a context that never packs."""
    plain = capi.Context(0)
    try:
        plain.set_option("narrow_codes", -1)
        pd = plain.upload(h)
        outs, counts, _, total = plain.filter_project_chunked([pd], 1024, pred, [0])
        assert plain.get_option("narrow_builds") == 0 and ran(plain)[2] & (NARROW16 | NARROW32) == 0
        return outs[0].download(), np.array(counts, dtype=np.uint64), total
    finally:
        plain.close()


GEOMETRIES = [  # (code width, value range, rows per lane, share of the rows the predicate keeps)
    (2, (0, 999), 16, 0.10), (2, (0, 999), 8, 0.40), (2, (0, 999), 4, 0.70),
    (4, (-70000, 70000), 16, 0.10), (4, (-70000, 70000), 8, 0.40), (4, (-70000, 70000), 4, 0.70),
]


@pytest.mark.parametrize("width,span,r,keep", GEOMETRIES, ids=[f"{g[0]}-byte codes, {g[2]} rows per lane" for g in GEOMETRIES])
def test_other_geometries_through_chunked_windows(ctx, oracle, width, span, r, keep):
    """1024-row batches with per-batch counts: 16 rows per lane by default, 8 and 4 where the rule finds the slots crowded on the
    second call with the predicate; counts against numpy and against a context that never packs, values against both and the oracle."""
    lo, hi = span
    n = 9 * tile(r) + 5
    lit = hi - int((hi - lo + 1) * keep)
    v = uniform(lo, hi, n, seed=1000 * width + r)
    seen = float((v > lit).mean())
    assert walked_to(seen, 16) == r, (seen, r)  # the choice, from the rule's constants
    pred = Predicate([Term(0, ">", lit)])
    d, h = packed(ctx, oracle, v, width)
    ctx.set_option("direct", -1)  # (from 55 % on a launch would take the direct kernel instead of walking down)
    try:
        with limited(ctx, 1):
            for call in range(2):  # the second call knows the predicate's selectivity
                outs, counts, _, total = ctx.filter_project_chunked([d], 1024, pred, [0])
            assert_ran(ctx, r, NARROW16 if width == 2 else NARROW32, f"selectivity {seen}")
    finally:
        ctx.set_option("direct", 0)
    want_counts = np.add.reduceat((v > lit).astype(np.uint64), np.arange(0, n, 1024))
    p_values, p_counts, p_total = chunked_reference(h, pred)
    assert np.array_equal(np.array(counts, dtype=np.uint64), want_counts) and np.array_equal(p_counts, want_counts) and total == p_total
    got = outs[0].download()
    assert got.same_as(p_values) is None  # bit-identical to the plain path
    assert got.same_as(oracle.filter_project([h], pred, [0])[0]) is None


def test_nine_tall_tiles_are_bit_identical_to_the_plain_path(ctx, oracle):
    n = 9 * T + 5
    v = uniform(0, 999, n, seed=77)
    pred = Predicate([Term(0, ">", 899)])
    d, h = packed(ctx, oracle, v, 2)
    with limited(ctx, 1):
        outs = check(ctx, oracle, d, h, pred, "narrow")
        assert_ran(ctx, TALL, NARROW16)
    plain = capi.Context(0)
    try:
        plain.set_option("narrow_codes", -1)
        p_outs, rows, _ = plain.filter_project([plain.upload(h)], pred, [0])
        assert ran(plain)[2] & (NARROW16 | NARROW32) == 0
        assert outs[0].download().same_as(p_outs[0].download()) is None and rows == int((v > 899).sum())
    finally:
        plain.close()


# ---- code-space edges across tiles ------------------------------------------------------------------------------------------------
EDGES = [("2-byte, base INT64_MIN", I64_MIN, I64_MIN + 65535, 2), ("2-byte, max INT64_MAX", I64_MAX - 65535, I64_MAX, 2),
         ("4-byte, base INT64_MIN", I64_MIN, I64_MIN + (1 << 32) - 1, 4), ("4-byte, max INT64_MAX", I64_MAX - (1 << 32) + 1, I64_MAX, 4)]


@pytest.mark.parametrize("name,lo,hi,width", EDGES, ids=[e[0] for e in EDGES])
def test_code_space_edges_across_tiles(ctx, oracle, name, lo, hi, width):
    """Code 0 and the largest code in the first, a middle and the last (ragged) tile; every operator against literals on and just
    outside both ends of the values and at the ends of Int64.  Each predicate is new to the context: the default geometry of its class."""
    r = TALL if width == 2 else 16
    n = 3 * tile(r) + 5
    v = uniform(lo, hi, n, seed=width)
    for at in (7, tile(r) + 4001, 3 * tile(r) + 1):
        v[at], v[at + 2] = lo, hi
    d, h = packed(ctx, oracle, v, width)
    literals = sorted({lo, hi, I64_MIN, I64_MAX} | ({lo - 1} if lo > I64_MIN else set()) | ({hi + 1} if hi < I64_MAX else set()))
    with limited(ctx, 1):
        for op in OPS:
            for lit in literals:
                check(ctx, oracle, d, h, Predicate([Term(0, op, lit)]), f"{name}: x {op} {lit}")
                assert_ran(ctx, r, NARROW16 if width == 2 else NARROW32, f"{name}: x {op} {lit}")


# ---- tail slices: the request for the next tile runs into the end of the companion -------------------------------------------------------
def test_tail_slices(ctx, oracle):
    n = 4 * T + 5
    d, h = packed(ctx, oracle, uniform(0, 999, n, seed=5), 2)
    pred = Predicate([Term(0, ">", 899)])
    with limited(ctx, 1):
        for end in (n, n - 2):  # at the buffer's last row; one pair before it
            for length in (17, T + 3, 2 * T + 1):
                off = end - length
                assert off % 2 == 0
                check(ctx, oracle, d.slice(off, length), h.slice(off, length), pred, f"slice {off}+{length}")
                assert_ran(ctx, TALL, NARROW16, f"slice {off}+{length}")
                # an odd element offset is not aligned for the pair loads: the plain kernel, the same result
                check(ctx, oracle, d.slice(off + 1, length - 1), h.slice(off + 1, length - 1), pred, f"slice {off + 1}+{length - 1}")
                assert ran(ctx)[2] & (NARROW16 | NARROW32) == 0, ctx.last_kernel()


# ---- redo and overflow behind the pipeline ------------------------------------------------------------------------------------------
def test_redo_and_overflow_behind_the_pipeline(ctx, oracle):
    """Runs of survivors longer than a wave's LDS slot in tiles 1 and 4 of six, all walked by one workgroup: those wave ranges go to
    the redo kernel (which reads the 8-byte values), the others flush codes.  Then outputs sized far too small: the pass counts
    exactly and its plain twin re-runs it."""
    n = 6 * T
    v = np.zeros(n, dtype=np.int64)
    v[::97] = 901
    v[T + 5000:T + 8000] = 900 + (np.arange(3000) % 50)
    v[4 * T + 20000:4 * T + 23000] = 950
    d, h = packed(ctx, oracle, v, 2)
    pred = Predicate([Term(0, ">", 899)])
    with limited(ctx, 1):
        check(ctx, oracle, d, h, pred, "clustered")
        assert_ran(ctx, TALL, NARROW16)
        assert ctx.get_option("last_redo_ppm") > 0
        reruns = ctx.get_option("overflow_reruns")
        ctx.set_option("out_sizing", 2)  # two rows per million + 1024: far below the ~8000 survivors
        try:
            check(ctx, oracle, d, h, pred, "overflow re-run")
            assert_ran(ctx, TALL, NARROW16)
            assert ctx.get_option("overflow_reruns") == reruns + 1
        finally:
            ctx.set_option("out_sizing", 0)
