"""Narrow companions of resident Int64 columns (csrc/narrow.hip, narrow_rule.hpp; FF_NARROW16 / FF_NARROW32 of the lean filter pass)
against the oracle (-m gpu): value ranges on either side of every code width, range positions at the ends of Int64, ragged and
multi-tile row counts, every compare operator and literal kind, slices at aligned and unaligned offsets, the redo kernel and an
overflow re-run behind a pass over codes, per-batch counts of a chunked window, lifetime (pool reuse, wrapped and nullable columns,
the option's off switch) and both sides of the two constants that decide when a companion is built."""
import numpy as np
import pytest

from helpers import const
from rivulus_amd import capi
from rivulus_amd.capi import RV_INT64, Column, Predicate, Term, synth_spec

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NARROW16, NARROW32 = 4096, 8192  # FF_NARROW16 / FF_NARROW32 (csrc/scan_frontend.hpp)
OPS = ("==", "!=", "<", ">", "<=", ">=")
ROW_COUNTS = (1, 63, 64, 1023, 1024, 2 * 16384 + 5)  # ragged last tile; more than one 16384-row tile


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own, packing at the first whole scan whatever the size (option narrow_codes = 1)."""
    c = capi.Context(0)
    c.set_option("narrow_codes", 1)
    yield c
    c.close()


def flags(ctx):
    name = ctx.last_kernel()
    assert name.startswith("fused_filter_compact<"), name
    return int(name.rstrip(">").split(",")[-1])


def column(lo, hi, n, seed=7):
    """n Int64 values in [lo, hi], both ends present (n >= 2), the rest spread over the range; Python integers throughout."""
    rng = np.random.default_rng(seed)
    span = hi - lo
    vals = [lo + int(u * span) for u in rng.random(n)]
    vals = [min(max(v, lo), hi) for v in vals]
    if n >= 2:
        vals[n // 3], vals[(2 * n) // 3] = hi, lo
    return np.array(vals, dtype=np.int64)


def check(ctx, oracle, dcol, hcol, pred, what):
    outs, rows, _ = ctx.filter_project([dcol], pred, [0])
    want = oracle.filter_project([hcol], pred, [0])
    diff = outs[0].download().same_as(want[0])
    assert diff is None and rows == want[0].length, f"{what}: {diff} ({rows} rows, oracle {want[0].length}; {ctx.last_kernel()})"
    return rows


def packed(ctx, oracle, values, width):
    """The column uploaded and scanned once; width: the code bytes its companion must have (0: refused)."""
    h = Column.from_numpy(values)
    d = ctx.upload(h)
    builds, nbytes = ctx.get_option("narrow_builds"), ctx.get_option("narrow_bytes")
    check(ctx, oracle, d, h, Predicate([Term(0, ">", int(values[0]))]), "the first scan")
    assert flags(ctx) & (NARROW16 | NARROW32) == 0  # the triggering pass itself reads the 8-byte values
    assert ctx.get_option("narrow_builds") == builds + (1 if width else 0)
    assert ctx.get_option("narrow_bytes") == nbytes + width * len(values)
    return d, h


RANGES = [  # (name, min, max, code bytes; 0: refused)
    ("range 0", 41, 41, 2),
    ("range 65535", -5, 65530, 2),
    ("range 65536", -5, 65531, 4),
    ("range 2^32 - 1", 1000, 1000 + (1 << 32) - 1, 4),
    ("range 2^32", 1000, 1000 + (1 << 32), 0),
    ("base INT64_MIN, range 65535", I64_MIN, I64_MIN + 65535, 2),
    ("max INT64_MAX, 2-byte", I64_MAX - 65535, I64_MAX, 2),
    ("max INT64_MAX, 4-byte", I64_MAX - (1 << 32) + 1, I64_MAX, 4),
    ("both extremes", I64_MIN, I64_MAX, 0),
]


@pytest.mark.parametrize("name,lo,hi,width", RANGES, ids=[r[0] for r in RANGES])
def test_every_operator_and_literal_over_every_range(ctx, oracle, name, lo, hi, width):
    n = 1023
    d, h = packed(ctx, oracle, column(lo, hi, n), width)
    mid = lo + (hi - lo) // 2
    literals = sorted({lo, hi, mid, I64_MIN, I64_MAX} | ({lo - 1} if lo > I64_MIN else set()) | ({hi + 1} if hi < I64_MAX else set()))
    passes = ctx.get_option("narrow_passes")
    ran = 0
    for nulls in ("drops", "least"):
        for op in OPS:
            for lit in literals:
                check(ctx, oracle, d, h, Predicate([Term(0, op, lit)], nulls), f"{name}: x {op} {lit} ({nulls})")
                want = (NARROW16 if width == 2 else NARROW32) if width else 0
                assert flags(ctx) & (NARROW16 | NARROW32) == want, (name, op, lit, ctx.last_kernel())
                ran += 1
            # null literal and cross-type literal: constant terms, not the lean form -- the 8-byte values, the same result
            for lit in (None, 0.5, float(mid)):
                check(ctx, oracle, d, h, Predicate([Term(0, op, lit)], nulls), f"{name}: x {op} {lit!r} ({nulls})")
    assert ctx.get_option("narrow_passes") == passes + (ran if width else 0)


@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("lo,hi,width", [(100, 1099, 2), (-70000, 70000, 4)])
def test_row_counts(ctx, oracle, n, lo, hi, width):
    v = column(lo, hi, n, seed=n)
    if n < 2:  # one row holds one end of the range at most: its own range is 0
        width = 2
    assert width == (2 if int(v.max()) - int(v.min()) <= 65535 else 4)
    d, h = packed(ctx, oracle, v, width)
    mid = lo + (hi - lo) // 2
    for op, lit in ((">", mid), ("<=", lo), ("!=", hi), (">=", lo), ("<", lo), ("==", int(v[0]))):
        check(ctx, oracle, d, h, Predicate([Term(0, op, lit)]), f"{n} rows: x {op} {lit}")
        assert flags(ctx) & (NARROW16 if width == 2 else NARROW32)


@pytest.mark.parametrize("width,hi", [(2, 999), (4, 99999)])
def test_slices_of_a_packed_buffer(ctx, oracle, width, hi):
    n = 2 * 16384 + 5
    d, h = packed(ctx, oracle, column(0, hi, n, seed=3), width)
    for off in (0, 2, 3, 1026):
        for length in (n - off, 1024, 17):
            sd, sh = d.slice(off, length), h.slice(off, length)
            check(ctx, oracle, sd, sh, Predicate([Term(0, ">", hi - hi // 10)]), f"slice {off}+{length}")  # (sparse: the staged pass)
            # an odd element offset is not aligned for the pair loads: the plain kernel, the same result
            assert bool(flags(ctx) & (NARROW16 | NARROW32)) == (off % 2 == 0), (off, length, ctx.last_kernel())


def test_redo_kernel_and_overflow_rerun_behind_a_narrow_pass(ctx, oracle):
    """A clustered column: whole wave ranges survive, more than their LDS slots hold -- the redo kernel re-reads them (from the 8-byte
    values) behind a pass over codes.  Then outputs sized far too small: the pass counts exactly and is re-run once."""
    n = 2 * 16384 + 5
    v = np.zeros(n, dtype=np.int64)
    v[1024:3072] = 900 + (np.arange(2048) % 50)
    v[20000:21024] = 950
    v[::97] = 901
    d, h = packed(ctx, oracle, v, 2)
    pred = Predicate([Term(0, ">", 899)])
    for _ in range(2):
        check(ctx, oracle, d, h, pred, "clustered")
        assert flags(ctx) & NARROW16 and ctx.get_option("last_redo_ppm") > 0, ctx.last_kernel()
    reruns = ctx.get_option("overflow_reruns")
    ctx.set_option("out_sizing", 2)  # two rows per million + 1024: far below the ~3400 survivors
    try:
        check(ctx, oracle, d, h, pred, "overflow re-run")
        assert flags(ctx) & NARROW16 and ctx.get_option("overflow_reruns") == reruns + 1
    finally:
        ctx.set_option("out_sizing", 0)


def test_chunked_window_counts_match_the_plain_path(ctx, oracle):
    n = 2 * 16384 + 5
    v = column(0, 999, n, seed=11)
    h = Column.from_numpy(v)
    pred = Predicate([Term(0, ">", 899)])
    want_counts = np.add.reduceat((v > 899).astype(np.uint64), np.arange(0, n, 1024))
    plain = capi.Context(0)
    try:
        plain.set_option("narrow_codes", -1)
        pd = plain.upload(h)
        for _ in range(2):
            p_outs, p_counts, _, p_total = plain.filter_project_chunked([pd], 1024, pred, [0])
        assert plain.get_option("narrow_builds") == 0 and plain.last_kernel().endswith(",32>")
        p_counts = np.array(p_counts, dtype=np.uint64)
        p_values = p_outs[0].download()
    finally:
        plain.close()
    d, _ = packed(ctx, oracle, v, 2)
    in_pass = ctx.get_option("batch_counts_in_pass")
    outs, counts, _, total = ctx.filter_project_chunked([d], 1024, pred, [0])
    assert flags(ctx) & NARROW16 and ctx.get_option("batch_counts_in_pass") == in_pass + 1
    assert np.array_equal(np.array(counts, dtype=np.uint64), p_counts) and np.array_equal(p_counts, want_counts) and total == p_total
    assert outs[0].download().same_as(p_values) is None
    assert outs[0].download().same_as(oracle.filter_project([h], pred, [0])[0]) is None


def test_a_reused_pool_block_starts_without_codes(ctx, oracle):
    n = 40000
    a = column(0, 999, n, seed=1)
    d, h = packed(ctx, oracle, a, 2)
    ptr = d.device_ptrs().values
    check(ctx, oracle, d, h, Predicate([Term(0, ">", 500)]), "packed")
    assert flags(ctx) & NARROW16
    d.free()
    b = column(5000, 5999, n, seed=2)  # other values: codes inherited with the block would give other survivors
    hb = Column.from_numpy(b)
    held = []  # (freed outputs of the same size may be handed out first)
    for _ in range(8):
        held.append(ctx.upload(hb))
        if held[-1].device_ptrs().values == ptr:
            break
    db = held[-1]
    assert db.device_ptrs().values == ptr, "the pool did not hand the freed block out again"
    builds = ctx.get_option("narrow_builds")
    check(ctx, oracle, db, hb, Predicate([Term(0, ">", 5500)]), "the block's next column")
    assert flags(ctx) & (NARROW16 | NARROW32) == 0 and ctx.get_option("narrow_builds") == builds + 1
    check(ctx, oracle, db, hb, Predicate([Term(0, ">", 5500)]), "the block's next column, packed")
    assert flags(ctx) & NARROW16


def test_wrapped_and_nullable_columns_never_get_codes(ctx, oracle):
    n = 5000
    v = column(0, 999, n, seed=5)
    h = Column.from_numpy(v)
    owner = ctx.upload(h)
    wrapped = ctx.wrap(owner.device_ptrs())  # caller-owned memory: the caller may write to it
    valid = np.random.default_rng(6).random(n) > 0.1
    hn = Column.from_numpy(v, valid)
    nullable = ctx.upload(hn)
    builds = ctx.get_option("narrow_builds")
    for _ in range(3):
        check(ctx, oracle, wrapped, h, Predicate([Term(0, ">", 500)]), "wrapped")
        assert flags(ctx) & (NARROW16 | NARROW32) == 0
        check(ctx, oracle, nullable, hn, Predicate([Term(0, ">", 500)]), "nullable")
        assert flags(ctx) & (NARROW16 | NARROW32) == 0
    assert ctx.get_option("narrow_builds") == builds


def test_option_off_gives_the_plain_kernels(oracle):
    n = 2 * 16384 + 5
    v = column(0, 999, n, seed=9)
    h = Column.from_numpy(v)
    off = capi.Context(0)
    try:
        off.set_option("narrow_codes", -1)
        d = off.upload(h)
        for _ in range(4):
            check(off, oracle, d, h, Predicate([Term(0, ">", 899)]), "narrow_codes = -1")
            assert off.last_kernel() == "fused_filter_compact<1,16,2,16,32>"
        assert off.get_option("narrow_builds") == 0 and off.get_option("narrow_passes") == 0 and off.get_option("narrow_bytes") == 0
    finally:
        off.close()


@pytest.mark.parametrize("rows,builds_after", [
    (const("kNarrowFromRows") - 64, None),  # one tile short of the floor: never
    (const("kNarrowFromRows"), const("kNarrowAfterWholeScans")),
], ids=["below kNarrowFromRows", "at kNarrowFromRows"])
def test_both_sides_of_the_trigger(rows, builds_after):
    """Option narrow_codes = 0 (auto): a companion is built behind whole scan number kNarrowAfterWholeScans of a buffer of
    kNarrowFromRows elements and more -- not one scan earlier, not one tile below."""
    auto = capi.Context(0)
    try:
        x = auto.generate(synth_spec(RV_INT64, seed=42, length=rows))
        pred = Predicate([Term(0, ">", 899)])
        want = None
        for scan in range(1, const("kNarrowAfterWholeScans") + 3):
            outs, got, _ = auto.filter_project([x], pred, [0])
            want = got if want is None else want
            assert got == want and got == outs[0].length
            built = builds_after is not None and scan >= builds_after
            assert auto.get_option("narrow_builds") == (1 if built else 0), (rows, scan)
            narrow = builds_after is not None and scan > builds_after  # the triggering pass itself read the 8-byte values
            assert bool(flags(auto) & NARROW16) == narrow, (rows, scan, auto.last_kernel())
            if scan == 1:
                first = outs[0].download()
            else:
                assert outs[0].download().same_as(first) is None
        # half the buffer, read again and again, is no whole scan
        y = auto.generate(synth_spec(RV_INT64, seed=43, length=const("kNarrowFromRows")))
        half = y.slice(0, const("kNarrowFromRows") // 2)
        builds = auto.get_option("narrow_builds")
        for _ in range(2 * const("kNarrowAfterWholeScans") + 1):
            auto.filter_project([half], pred, [0])
        assert auto.get_option("narrow_builds") == builds
    finally:
        auto.close()
