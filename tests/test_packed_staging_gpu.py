"""The whole-tile staging and the write-out of the passes over PACKED codes (csrc/fused_kernel.hpp, kPack10; -m gpu), under option
narrow_codes = 2 with the packed geometries forced to 48, 24 and 12 rows per lane, row for row against the oracle and against a context
that never builds codes (narrow_codes = -1):

  predicate classes   a whole tile runs one of three forms, chosen by which ends of the code interval a code can fall outside of
                      (csrc/narrow_sides.hpp): every operator with the literal below, at, inside, at and above the column's range
                      reaches the lower-only, the upper-only and the two-sided form, the full and the empty set among them;
  row counts          exactly one tile; four tiles + 385 rows (three stages rotate, the last tile is ragged); the same walked by one
                      workgroup;
  clamp, spare cell   ONE clamp per pair: a wave range with exactly `cap` survivors whose last is an odd row behind a surviving even
                      row of the same lane (the last cell of the slot), and one with cap + 1 of that shape (dense: the odd row lands in
                      the slot's spare cell) -- the waves and stages behind them must come out intact, the redo list as the plain
                      pass's rule gives it;
  write-out           whole lines: the second wave's run starts at every offset 0..16 inside a line, a run of fewer than 16 survivors
                      lies inside one line, and the output's capacity ends inside the last run's last line.
Every case reads the geometry and the flags of the kernel that ran from last_kernel(): a fallback to another kernel fails."""
import numpy as np
import pytest

from rivulus_amd import capi
from rivulus_amd.capi import Column, Predicate, Term

pytestmark = pytest.mark.gpu

NARROW16, NARROW32, PACK10 = 4096, 8192, 16384  # FF_NARROW16 / FF_NARROW32 / FF_PACK10 (csrc/scan_frontend.hpp)
CODES = NARROW16 | NARROW32 | PACK10
PACKED = NARROW16 | PACK10
WAVES = 16
CAP = 128  # option cap_rows = 64 asks for the smallest slot; a slot holds at least one chunk of 64 * VEC rows, VEC = 2
GEOMETRIES = [48, 24, 12]
OPS = (">", ">=", "<", "<=", "==", "!=")
LO, HI = 100, 1099  # the columns' value range: codes 0 .. 999
PRED = Predicate([Term(0, ">", 999)])  # keeps a tenth of a uniform column


class option:
    def __init__(self, ctx, **values):
        self.ctx, self.values = ctx, values

    def __enter__(self):
        for k, v in self.values.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            self.ctx.set_option(k, 0)


@pytest.fixture(scope="module")
def packing():
    """Packs at the first whole scan whatever the size, packed where the rule allows."""
    c = capi.Context(0)
    c.set_option("narrow_codes", 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain():
    """Never builds codes: every pass reads the 8-byte values."""
    c = capi.Context(0)
    c.set_option("narrow_codes", -1)
    yield c
    c.close()


def ran(ctx):
    """(rows per lane, waves, flags) of the kernel of the last pass."""
    name = ctx.last_kernel()
    assert name.startswith("fused_filter_compact<"), name
    _, r, _, w, f = (int(x) for x in name[name.index("<") + 1:-1].split(","))
    return r, w, f


def assert_packed(ctx, r, what):
    got = ran(ctx)
    assert got[0] == r and got[1] == WAVES and got[2] & CODES == PACKED, (what, ctx.last_kernel(), r)


def packed_bytes(n):
    return (n + 383) // 384 * 512


def upload_both(packing, plain, oracle, values):
    """The column in both contexts; in the packing one scanned whole once, which builds its packed companion (that scan reads the
    8-byte values and keeps nothing)."""
    h = Column.from_numpy(values)
    d, pd = packing.upload(h), plain.upload(h)
    builds, before = packing.get_option("narrow_builds"), packing.get_option("narrow_bytes")
    outs, rows, _ = packing.filter_project([d], Predicate([Term(0, "<", int(values.min()))]), [0])
    assert rows == 0 and ran(packing)[2] & CODES == 0
    assert packing.get_option("narrow_builds") == builds + 1 and packing.get_option("narrow_bytes") == before + packed_bytes(len(values))
    return d, pd, h


def check(packing, plain, oracle, d, pd, h, pred, r, what):
    """The packed pass at r rows per lane against the oracle and against the pass over the 8-byte values; -> the surviving rows."""
    outs, rows, _ = packing.filter_project([d], pred, [0])
    assert_packed(packing, r, what)
    want = oracle.filter_project([h], pred, [0])
    assert rows == want[0].length, f"{what}: {rows} rows, oracle {want[0].length}; {packing.last_kernel()}"
    got = outs[0].download()
    diff = got.same_as(want[0])
    assert diff is None, f"{what}: {diff} ({packing.last_kernel()})"
    p_outs, p_rows, _ = plain.filter_project([pd], pred, [0])
    assert plain.get_option("narrow_builds") == 0
    assert p_rows == rows and got.same_as(p_outs[0].download()) is None, f"{what}: differs from the pass over the 8-byte values"
    return rows


def uniform(n, seed):
    v = np.random.default_rng(seed).integers(LO, HI + 1, n, dtype=np.int64)
    v[1], v[n // 2], v[n - 1], v[n - 2] = LO, HI, HI, LO  # both ends are there; the last row survives `x > 999`, the one before not
    return v


# ---- predicate classes x row counts --------------------------------------------------------------------------------------------------
SHAPES = [("one tile", 1, 0, 0), ("4 tiles + 385 rows", 4, 385, 0), ("4 tiles + 385 rows, one workgroup", 4, 385, 1)]


@pytest.mark.parametrize("r", GEOMETRIES)
@pytest.mark.parametrize("name,tiles,extra,limit", SHAPES, ids=[s[0] for s in SHAPES])
def test_predicate_classes(packing, plain, oracle, name, tiles, extra, limit, r):
    n = tiles * WAVES * 64 * r + extra
    v = uniform(n, seed=r + tiles)
    d, pd, h = upload_both(packing, plain, oracle, v)
    literals = (LO - 1, LO, (LO + HI) // 2, HI, HI + 1)  # below the minimum, at it, inside, at the maximum, above it
    empty = full = 0
    with option(packing, grid_limit=limit, rows_per_lane=r | WAVES << 8):
        for op in OPS:
            for lit in literals:
                rows = check(packing, plain, oracle, d, pd, h, Predicate([Term(0, op, lit)]), r, f"{name} at {r} rows per lane: x {op} {lit}")
                empty += rows == 0
                full += rows == n
    assert empty >= 6 and full >= 6, (name, empty, full)  # x > max, x >= max + 1, x < min, x <= min - 1, x == outside ... and their complements


# ---- one clamp per pair, the spare cell ------------------------------------------------------------------------------------------------
def place(v, first, rows_per_wave, count, rng, last_pair):
    """`count` survivors (values above 999) in the wave range that starts at row `first`.  last_pair: the last two are an even row and
    the odd row behind it -- one lane's two rows of a pair; the others lie in front of them."""
    v[first:first + rows_per_wave] = rng.integers(LO, 1000, rows_per_wave)
    if not last_pair:
        at = rng.choice(rows_per_wave, count, replace=False)
    else:
        even = 2 * int(rng.integers(rows_per_wave // 4, rows_per_wave // 2 - 1))
        at = np.concatenate([rng.choice(even, count - 2, replace=False), [even, even + 1]])
    v[first + at] = 1050


@pytest.mark.parametrize("r", GEOMETRIES)
@pytest.mark.parametrize("mirror", [False, True], ids=["lower-only and two-sided", "upper-only and two-sided"])
def test_one_clamp_and_the_spare_cell(packing, plain, oracle, r, mirror):
    """5 tiles + 385 rows, one workgroup (tile t is staged in stage t % 3 and written out behind the staging of tile t + 2), slots of CAP
    rows.  Exactly CAP survivors ending on an odd row behind its even row: tile 0's wave 15 and tile 2's wave 0.  CAP + 1 of the same
    shape (dense; the odd row is stored one cell past the slot): tile 1's wave 3 -- the spare cell lies in front of wave 4's slot -- and
    tile 3's wave 15, whose spare cell lies in front of the next STAGE's wave 0: stage 1, where tile 1's wave 0 still waits to be written
    out while tile 3 is staged, so a store past the spare cell would change its first survivor.
    Every other wave range holds 1 .. CAP - 1 survivors, so every slot around them is flushed and compared.  The redo list: the two
    dense ranges and no other, and the same count from the plain twin, which re-runs the launch after an output overflow in the same
    slots.  Survivors are the value
    1050 (and one 1099 in the ragged tile), so `x > 999` (lower-only) and `x == 1050` (two-sided) both stage these shapes; mirrored, the
    column's values are LO + HI - v and `x < 200` (upper-only) and `x == 149` do."""
    rows_per_wave, tile = 64 * r, WAVES * 64 * r
    n = 5 * tile + 385
    rng = np.random.default_rng(100 + r)
    v = rng.integers(LO, 1000, n, dtype=np.int64)
    special = {(0, 15): CAP, (2, 0): CAP, (1, 3): CAP + 1, (3, 15): CAP + 1}
    for t in range(5):
        for w in range(WAVES):
            count = special.get((t, w))
            place(v, t * tile + w * rows_per_wave, rows_per_wave, count if count else int(rng.integers(1, CAP)), rng, last_pair=count is not None)
    v[5 * tile + rng.choice(385, 40, replace=False)] = 1050
    v[5 * tile + np.flatnonzero(v[5 * tile:] < 1000)[0]] = HI
    held = [int((v[i:i + rows_per_wave] > 999).sum()) for i in range(0, n, rows_per_wave)]
    assert sorted(k for k in held if k >= CAP) == [CAP, CAP, CAP + 1, CAP + 1] and held[-1] == 41
    for (t, w), count in special.items():  # the shape: the range's last two survivors are rows 2l, 2l + 1
        at = np.flatnonzero(v[t * tile + w * rows_per_wave:t * tile + (w + 1) * rows_per_wave] > 999)
        assert len(at) == count and at[-2] % 2 == 0 and at[-1] == at[-2] + 1
    one_sided, two_sided = PRED, Predicate([Term(0, "==", 1050)])
    if mirror:
        v = LO + HI - v
        one_sided, two_sided = Predicate([Term(0, "<", LO + HI - 999)]), Predicate([Term(0, "==", LO + HI - 1050)])
    d, pd, h = upload_both(packing, plain, oracle, v)
    reruns = packing.get_option("overflow_reruns")
    with option(packing, grid_limit=1, cap_rows=64, rows_per_lane=r | WAVES << 8):
        assert check(packing, plain, oracle, d, pd, h, one_sided, r, f"clamp at {r} rows per lane") == sum(held)
        # the redo list: the ranges with more than CAP survivors and no other -- the plain pass's rule (wave_total > cap)
        nranges = (n + tile - 1) // tile * WAVES
        assert packing.get_option("last_redo_ppm") == int(2 / nranges * 1e6), (packing.get_option("last_redo_ppm"), nranges)
        assert check(packing, plain, oracle, d, pd, h, two_sided, r, "clamp, two-sided form") == sum(held) - 1
        assert packing.get_option("last_redo_ppm") == int(2 / nranges * 1e6)
        assert packing.get_option("overflow_reruns") == reruns
        # the plain twin over the 8-byte values: an output sized for 1024 rows overflows, and the twin re-runs the launch in the same slots
        assert sum(held) > 1024 + n * 2 // 1000000
        with option(packing, out_sizing=2):
            assert check(packing, plain, oracle, d, pd, h, one_sided, r, "clamp, the plain twin's re-run") == sum(held)
        assert packing.get_option("overflow_reruns") == reruns + 1
        assert packing.get_option("last_redo_ppm") == int(2 / nranges * 1e6), "the plain twin lists other ranges"


# ---- write-out in whole lines ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", GEOMETRIES)
def test_runs_start_at_every_offset_inside_a_line(packing, plain, oracle, r):
    """One tile + 77 rows per column, 17 columns: wave 0 holds k = 0 .. 16 survivors, so wave 1's run starts k rows into a line; wave 1
    holds as many as put wave 2's run 3 rows into a line, and wave 2 holds 5: a run inside one line.  The rest is uniform."""
    rows_per_wave, tile = 64 * r, WAVES * 64 * r
    n = tile + 77
    with option(packing, rows_per_lane=r | WAVES << 8):
        for k in range(17):
            rng = np.random.default_rng(1000 * r + k)
            v = uniform(n, seed=r + k)
            second = 70 + (3 - k - 70) % 16  # 70 .. 85 survivors: two store instructions, and (k + second) % 16 == 3
            for w, count in enumerate((k, second, 5)):
                v[w * rows_per_wave:(w + 1) * rows_per_wave] = rng.integers(LO, 1000, rows_per_wave)
                v[w * rows_per_wave + rng.choice(rows_per_wave, count, replace=False)] = 1000 + rng.integers(0, 100, count)
            assert (k + second) % 16 == 3 and int((v[:3 * rows_per_wave] > 999).sum()) == k + second + 5
            d, pd, h = upload_both(packing, plain, oracle, v)
            check(packing, plain, oracle, d, pd, h, PRED, r, f"wave 0 holds {k} at {r} rows per lane")


@pytest.mark.parametrize("r", GEOMETRIES)
@pytest.mark.parametrize("short", [0, 3, 13])
def test_capacity_ends_inside_the_last_line(packing, plain, oracle, r, short):
    """out_sizing = 100 sizes the output for 100 rows per million + 1024, no multiple of a line's 16 rows here.  The column holds exactly
    that many survivors less `short`: the last run's last line is cut by the buffer's end, nothing overflows and nothing is re-run."""
    tile = WAVES * 64 * r
    n = 2 * tile + 385
    capacity = int(n * 100 * 1e-6) + 1024
    assert capacity % 16 != 0
    rng = np.random.default_rng(r + short)
    v = rng.integers(LO, 1000, n, dtype=np.int64)
    v[rng.choice(n, capacity - short, replace=False)] = 1001
    d, pd, h = upload_both(packing, plain, oracle, v)
    reruns = packing.get_option("overflow_reruns")
    with option(packing, out_sizing=100, rows_per_lane=r | WAVES << 8):
        assert check(packing, plain, oracle, d, pd, h, PRED, r, f"capacity {capacity}, {short} short") == capacity - short
    assert packing.get_option("overflow_reruns") == reruns
