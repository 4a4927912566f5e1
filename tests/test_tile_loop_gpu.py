"""The staged pass's tile loop outside its staging loop (csrc/fused_kernel.hpp; -m gpu): what a tile publishes and where its codes are read.

Publish: every wave takes its output offset from the wave totals of the waves in front of it (one LDS word per lane, a DPP sum over a
row of 16 lanes) -- so a table whose wave ranges ALL hold different survivor counts, with 0, 1, exactly the slot's capacity and one more
(a dense wave: the redo list) among them and waves 0 and 15 among the empty and the dense ones, comes out in order only when every prefix
is right.  One workgroup walks all tiles.  The same table goes through the pass over packed codes at 48 and 12 rows per lane, the plain
lean pass, a generic two-column nullable query and the chunked call, whose per-batch counts are the wave totals themselves.

Code addresses: a tile's codes lie at view_byte0 + tile * tile_bytes + wave * wave_bytes (csrc/tile_addr.hpp) -- slices that start on
later super-groups (packed), at even elements (2-byte codes) and of a 4-byte-code column, of lengths around a wave range and a tile.
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
PRED = Predicate([Term(0, ">", 899)])


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
def two_byte():
    """Builds 2- or 4-byte codes at the first whole scan, never the packed layout."""
    c = capi.Context(0)
    c.set_option("narrow_codes", 1)
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


def assert_ran(ctx, r, codes, what=""):
    got = ran(ctx)
    assert (r is None or got[0] == r) and got[1] == WAVES and got[2] & CODES == codes, (what, ctx.last_kernel(), r, codes)


def check(ctx, oracle, dcol, hcol, pred, what):
    outs, rows, _ = ctx.filter_project([dcol], pred, [0])
    want = oracle.filter_project([hcol], pred, [0])
    assert rows == want[0].length, f"{what}: {rows} rows, oracle {want[0].length}; {ctx.last_kernel()}"
    diff = outs[0].download().same_as(want[0])
    assert diff is None, f"{what}: {diff} ({ctx.last_kernel()})"
    return rows


def with_companion(ctx, oracle, values, nbytes):
    """The column uploaded and scanned whole once, which builds its companion of `nbytes` bytes (that scan reads the 8-byte values)."""
    h = Column.from_numpy(values)
    d = ctx.upload(h)
    builds, before = ctx.get_option("narrow_builds"), ctx.get_option("narrow_bytes")
    assert check(ctx, oracle, d, h, Predicate([Term(0, "<", int(values.min()))]), "the first scan") == 0
    assert ctx.get_option("narrow_builds") == builds + 1 and ctx.get_option("narrow_bytes") == before + nbytes
    return d, h


def packed_bytes(n):
    return (n + 383) // 384 * 512


# ---- publish ----------------------------------------------------------------------------------------------------------------------
def publish_table(r):
    """3 tiles + 77 rows at r rows per lane.  Survivors (values above 899) per wave range: all different, except that 0 stands in
    tile 0's wave 0 and tile 1's wave 15; CAP + 1 and CAP + 2 (dense) in tile 1's wave 0 and tile 0's wave 15; 1, CAP - 1, CAP and the
    counts around a 64-row flush step are among the rest; the ragged tile's 77 rows hold 10."""
    rows_per_wave, tile = 64 * r, WAVES * 64 * r
    n = 3 * tile + 77
    pool = [1, CAP, CAP - 1, 63, 64, 65, 2] + [k for k in range(3, 3 * CAP) if k % 5 == 4 and k not in (64, 129, 130)]
    counts = np.array(pool[:3 * WAVES]).reshape(3, WAVES)
    counts[0, 0], counts[1, 15], counts[1, 0], counts[0, 15] = 0, 0, CAP + 1, CAP + 2
    assert counts.max() < rows_per_wave and len(set(counts.ravel()) - {0}) == 3 * WAVES - 2 and 10 not in counts
    rng = np.random.default_rng(r)
    v = rng.integers(0, 900, n, dtype=np.int64)
    for t in range(3):
        for w in range(WAVES):
            at = t * tile + w * rows_per_wave + rng.choice(rows_per_wave, counts[t, w], replace=False)
            v[at] = 900 + rng.integers(0, 100, counts[t, w])
    v[3 * tile + rng.choice(77, 10, replace=False)] = 950
    got = [int((v[i:i + rows_per_wave] > 899).sum()) for i in range(0, n, rows_per_wave)]
    assert got == list(counts.ravel()) + [10]
    return v


@pytest.mark.parametrize("forced,r", [(48 | WAVES << 8, 48), (12, 12)], ids=["48 rows per lane", "12 rows per lane"])
def test_publish_packed(packing, oracle, forced, r):
    v = publish_table(r)
    d, h = with_companion(packing, oracle, v, packed_bytes(len(v)))
    with option(packing, grid_limit=1, cap_rows=64, rows_per_lane=forced):
        check(packing, oracle, d, h, PRED, f"publish at {r} rows per lane")
        assert_ran(packing, r, PACKED)
        assert packing.get_option("last_redo_ppm") > 0  # the two dense ranges
        check(packing, oracle, d, h, Predicate([Term(0, "<", 900)]), "the complement: every range dense")
        assert_ran(packing, r, PACKED)


@pytest.mark.parametrize("r", [48, 12])
def test_publish_plain_lean(plain, oracle, r):
    """The same tables through the pass over the 8-byte values at 16 rows per lane: other wave ranges, the same rows in the same order."""
    v = publish_table(r)
    h = Column.from_numpy(v)
    d = plain.upload(h)
    with option(plain, grid_limit=1, cap_rows=64, rows_per_lane=16 | WAVES << 8):
        check(plain, oracle, d, h, PRED, "plain lean pass")
        assert_ran(plain, 16, 0)
        assert plain.get_option("narrow_builds") == 0


def test_publish_generic_two_columns(plain, oracle):
    """Publish is shared by every instantiation: the table beside a nullable Float64 column, itself nullable, both projected."""
    v = publish_table(12)
    n = len(v)
    rng = np.random.default_rng(5)
    hf = Column.from_numpy(rng.random(n), rng.random(n) < 0.9)
    hx = Column.from_numpy(v, rng.random(n) < 0.8)
    f, x = plain.upload(hf), plain.upload(hx)
    pred = Predicate([Term(0, ">", 0.5), Term(1, ">", 899)])
    with option(plain, grid_limit=1):
        outs, rows, _ = plain.filter_project([f, x], pred, [0, 1])
    want = oracle.filter_project([hf, hx], pred, [0, 1])
    assert rows == want[0].length and rows > 0
    for o, e in zip(outs, want):
        assert o.download().same_as(e) is None, plain.last_kernel()
    assert ran(plain)[2] & CODES == 0 and plain.last_kernel().startswith("fused_filter_compact<2,")


@pytest.mark.parametrize("forced,r", [(0, 16), (8 | WAVES << 8, 8)], ids=["a batch is a wave range", "a batch is two wave ranges"])
def test_publish_batch_counts(plain, oracle, forced, r):
    """1024-row batches: at 16 rows per lane the pass writes a tile's wave totals straight into the caller's per-batch array, at 8 it
    leaves them as wave counts that are summed by twos -- both are the totals publish reads, compared batch by batch."""
    v = publish_table(12)
    n = len(v)
    h = Column.from_numpy(v)
    d = plain.upload(h)
    want_counts = np.add.reduceat((v > 899).astype(np.uint64), np.arange(0, n, 1024))
    in_pass = plain.get_option("batch_counts_in_pass")
    with option(plain, grid_limit=1, rows_per_lane=forced):
        outs, counts, _, total = plain.filter_project_chunked([d], 1024, PRED, [0])
        assert_ran(plain, r, 0)
    assert plain.get_option("batch_counts_in_pass") == in_pass + 1
    assert np.array_equal(np.array(counts, dtype=np.uint64), want_counts) and total == int(want_counts.sum())
    assert outs[0].download().same_as(oracle.filter_project([h], PRED, [0])[0]) is None


# ---- code addresses -----------------------------------------------------------------------------------------------------------------
def lengths(r, have):
    rows_per_wave, tile = 64 * r, WAVES * 64 * r
    return [x for x in (17, rows_per_wave - 1, rows_per_wave, rows_per_wave + 1, tile - 1, tile, tile + 1) if x <= have]


def sliced(ctx, oracle, d, h, off, length, r, codes):
    for pred in (PRED, Predicate([Term(0, "==", 0)])):  # (`x == 0` keeps code 0: what padding and bytes past the companion read as)
        check(ctx, oracle, d.slice(off, length), h.slice(off, length), pred, f"slice {off}+{length}")
        assert_ran(ctx, r, codes, f"slice {off}+{length}")


def column(r, seed):
    """2 tiles + 385 rows at r rows per lane, a tenth of them above 899; the last row survives `x > 899`, the one before it does not."""
    n = 2 * WAVES * 64 * r + 385
    v = np.random.default_rng(seed).integers(0, 1000, n, dtype=np.int64)
    v[n - 1], v[n - 2] = 950, 0
    return v


@pytest.mark.parametrize("off", [384, 768, 384 * 129])
def test_packed_slices(packing, oracle, off):
    v = column(48, seed=off)
    d, h = with_companion(packing, oracle, v, packed_bytes(len(v)))
    for length in lengths(48, len(v) - off) + [len(v) - off]:
        sliced(packing, oracle, d, h, off, length, 48, PACKED)


@pytest.mark.parametrize("off", [2, 130])
def test_two_byte_slices(two_byte, oracle, off):
    v = column(32, seed=off)
    d, h = with_companion(two_byte, oracle, v, 2 * len(v))
    for length in lengths(32, len(v) - off) + [len(v) - off]:
        sliced(two_byte, oracle, d, h, off, length, 32, NARROW16)


def test_four_byte_slices(two_byte, oracle):
    v = column(16, seed=4)
    v[5] = 100000  # the range needs more than 16 bits
    d, h = with_companion(two_byte, oracle, v, 4 * len(v))
    for off in (0, 2, 130):
        for length in lengths(16, len(v) - off) + [len(v) - off]:
            sliced(two_byte, oracle, d, h, off, length, None, NARROW32)  # (whichever geometry the 4-byte class takes)
