"""GPU suite: the device string dictionary (rv_string_dict_build / _encode / _info / _free) against a Python dict of first
occurrences, and the join property -- the Int64 join over the ids yields the reference's pairs for the String keys
(tests/join_model.py with RV_STRING).  Everything is compared exactly."""
import numpy as np
import pytest

from join_model import inner_join_pairs
from rivulus_amd.capi import RV_INT64, RV_STRING, Column, RvError

pytestmark = pytest.mark.gpu

RV_ERR_INVALID_ARG, RV_ERR_TYPE_MISMATCH = 1, 3

LONG = "L" * (100 * 1024 - 1) + "x"  # one 100 KiB cell
SPECIAL = [
    "", "a", "a\0", "\0", "\0\0", "abcdefg", "abcdefgh", "abcdefghi", "fifteen-bytes-xx", "sixteen-bytes-xxx", "seventeen-bytes-xx",
    "x" * 15, "x" * 16, "x" * 17, "y" * 31, "y" * 33,
    "naïve", "日本語のキー", "🙂", "🙂🙂",          # multi-byte UTF-8
    "prefix08A", "prefix08B", "prefix08",           # share 8 bytes: differ in the last byte / only in length
    "prefix-of-16-byt" + "A", "prefix-of-16-byt" + "B", "prefix-of-16-byt",  # share 16 bytes
    "nul\0inside", "nul\0insidf", "nul", "nul\0",
    LONG, LONG[:-1] + "y", LONG[:-1],
]


def first_rows(cells):
    first = {}
    for i, x in enumerate(cells):
        if x is not None:
            first.setdefault(x, i)
    return first


def model_ids(first, cells):
    return [None if x is None else first.get(x, -1) for x in cells]


def ids_of(dev):
    """(cells of an ids column, the downloaded Column); checks what every ids column promises about itself."""
    info = dev.info()
    assert info.dtype == RV_INT64 and info.offset == 0
    col = dev.download()
    vals, valid = col.logical_values(), col.logical_valid()
    cells = [None if valid is not None and not valid[i] else int(vals[i]) for i in range(col.length)]
    nulls = sum(c is None for c in cells)
    assert info.null_count == nulls, "null_count is known"
    assert dev.null_count() == nulls
    assert (col.validity is not None) == (nulls > 0), "the validity is absent without nulls"
    return cells, col


def check_dict(ctx, build_cells, probe_cells=None, build_dev=None, probe_dev=None):
    """Build over build_cells (uploaded, or `build_dev`), compare ids, info and the encode of probe_cells with the model."""
    dev = build_dev if build_dev is not None else ctx.upload(Column.from_strings(build_cells))
    d, ids = ctx.string_dict_build(dev)
    first = first_rows(build_cells)
    got, _ = ids_of(ids)
    assert got == model_ids(first, build_cells)
    again, _ = ids_of(d.encode(dev))
    assert again == got, "out_ids of the build == encode(dict, col)"
    rows, distinct, slots = d.info()
    nonnull = sum(x is not None for x in build_cells)
    assert rows == len(build_cells) and distinct == len(first)
    assert slots >= 2 * nonnull and slots & (slots - 1) == 0 and slots >= 1
    if probe_cells is not None:
        pdev = probe_dev if probe_dev is not None else ctx.upload(Column.from_strings(probe_cells))
        enc, _ = ids_of(d.encode(pdev))
        assert enc == model_ids(first, probe_cells)
    return d, got


def random_cells(rng, n, distinct, null_share):
    pool = [f"key-{k:05d}-" + "z" * (k % 23) for k in range(max(1, distinct))]
    picks = rng.integers(0, len(pool), n)
    nulls = rng.random(n) < null_share
    return [None if z else pool[k] for k, z in zip(picks, nulls)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 10_000])
def test_row_counts(gpu_ctx, n):
    rng = np.random.default_rng(n)
    build = random_cells(rng, n, max(1, n // 3), 0.2)
    probe = random_cells(rng, n + 5, max(2, n // 2), 0.2) + ["absent", None, ""]
    check_dict(gpu_ctx, build, probe)


def test_cell_shapes(gpu_ctx):
    """Every length around the 8-byte groups, "" next to nulls, embedded NUL, multi-byte UTF-8, shared prefixes, one 100 KiB cell."""
    rng = np.random.default_rng(7)
    build = SPECIAL[:-3] + [None, "", None] + SPECIAL[:-3][::-1] + [LONG, LONG]
    probe = SPECIAL + [None, "", "absent", "a\0\0", "abcdefgh\0", "prefix08C", "prefix-of-16-byt" + "C", "🙂🙂🙂"]
    order = rng.permutation(len(probe))
    check_dict(gpu_ctx, build, [probe[i] for i in order])


@pytest.mark.parametrize("shape", ["nulls20", "all_nulls", "no_nulls", "one_key", "all_distinct"])
def test_shapes(gpu_ctx, shape):
    rng = np.random.default_rng(11)
    n = 10_000
    if shape == "nulls20":
        build = random_cells(rng, n, 500, 0.2)
    elif shape == "all_nulls":
        build = [None] * n
    elif shape == "no_nulls":
        build = random_cells(rng, n, 500, 0.0)
    elif shape == "one_key":
        build = ["the one key"] * n
    else:
        build = [f"distinct-{i}" for i in rng.permutation(n)]
    probe = random_cells(rng, 1000, 700, 0.1) + build[:50] + ["absent"]
    _, ids = check_dict(gpu_ctx, build, probe)
    if shape == "one_key":
        assert ids == [0] * n
    if shape == "all_distinct":
        assert ids == list(range(n))


@pytest.mark.parametrize("offset,length", [(3, 61), (67, 125), (67, 1003)])
def test_slices(gpu_ctx, offset, length):
    """Offsets 3 and 67, lengths that are no multiple of 8: validity and string offsets are re-based, ids count from the slice."""
    rng = np.random.default_rng(offset + length)
    whole = random_cells(rng, offset + length + 9, 40, 0.25)
    dev = gpu_ctx.upload(Column.from_strings(whole)).slice(offset, length)
    pwhole = random_cells(rng, offset + length + 9, 60, 0.25)
    pdev = gpu_ctx.upload(Column.from_strings(pwhole)).slice(offset, length)
    check_dict(gpu_ctx, whole[offset:offset + length], pwhole[offset:offset + length], build_dev=dev, probe_dev=pdev)
    # a slice without a null inside a column with nulls: no validity on the ids
    cells = [None] * 3 + [f"k{i % 5}" for i in range(61)] + [None] * 4
    sdev = gpu_ctx.upload(Column.from_strings(cells)).slice(3, 61)
    check_dict(gpu_ctx, cells[3:64], build_dev=sdev)


@pytest.mark.parametrize("bits", [1, 2, 4])
def test_collision_chains(gpu_ctx, bits):
    """Option string_hash_bits: 2^bits chain starts for 200 distinct keys -- chains of hundreds, every hit confirmed by the bytes."""
    rng = np.random.default_rng(bits)
    build = random_cells(rng, 2000, 200, 0.1) + SPECIAL[:-3]
    probe = random_cells(rng, 1500, 260, 0.1) + SPECIAL[:-3] + ["absent"]
    _, plain = check_dict(gpu_ctx, build, probe)
    try:
        gpu_ctx.set_option("string_hash_bits", bits)
        assert gpu_ctx.get_option("string_hash_bits") == bits
        _, chained = check_dict(gpu_ctx, build, probe)
    finally:
        gpu_ctx.set_option("string_hash_bits", 0)
    assert chained == plain


def test_run_to_run_identity(gpu_ctx):
    rng = np.random.default_rng(3)
    build = random_cells(rng, 10_000, 300, 0.2)
    probe = random_cells(rng, 10_000, 400, 0.2)
    bdev, pdev = gpu_ctx.upload(Column.from_strings(build)), gpu_ctx.upload(Column.from_strings(probe))
    runs = []
    for _ in range(2):
        d, ids = gpu_ctx.string_dict_build(bdev)
        a, b = ids.download(), d.encode(pdev).download()
        runs.append((a.values.tobytes(), a.validity.tobytes(), b.values.tobytes(), b.validity.tobytes(), d.info()))
    assert runs[0] == runs[1]


def test_dictionary_keeps_the_source_alive(gpu_ctx):
    rng = np.random.default_rng(5)
    build = random_cells(rng, 3000, 100, 0.2)
    probe = random_cells(rng, 3000, 150, 0.2)
    bdev = gpu_ctx.upload(Column.from_strings(build))
    d, _ = gpu_ctx.string_dict_build(bdev, want_ids=False)
    bdev.free()
    filler = gpu_ctx.upload(Column.from_strings(["overwrite me"] * 3000))  # would reuse the freed blocks, had they gone back to the pool
    got, _ = ids_of(d.encode(gpu_ctx.upload(Column.from_strings(probe))))
    assert got == model_ids(first_rows(build), probe)
    filler.free()


def pairs_through_ids(ctx, build, probe):
    d, ids_b = ctx.string_dict_build(ctx.upload(Column.from_strings(build)))
    ids_p = d.encode(ctx.upload(Column.from_strings(probe)))
    pi, bi, rows = ctx.join_build(ids_b).probe(ids_p)
    a = pi.download().logical_values() if rows else np.zeros(0, np.int64)
    b = bi.download().logical_values() if rows else np.zeros(0, np.int64)
    return list(zip(a.tolist(), b.tolist()))


@pytest.mark.parametrize("n", [70, 5000])
def test_join_property(gpu_ctx, n):
    """join_build(ids_B) + probe(ids_P) == the reference's result_pairs for the String keys: duplicate build keys, null to null, misses."""
    rng = np.random.default_rng(n)
    build = random_cells(rng, n, max(2, n // 7), 0.1)
    probe = random_cells(rng, n + 3, max(3, n // 4), 0.1) + [None, "absent", build[0]]
    want = inner_join_pairs(RV_STRING, build, RV_STRING, probe)
    assert any(probe[p] is None for p, _ in want) and len(want) > n  # null-to-null pairs and duplicate build keys are in
    assert len({p for p, _ in want}) < len(probe)                     # ... and misses
    assert pairs_through_ids(gpu_ctx, build, probe) == want


def test_errors(gpu_ctx):
    ints = gpu_ctx.upload(Column.from_numpy(np.arange(10, dtype=np.int64)))
    with pytest.raises(RvError) as e:
        gpu_ctx.string_dict_build(ints)
    assert e.value.status == RV_ERR_TYPE_MISMATCH
    d, _ = check_dict(gpu_ctx, ["a", "b", None, "a"], ["b", "c", None])  # the context still works
    with pytest.raises(RvError) as e:
        d.encode(ints)
    assert e.value.status == RV_ERR_TYPE_MISMATCH
    from rivulus_amd import capi
    out = capi.C.c_void_p()
    assert capi.load().rv_string_dict_build(gpu_ctx.handle, None, capi.C.byref(out), None) == RV_ERR_INVALID_ARG
    assert capi.load().rv_string_dict_encode(gpu_ctx.handle, d.handle, None, capi.C.byref(out)) == RV_ERR_INVALID_ARG
    assert capi.load().rv_string_dict_info(None, None, None, None) == RV_ERR_INVALID_ARG
    check_dict(gpu_ctx, ["still", "works", "still"])


def test_null_column(gpu_ctx):
    """An RV_NULL column: all-null ids and an empty dictionary; a String column against that dictionary: every valid cell absent."""
    nulls = gpu_ctx.upload(Column.nulls(70))
    d, ids = gpu_ctx.string_dict_build(nulls)
    got, _ = ids_of(ids)
    assert got == [None] * 70
    rows, distinct, slots = d.info()
    assert (rows, distinct) == (70, 0) and slots & (slots - 1) == 0
    enc, _ = ids_of(d.encode(gpu_ctx.upload(Column.from_strings(["a", None, ""]))))
    assert enc == [-1, None, -1]
    d2, _ = gpu_ctx.string_dict_build(gpu_ctx.upload(Column.from_strings(["a", "b"])))
    enc2, _ = ids_of(d2.encode(nulls))
    assert enc2 == [None] * 70
    d0, ids0 = gpu_ctx.string_dict_build(gpu_ctx.upload(Column.nulls(0)))
    assert ids_of(ids0)[0] == [] and d0.info()[:2] == (0, 0)
