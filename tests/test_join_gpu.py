"""GPU suite: the inner hash join (rv_join_build / rv_join_probe / rv_hash_join) against the reference model
(tests/join_model.py, plan.rs:174-284), bit-exact at AnyValue level: the value where a cell is valid, null where not."""
import numpy as np
import pytest

from join_model import comparable, inner_join_pairs, materialize
from rivulus_amd import capi
from rivulus_amd.capi import RV_BOOLEAN, RV_FLOAT64, RV_INT64, RV_NULL, RV_STRING, Column, RvError

pytestmark = pytest.mark.gpu

RV_ERR_INVALID_ARG, RV_ERR_LENGTH_MISMATCH, RV_ERR_UNSUPPORTED, RV_ERR_OOM = 1, 2, 5, 7


# ---- host columns <-> cells -------------------------------------------------------------------------------------------------------
def host_column(dtype, cells):
    n = len(cells)
    if dtype == RV_NULL:
        return Column.nulls(n)
    if dtype == RV_STRING:
        return Column.from_strings(cells)
    valid = np.array([c is not None for c in cells], dtype=bool)
    fill = {RV_INT64: 0, RV_FLOAT64: 0.0, RV_BOOLEAN: False}[dtype]
    npd = {RV_INT64: np.int64, RV_FLOAT64: np.float64, RV_BOOLEAN: np.bool_}[dtype]
    vals = np.array([fill if c is None else c for c in cells], dtype=npd)
    return Column.from_numpy(vals, None if valid.all() else valid)


def cells_of(col: Column):
    if col.dtype == RV_NULL:
        return [None] * col.length
    if col.dtype == RV_STRING:
        return col.to_strings()
    vals = col.logical_values()
    valid = col.logical_valid()
    out = []
    for i in range(col.length):
        if valid is not None and not valid[i]:
            out.append(None)
        elif col.dtype == RV_FLOAT64:
            out.append(float(vals[i]))
        elif col.dtype == RV_BOOLEAN:
            out.append(bool(vals[i]))
        else:
            out.append(int(vals[i]))
    return out


def upload(ctx, dtype, cells, pad: int = 0):
    """A device column of `cells`; pad > 0: a slice at row `pad` of a longer column (offset not a multiple of 64, validity
    at a bit offset)."""
    if pad == 0:
        return ctx.upload(host_column(dtype, cells))
    filler = [None if dtype == RV_NULL else {RV_INT64: 5, RV_FLOAT64: 5.0, RV_BOOLEAN: True, RV_STRING: "pad"}[dtype]] * pad
    whole = list(filler) + list(cells) + list(filler[:7])
    return ctx.upload(host_column(dtype, whole)).slice(pad, len(cells))


def run_join(ctx, probe_frame, build_frame, build_key, probe_key, pad=0):
    """rv_hash_join over frames of (name, dtype, cells) against the model; returns the pair count."""
    bcols = [upload(ctx, d, c, pad) for _, d, c in build_frame]
    pcols = [upload(ctx, d, c, pad) for _, d, c in probe_frame]
    bi = [n for n, _, _ in build_frame].index(build_key)
    pi = [n for n, _, _ in probe_frame].index(probe_key)
    outs, rows = ctx.hash_join(bcols, bi, pcols, pi)
    pairs = inner_join_pairs(build_frame[bi][1], build_frame[bi][2], probe_frame[pi][1], probe_frame[pi][2])
    want = materialize(probe_frame, build_frame, build_key, pairs)
    assert rows == len(pairs)
    assert len(outs) == len(want)
    for o, (name, dtype, cells) in zip(outs, want):
        got = o.download()
        assert got.dtype == dtype, name
        assert got.length == len(pairs), name
        assert comparable(dtype, cells_of(got)) == comparable(dtype, cells), name
    return rows


def probe_pairs(table, key):
    pi, bi, rows = table.probe(key)
    a = pi.download().logical_values() if rows else np.zeros(0, np.int64)
    b = bi.download().logical_values() if rows else np.zeros(0, np.int64)
    assert pi.length == rows and bi.length == rows and pi.null_count() == 0 and bi.null_count() == 0
    return list(zip(a.tolist(), b.tolist()))


def random_keys(rng, dtype, n, distinct, null_share):
    if dtype == RV_NULL:
        return [None] * n
    if dtype == RV_INT64:
        base = rng.integers(-distinct, distinct, n).tolist()
    elif dtype == RV_FLOAT64:
        pool = [0.0, -0.0, float("nan"), float("inf"), -1.5] + (rng.integers(0, distinct, distinct) * 0.25).tolist()
        base = [pool[i] for i in rng.integers(0, len(pool), n)]
    else:
        base = (rng.integers(0, 2, n) == 1).tolist()
    nulls = rng.random(n) < null_share
    return [None if z else v for v, z in zip(base, nulls)]


def payloads(rng, n, tag):
    return [
        (f"i{tag}", RV_INT64, [None if rng.random() < 0.2 else int(x) for x in rng.integers(-10**12, 10**12, n)]),
        (f"f{tag}", RV_FLOAT64, [None if rng.random() < 0.2 else float(x) for x in rng.normal(size=n)]),
        (f"b{tag}", RV_BOOLEAN, [None if rng.random() < 0.2 else bool(x) for x in rng.integers(0, 2, n)]),
        (f"s{tag}", RV_STRING, [None if rng.random() < 0.2 else "x" * int(x) + str(i) for i, x in enumerate(rng.integers(0, 9, n))]),
        (f"z{tag}", RV_NULL, [None] * n),
    ]


# ---- every key dtype, with and without nulls, payloads of every dtype on both sides -----------------------------------------------
@pytest.mark.parametrize("dtype", [RV_INT64, RV_FLOAT64, RV_BOOLEAN, RV_NULL])
@pytest.mark.parametrize("null_share", [0.0, 0.1])
def test_key_dtypes_with_payloads(gpu_ctx, dtype, null_share):
    rng = np.random.default_rng(dtype * 10 + int(null_share * 10))
    nb, np_ = (300, 500) if dtype in (RV_BOOLEAN, RV_NULL) else (3000, 5000)
    build = [("k", dtype, random_keys(rng, dtype, nb, 1500, null_share))] + payloads(rng, nb, "b")
    probe = payloads(rng, np_, "p") + [("k", dtype, random_keys(rng, dtype, np_, 1500, null_share))]
    run_join(gpu_ctx, probe, build, "k", "k")


def test_int64_keys_against_float64_keys_meet_null_to_null(gpu_ctx):
    rng = np.random.default_rng(7)
    build = [("k", RV_INT64, random_keys(rng, RV_INT64, 400, 50, 0.1)), ("v", RV_INT64, list(range(400)))]
    probe = [("k", RV_FLOAT64, random_keys(rng, RV_FLOAT64, 600, 50, 0.1))]
    assert run_join(gpu_ctx, probe, build, "k", "k") > 0


def test_name_collisions_and_column_order(gpu_ctx):
    build = [("id", RV_INT64, [1, 2, 2, None]), ("amount", RV_FLOAT64, [0.5, -0.0, 2.5, None]), ("tag", RV_STRING, ["a", None, "c", "d"])]
    probe = [("amount", RV_FLOAT64, [1.0, 2.0, 3.0]), ("id", RV_INT64, [2, None, 1])]
    run_join(gpu_ctx, probe, build, "id", "id")


# ---- slices ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [37, 101])
def test_sliced_inputs(gpu_ctx, pad):
    rng = np.random.default_rng(pad)
    build = [("k", RV_INT64, random_keys(rng, RV_INT64, 700, 200, 0.1))] + payloads(rng, 700, "b")
    probe = [("k", RV_INT64, random_keys(rng, RV_INT64, 900, 200, 0.1))] + payloads(rng, 900, "p")
    run_join(gpu_ctx, probe, build, "k", "k", pad=pad)
    bk = [("k", RV_BOOLEAN, random_keys(rng, RV_BOOLEAN, 90, 2, 0.2))]
    pk = [("k", RV_BOOLEAN, random_keys(rng, RV_BOOLEAN, 70, 2, 0.2)), ("s", RV_STRING, [str(i) for i in range(70)])]
    run_join(gpu_ctx, pk, bk, "k", "k", pad=pad)


# ---- empty inputs and empty results ------------------------------------------------------------------------------------------------
def test_zero_row_build_zero_row_probe_zero_pairs(gpu_ctx):
    cols = lambda n, base: [("k", RV_INT64, [base + i for i in range(n)]), ("s", RV_STRING, ["v"] * n), ("b", RV_BOOLEAN, [True] * n),
                            ("f", RV_FLOAT64, [1.0] * n), ("z", RV_NULL, [None] * n)]
    assert run_join(gpu_ctx, cols(5, 0), cols(0, 0), "k", "k") == 0
    assert run_join(gpu_ctx, cols(0, 0), cols(5, 0), "k", "k") == 0
    assert run_join(gpu_ctx, cols(5, 100), cols(5, 0), "k", "k") == 0
    assert run_join(gpu_ctx, cols(0, 0), cols(0, 0), "k", "k") == 0


# ---- skew ----------------------------------------------------------------------------------------------------------------------------
def test_one_list_of_1e5_build_rows(gpu_ctx):
    n = 100_000
    t = gpu_ctx.join_build(gpu_ctx.upload(Column.from_numpy(np.full(n, 42, np.int64))))
    assert t.info()[2] == n
    got = probe_pairs(t, gpu_ctx.upload(Column.from_numpy(np.array([1, 42, 3, 42], np.int64))))
    assert gpu_ctx.last_kernel() == "join_probe_emit<2>"
    assert got == [(1, b) for b in range(n)] + [(3, b) for b in range(n)]
    t.free()


def test_1e5_probe_rows_hit_one_key(gpu_ctx):
    n = 100_000
    t = gpu_ctx.join_build(gpu_ctx.upload(Column.from_numpy(np.arange(1000, dtype=np.int64))))
    got = probe_pairs(t, gpu_ctx.upload(Column.from_numpy(np.full(n, 777, np.int64))))
    assert gpu_ctx.last_kernel() == "join_probe_emit<0>"
    assert got == [(p, 777) for p in range(n)]
    t.free()


# ---- collisions --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 3])
def test_hash_masked_to_a_few_bits(gpu_ctx, bits):
    rng = np.random.default_rng(bits)
    gpu_ctx.set_option("join_hash_bits", bits)
    try:
        build = [("k", RV_FLOAT64, random_keys(rng, RV_FLOAT64, 2000, 400, 0.05)), ("v", RV_INT64, list(range(2000)))]
        probe = [("k", RV_FLOAT64, random_keys(rng, RV_FLOAT64, 3000, 400, 0.05))]
        run_join(gpu_ctx, probe, build, "k", "k")
        build = [("k", RV_INT64, rng.integers(0, 10**15, 3000).tolist())]
        probe = [("k", RV_INT64, [build[0][2][i] for i in rng.integers(0, 3000, 2000)] + rng.integers(0, 10**15, 500).tolist())]
        run_join(gpu_ctx, probe, build, "k", "k")
    finally:
        gpu_ctx.set_option("join_hash_bits", 0)


# ---- one table, many probes -------------------------------------------------------------------------------------------------------
def test_one_table_probed_twice_and_by_two_slices(gpu_ctx):
    rng = np.random.default_rng(11)
    bcells = random_keys(rng, RV_INT64, 5000, 800, 0.05)
    pcells = random_keys(rng, RV_INT64, 20000, 800, 0.05)
    t = gpu_ctx.join_build(upload(gpu_ctx, RV_INT64, bcells))
    key = upload(gpu_ctx, RV_INT64, pcells)
    first = probe_pairs(t, key)
    assert first == inner_join_pairs(RV_INT64, bcells, RV_INT64, pcells)
    assert probe_pairs(t, key) == first
    cut = 8765
    lo = probe_pairs(t, key.slice(0, cut))
    hi = probe_pairs(t, key.slice(cut, len(pcells) - cut))
    assert lo + [(p + cut, b) for p, b in hi] == first
    t.free()


# ---- both sides of every switch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("longest,kernel", [(1, 0), (2, 1), (32, 1), (33, 2)])
def test_emit_kernel_by_longest_list(gpu_ctx, longest, kernel):
    """kJoinLaneListMost = 32 (thresholds.hpp): lists of up to 32 rows lane by lane, longer by the workgroup; lists of one row
    the plain compaction."""
    rng = np.random.default_rng(longest)
    bcells = list(range(500)) + [7] * (longest - 1) + ([None, 3] if longest > 1 else [])
    bcells = [bcells[i] for i in rng.permutation(len(bcells))]
    pcells = rng.integers(-20, 600, 9000).tolist() + [None, 7]
    t = gpu_ctx.join_build(upload(gpu_ctx, RV_INT64, bcells))
    assert t.info()[2] == longest
    assert probe_pairs(t, upload(gpu_ctx, RV_INT64, pcells)) == inner_join_pairs(RV_INT64, bcells, RV_INT64, pcells)
    assert gpu_ctx.last_kernel() == f"join_probe_emit<{kernel}>"
    t.free()


# ---- errors leave the context usable and create nothing ----------------------------------------------------------------------------
def _status(fn):
    with pytest.raises(RvError) as e:
        fn()
    return e.value.status


def test_errors(gpu_ctx):
    a = gpu_ctx.upload(host_column(RV_INT64, [1, 2, 3]))
    b = gpu_ctx.upload(host_column(RV_INT64, [1, 2]))
    s = gpu_ctx.upload(host_column(RV_STRING, ["x", "y", "z"]))
    assert _status(lambda: gpu_ctx.hash_join([a], 1, [a], 0)) == RV_ERR_INVALID_ARG
    assert _status(lambda: gpu_ctx.hash_join([a], 0, [a], 2)) == RV_ERR_INVALID_ARG
    assert _status(lambda: gpu_ctx.hash_join([a, b], 0, [a], 0)) == RV_ERR_LENGTH_MISMATCH
    assert _status(lambda: gpu_ctx.hash_join([a], 0, [a, b], 0)) == RV_ERR_LENGTH_MISMATCH
    assert _status(lambda: gpu_ctx.hash_join([s, a], 0, [a], 0)) == RV_ERR_UNSUPPORTED
    assert _status(lambda: gpu_ctx.hash_join([a], 0, [s], 0)) == RV_ERR_UNSUPPORTED
    assert _status(lambda: gpu_ctx.join_build(s)) == RV_ERR_UNSUPPORTED
    t = gpu_ctx.join_build(a)
    assert _status(lambda: t.probe(s)) == RV_ERR_UNSUPPORTED
    assert probe_pairs(t, b) == [(0, 0), (1, 1)]
    t.free()
    outs, rows = gpu_ctx.hash_join([a, s], 0, [a], 0)
    assert rows == 3 and outs[1].download().to_strings() == ["x", "y", "z"]


def test_pair_count_beyond_the_device_is_oom(gpu_ctx):
    """2e5 equal build keys x 1e6 probe rows of that key = 2e11 pairs, 3.2 TB of indices: refused after the count pass,
    before any output is allocated or written."""
    t = gpu_ctx.join_build(gpu_ctx.upload(Column.from_numpy(np.full(200_000, 9, np.int64))))
    key = gpu_ctx.upload(Column.from_numpy(np.full(1_000_000, 9, np.int64)))
    assert _status(lambda: t.probe(key)) == RV_ERR_OOM
    assert gpu_ctx.last_kernel() == "join_probe_count"
    small = gpu_ctx.upload(Column.from_numpy(np.array([9, 8], np.int64)))
    pi, bi, rows = t.probe(small)
    assert rows == 200_000 and bi.download().logical_values()[-1] == 199_999
    t.free()


# ---- scale ------------------------------------------------------------------------------------------------------------------------
def test_scale_1e8_probe_rows_against_1e6_keys(gpu_ctx):
    """1e8 probe rows against 1e6 unique Int64 keys at ~10 % hits, exact pairs against numpy (sorted keys + searchsorted); the
    same probe against 8 build rows per key: counts and windows of the pairs."""
    rng = np.random.default_rng(2024)
    nb, npr = 1_000_000, 100_000_000
    bkeys = rng.permutation(nb).astype(np.int64) * 10       # 1e6 unique keys, the multiples of 10 below 1e7
    pkeys = rng.integers(0, 10 * nb, npr, dtype=np.int64)   # ~10 % of the probe rows hit
    key = gpu_ctx.upload(Column.from_numpy(pkeys))
    hit = np.nonzero(pkeys % 10 == 0)[0]
    order = np.argsort(bkeys, kind="stable")
    sk = bkeys[order]
    pos = np.searchsorted(sk, pkeys[hit])
    assert np.array_equal(sk[pos], pkeys[hit])
    t = gpu_ctx.join_build(gpu_ctx.upload(Column.from_numpy(bkeys)))
    pi, bi, rows = t.probe(key)
    assert gpu_ctx.last_kernel() == "join_probe_emit<0>"
    assert rows == len(hit) and 0.09 < rows / npr < 0.11
    assert np.array_equal(pi.download().logical_values(), hit)
    assert np.array_equal(bi.download().logical_values(), order[pos])
    t.free()
    del pi, bi
    b8 = np.repeat(bkeys, 8)[rng.permutation(8 * nb)]
    order8 = np.argsort(b8, kind="stable")                   # each key's 8 rows ascending
    sk8 = b8[order8]
    t8 = gpu_ctx.join_build(gpu_ctx.upload(Column.from_numpy(b8)))
    assert t8.info()[2] == 8
    pi, bi, rows = t8.probe(key)
    assert gpu_ctx.last_kernel() == "join_probe_emit<1>"
    assert rows == 8 * len(hit)
    w = 10_000  # probe rows per window
    for first in (0, len(hit) // 3, len(hit) - w):
        rows_p = hit[first:first + w]
        lo = np.searchsorted(sk8, pkeys[rows_p], "left")
        want_b = order8[lo[:, None] + np.arange(8)].ravel()
        assert np.array_equal(pi.slice(first * 8, w * 8).download().logical_values(), np.repeat(rows_p, 8))
        assert np.array_equal(bi.slice(first * 8, w * 8).download().logical_values(), want_b)
    t8.free()
