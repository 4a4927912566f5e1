"""GPU suite: rv_hash_join_chunked, the window call of the streaming inner join.  Output batch b must equal rv_hash_join of the
whole build side against probe batch b alone (tests/join_model.py, plan.rs:174-284): pairs per batch, cells at AnyValue level,
dtypes, null counts, and a bitmap on a batch's slice exactly when the batch holds a null."""
import numpy as np
import pytest

from join_model import comparable, inner_join_pairs, materialize
from rivulus_amd.capi import RV_BOOLEAN, RV_FLOAT64, RV_INT64, RV_NULL, RV_STRING, Column, RvError
from test_join_gpu import cells_of, payloads, random_keys, upload

pytestmark = pytest.mark.gpu

RV_ERR_INVALID_ARG, RV_ERR_LENGTH_MISMATCH, RV_ERR_UNSUPPORTED, RV_ERR_OOM = 1, 2, 5, 7


def run_chunked(ctx, probe_frame, build_frame, build_key, probe_key, chunk, pad=0, max_pairs=0, eager_batches=4):
    """rv_hash_join_chunked over frames of (name, dtype, cells) against the model, batch by batch, and against rv_hash_join on
    the first `eager_batches` batch slices; returns (rows per batch, batches taken, the outputs, the call's last_kernel)."""
    bcols = [upload(ctx, d, c, pad) for _, d, c in build_frame]
    pcols = [upload(ctx, d, c, pad) for _, d, c in probe_frame]
    bi = [n for n, _, _ in build_frame].index(build_key)
    pi = [n for n, _, _ in probe_frame].index(probe_key)
    table = ctx.join_build(bcols[bi])
    outs, rows, nulls, total, taken = ctx.hash_join_chunked(table, bcols, bi, pcols, pi, chunk, max_pairs)
    kernel = ctx.last_kernel()
    n = len(probe_frame[0][2])
    k = (n + chunk - 1) // chunk
    assert len(rows) == k and (taken >= 1 if k else taken == 0)
    assert total == int(rows[:taken].sum())
    pairs = inner_join_pairs(build_frame[bi][1], build_frame[bi][2], probe_frame[pi][1], probe_frame[pi][2])
    per_batch = [[] for _ in range(k)]
    for p, b in pairs:
        per_batch[p // chunk].append((p % chunk, b))
    assert [len(x) for x in per_batch] == rows.tolist()  # every batch's count, taken or not
    got = [cells_of(o.download()) for o in outs]
    nout = len(outs)
    at = 0
    for b in range(taken):
        lo = b * chunk
        sl = [(name, dtype, cells[lo:lo + chunk]) for name, dtype, cells in probe_frame]
        want = materialize(sl, build_frame, build_key, per_batch[b])
        r = int(rows[b])
        for j, (o, (name, dtype, cells)) in enumerate(zip(outs, want)):
            assert o.info().dtype == dtype, name
            seg = got[j][at:at + r]
            assert comparable(dtype, seg) == comparable(dtype, cells), (b, name)
            assert nulls[b, j] == sum(c is None for c in cells), (b, name)
            piece = ctx.slice_known(o, at, r, int(nulls[b, j]))
            has_bitmap = piece.info().has_validity != 0
            assert has_bitmap == (dtype != RV_NULL and nulls[b, j] > 0), (b, name)
        if b < eager_batches:  # the eager call on the batch slice alone
            eo, er = ctx.hash_join(bcols, bi, [c.slice(lo, min(chunk, n - lo)) for c in pcols], pi)
            assert er == r
            for j in range(nout):
                assert cells_of(eo[j].download()) == got[j][at:at + r]
        at += r
    table.free()
    return rows, taken, outs, kernel


def frames(rng, nb, npr, dtype, distinct, null_share, with_payloads=True):
    build = [("k", dtype, random_keys(rng, dtype, nb, distinct, null_share))] + (payloads(rng, nb, "b") if with_payloads else [])
    probe = (payloads(rng, npr, "p") if with_payloads else []) + [("k", dtype, random_keys(rng, dtype, npr, distinct, null_share))]
    return build, probe


# ---- batch sizes: both count passes, batches inside and across tiles ------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 255, 256, 1000, 1024, 4096, 5000, 2 ** 20])
def test_batch_sizes(gpu_ctx, chunk):
    rng = np.random.default_rng(chunk)
    n = 9001 if chunk > 1 else 4500
    build = [("k", RV_INT64, rng.integers(0, 3000, 2500).tolist()), ("v", RV_INT64, list(range(2500)))]
    probe = [("k", RV_INT64, rng.integers(0, 6000, n).tolist()), ("s", RV_STRING, [str(i) for i in range(n)])]
    run_chunked(gpu_ctx, probe, build, "k", "k", chunk)
    # a probe side whose batches all end inside tiles, plus one row
    probe = [("k", RV_INT64, rng.integers(0, 6000, 3 * 4096 + 1).tolist())]
    run_chunked(gpu_ctx, probe, build, "k", "k", chunk, eager_batches=1)


@pytest.mark.parametrize("chunk", [1024, 1000])
def test_empty_probe_and_zero_pairs(gpu_ctx, chunk):
    build = [("k", RV_INT64, [1, 2, 3]), ("s", RV_STRING, ["a", "b", "c"]), ("z", RV_NULL, [None] * 3)]
    rows, taken, outs, kernel = run_chunked(gpu_ctx, [("k", RV_INT64, [])], build, "k", "k", chunk)
    assert len(rows) == 0 and taken == 0 and [o.length for o in outs] == [0, 0, 0]
    assert kernel == "join_probe_count_batched"
    rows, taken, outs, kernel = run_chunked(gpu_ctx, [("k", RV_INT64, [7] * 3000)], build, "k", "k", chunk)
    assert rows.sum() == 0 and taken == len(rows) and outs[1].download().to_strings() == []
    assert kernel == "join_probe_count_batched"
    rows, taken, _, _ = run_chunked(gpu_ctx, [("k", RV_INT64, [7] * 3000)], [("k", RV_INT64, [])], "k", "k", chunk)
    assert rows.sum() == 0


# ---- key dtypes x list lengths: every emit kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [RV_INT64, RV_FLOAT64, RV_BOOLEAN, RV_NULL])
@pytest.mark.parametrize("lists", ["unique", "dup32", "skewed"])
def test_key_dtypes_and_list_lengths(gpu_ctx, dtype, lists):
    rng = np.random.default_rng(dtype * 7 + len(lists))
    npr = 6000
    if dtype == RV_BOOLEAN:
        bcells = {"unique": [True, False, None], "dup32": [True] * 32 + [False] * 5 + [None] * 3, "skewed": [True] * 200 + [False, None]}[lists]
    elif dtype == RV_NULL:
        bcells = [None] * {"unique": 1, "dup32": 32, "skewed": 200}[lists]
    elif dtype == RV_FLOAT64:
        base = [0.0, -0.0, float("nan"), float("inf"), None] + [i * 0.25 for i in range(1, 400)]
        bcells = {"unique": base, "dup32": base + [1.5] * 31 + [-0.0] * 10, "skewed": base + [2.0] * 100}[lists]
    else:
        base = list(range(-200, 600))
        bcells = {"unique": base, "dup32": base + [5] * 31 + [None] * 3, "skewed": base + [9] * 99 + [None]}[lists]
    bcells = [bcells[i] for i in rng.permutation(len(bcells))]
    longest = max([bcells.count(x) for x in set(bcells) if not (isinstance(x, float) and x != x)] or [0])
    if dtype == RV_FLOAT64:  # +0.0 / -0.0 are two keys, NaN none: count by bits
        from join_model import any_key
        keys = [any_key(dtype, x) for x in bcells]
        longest = max(keys.count(x) for x in set(keys) if x is not None)
    mode = 0 if longest <= 1 else 1 if longest <= 32 else 2
    pk = random_keys(rng, dtype, npr, 600, 0.05) if dtype != RV_FLOAT64 else [bcells[i] for i in rng.integers(0, len(bcells), npr)]
    build = [("k", dtype, bcells), ("v", RV_INT64, list(range(len(bcells))))]
    probe = [("k", dtype, pk), ("f", RV_FLOAT64, rng.normal(size=npr).tolist())]
    for chunk in (1024, 1000):
        rows, _, _, kernel = run_chunked(gpu_ctx, probe, build, "k", "k", chunk, eager_batches=2)
        if rows.sum():
            assert kernel == f"join_probe_emit<{mode}>", (lists, longest)


# ---- payloads of every dtype, a probe frame that is a slice ------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 37])
def test_payloads_and_slices(gpu_ctx, pad):
    rng = np.random.default_rng(100 + pad)
    build, probe = frames(rng, 900, 5000, RV_INT64, 300, 0.1)
    for chunk in (1024, 333):
        run_chunked(gpu_ctx, probe, build, "k", "k", chunk, pad=pad)


def test_two_calls_give_identical_outputs(gpu_ctx):
    rng = np.random.default_rng(5)
    bk = rng.integers(0, 500, 4000)
    pk = rng.integers(0, 700, 50_000)
    b = [gpu_ctx.upload(Column.from_numpy(bk)), gpu_ctx.upload(Column.from_numpy(np.arange(4000, dtype=np.int64)))]
    p = [gpu_ctx.upload(Column.from_numpy(pk))]
    t = gpu_ctx.join_build(b[0])
    first = gpu_ctx.hash_join_chunked(t, b, 0, p, 0, 1000)
    second = gpu_ctx.hash_join_chunked(t, b, 0, p, 0, 1000)
    assert np.array_equal(first[1], second[1]) and first[3] == second[3]
    for x, y in zip(first[0], second[0]):
        assert np.array_equal(x.download().logical_values(), y.download().logical_values())
    t.free()


def test_null_counts_of_long_and_ragged_batches(gpu_ctx):
    """Per-batch null counts where the segmented count cuts a range into chunks: 601 090 probe rows in batches of 300 001 (about
    270 000 pairs each, 4219 bitmap words against chunks of 4096; every later boundary mid-word; a ragged last batch), then in
    batches of 1024.  Three output columns keep nulls -- a probe Int64, a build Float64 and a build String -- so three bitmaps share
    one table upload and one read-back.  Unique Int64 build keys, ~10 % of the probe rows miss: the model is numpy."""
    rng = np.random.default_rng(601_090)
    nb, npr = 50_000, 601_090
    bkeys = rng.permutation(nb).astype(np.int64) * 10
    pkeys = rng.integers(0, nb, npr).astype(np.int64) * 10 + (rng.random(npr) < 0.1)  # a key ending in 1 meets nothing
    pv, pv_valid = rng.integers(0, 1000, npr).astype(np.int64), rng.random(npr) > 0.2
    bf, bf_valid = rng.random(nb), rng.random(nb) > 0.3
    bs = [None if m else f"s{i % 97}" for i, m in enumerate(rng.random(nb) < 0.15)]
    bs_valid = np.array([x is not None for x in bs])
    bcols = [gpu_ctx.upload(Column.from_numpy(bkeys)), gpu_ctx.upload(Column.from_numpy(bf, bf_valid)), gpu_ctx.upload(Column.from_strings(bs))]
    pcols = [gpu_ctx.upload(Column.from_numpy(pv, pv_valid)), gpu_ctx.upload(Column.from_numpy(pkeys))]
    hit = np.nonzero(pkeys % 10 == 0)[0]           # the probe row of every pair, in output order
    brow = np.argsort(bkeys)[pkeys[hit] // 10]     # ... and its build row (bkeys = 10 x a permutation)
    assert np.array_equal(bkeys[brow], pkeys[hit])
    valid_out = [pv_valid[hit], np.ones(len(hit), bool), bf_valid[brow], bs_valid[brow]]  # pv, k, bf, bs
    t = gpu_ctx.join_build(bcols[0])
    for chunk in (300_001, 1024):
        outs, rows, nulls, total, taken = gpu_ctx.hash_join_chunked(t, bcols, 0, pcols, 1, chunk)
        k = (npr + chunk - 1) // chunk
        assert taken == k and total == len(hit)
        assert np.array_equal(rows, np.bincount(hit // chunk, minlength=k).astype(np.uint64))
        if chunk == 300_001:
            assert int(rows[0]) > 4096 * 64 and int(rows[2]) < 1088  # two chunks; the ragged batch
        ends = np.cumsum(rows).astype(np.int64)
        for j, v in enumerate(valid_out):
            invalid = np.concatenate([[0], np.cumsum(~v)])
            assert np.array_equal(nulls[:, j], invalid[ends] - invalid[ends - rows.astype(np.int64)]), (chunk, j)
        assert nulls[0, 0] > 0 and nulls[0, 2] > 0 and nulls[0, 3] > 0 and not nulls[:, 1].any()
        got = [o.download() for o in outs]
        assert np.array_equal(got[0].logical_values()[valid_out[0]], pv[hit][valid_out[0]])
        assert np.array_equal(got[1].logical_values(), pkeys[hit])
        assert np.array_equal(got[2].logical_values()[valid_out[2]], bf[brow][valid_out[2]])
        for j in (0, 2, 3):
            assert np.array_equal(got[j].logical_valid(), valid_out[j]), (chunk, j)
        lo = int(ends[0]) - 50  # strings across the first boundary
        assert outs[3].slice(lo, 100).download().to_strings() == [bs[r] for r in brow[lo:lo + 100]]
    t.free()


# ---- max_pairs -----------------------------------------------------------------------------------------------------------------------
def test_max_pairs_cuts_the_window(gpu_ctx):
    rng = np.random.default_rng(9)
    build = [("k", RV_INT64, rng.integers(0, 50, 400).tolist()), ("v", RV_INT64, list(range(400)))]
    probe = [("k", RV_INT64, rng.integers(0, 60, 10_000).tolist())]
    rows, taken, _, _ = run_chunked(gpu_ctx, probe, build, "k", "k", 1024)
    assert taken == len(rows)
    cum = np.cumsum(rows)
    for j in (1, 3, len(rows) - 1):
        cap = int(cum[j - 1])  # exactly j batches fit
        r2, t2, _, _ = run_chunked(gpu_ctx, probe, build, "k", "k", 1024, max_pairs=cap, eager_batches=0)
        assert t2 == j and np.array_equal(r2, rows)
        r3, t3, _, _ = run_chunked(gpu_ctx, probe, build, "k", "k", 1024, max_pairs=cap + int(rows[j]) - 1, eager_batches=0)
        assert t3 == j
    r4, t4, _, _ = run_chunked(gpu_ctx, probe, build, "k", "k", 1024, max_pairs=1, eager_batches=1)  # below one batch: still one
    assert t4 == 1 and np.array_equal(r4, rows)


def test_join_beyond_the_device_streams_its_first_batches(gpu_ctx):
    """2e5 equal build keys x 1e6 probe rows of that key (the shape rv_hash_join refuses with RV_ERR_OOM): every batch holds
    1024 x 2e5 pairs; a cap of 5e8 pairs materialises the first two."""
    nb, npr = 200_000, 1_000_000
    bcols = [gpu_ctx.upload(Column.from_numpy(np.full(nb, 9, np.int64))), gpu_ctx.upload(Column.from_numpy(np.arange(nb, dtype=np.int64)))]
    pcols = [gpu_ctx.upload(Column.from_numpy(np.full(npr, 9, np.int64))), gpu_ctx.upload(Column.from_numpy(np.arange(npr, dtype=np.int64)))]
    with pytest.raises(RvError) as e:
        gpu_ctx.hash_join(bcols[:1], 0, pcols[:1], 0)
    assert e.value.status == RV_ERR_OOM
    t = gpu_ctx.join_build(bcols[0])
    outs, rows, nulls, total, taken = gpu_ctx.hash_join_chunked(t, bcols, 0, pcols, 0, 1024, max_pairs=500_000_000)
    k = (npr + 1023) // 1024
    assert len(rows) == k and taken == 2 and total == 2 * 1024 * nb
    assert np.all(rows[:-1] == 1024 * nb) and rows[-1] == (npr - (k - 1) * 1024) * nb
    assert gpu_ctx.last_kernel() == "join_probe_emit<2>"
    probe_row, build_row = outs[1], outs[2]
    for at in (0, 1024 * nb - 3, 2 * 1024 * nb - 5):
        assert probe_row.slice(at, 3).download().logical_values().tolist() == [(at + i) // nb for i in range(3)]
        assert build_row.slice(at, 3).download().logical_values().tolist() == [(at + i) % nb for i in range(3)]
    del outs, probe_row, build_row
    t.free()


# ---- errors leave the context usable and create nothing -----------------------------------------------------------------------------
def test_errors_then_a_good_call(gpu_ctx):
    a = upload(gpu_ctx, RV_INT64, [1, 2, 3])
    b = upload(gpu_ctx, RV_INT64, [1, 2])
    s = upload(gpu_ctx, RV_STRING, ["x", "y", "z"])
    t = gpu_ctx.join_build(a)
    t2 = gpu_ctx.join_build(b)

    def good():
        outs, rows, _, total, taken = gpu_ctx.hash_join_chunked(t, [a], 0, [a], 0, 2)
        assert rows.tolist() == [2, 1] and total == 3 and taken == 2

    cases = [
        (lambda: gpu_ctx.hash_join_chunked(t, [a], 0, [a], 0, 0), RV_ERR_INVALID_ARG),                 # chunk_rows 0
        (lambda: gpu_ctx.hash_join_chunked(t, [a], 0, [a], 0, 1, nchunks=2), RV_ERR_INVALID_ARG),      # room for 2 of 3 batches
        (lambda: gpu_ctx.hash_join_chunked(t, [a], 1, [a], 0, 2), RV_ERR_INVALID_ARG),                 # build key out of range
        (lambda: gpu_ctx.hash_join_chunked(t, [a], 0, [a], 3, 2), RV_ERR_INVALID_ARG),                 # probe key out of range
        (lambda: gpu_ctx.hash_join_chunked(t2, [a], 0, [a], 0, 2), RV_ERR_LENGTH_MISMATCH),            # not the table's build rows
        (lambda: gpu_ctx.hash_join_chunked(t, [a, b], 0, [a], 0, 2), RV_ERR_LENGTH_MISMATCH),          # unequal build columns
        (lambda: gpu_ctx.hash_join_chunked(t, [a], 0, [a, b], 0, 2), RV_ERR_LENGTH_MISMATCH),          # unequal probe columns
        (lambda: gpu_ctx.hash_join_chunked(t, [a], 0, [s, a], 0, 2), RV_ERR_UNSUPPORTED),              # String probe key
        (lambda: gpu_ctx.hash_join_chunked(t, [s, a], 0, [a], 0, 2), RV_ERR_UNSUPPORTED),              # String build key
    ]
    for fn, status in cases:
        with pytest.raises(RvError) as e:
            fn()
        assert e.value.status == status
        good()
    t.free()
    t2.free()


# ---- scale -------------------------------------------------------------------------------------------------------------------------
def test_scale_1e8_probe_rows_in_1024_row_batches(gpu_ctx):
    """1e8 probe rows at 1024-row batches against 1e6 unique Int64 keys at ~10 % hits: the total, every batch's count and sampled
    batches exactly against numpy (sorted keys + searchsorted)."""
    rng = np.random.default_rng(2025)
    nb, npr, chunk = 1_000_000, 100_000_000, 1024
    bkeys = rng.permutation(nb).astype(np.int64) * 10
    pkeys = rng.integers(0, 10 * nb, npr, dtype=np.int64)
    hit = np.nonzero(pkeys % 10 == 0)[0]
    order = np.argsort(bkeys, kind="stable")
    sk = bkeys[order]
    bcols = [gpu_ctx.upload(Column.from_numpy(bkeys)), gpu_ctx.upload(Column.from_numpy(np.arange(nb, dtype=np.int64)))]
    pcols = [gpu_ctx.upload(Column.from_numpy(pkeys))]
    t = gpu_ctx.join_build(bcols[0])
    outs, rows, nulls, total, taken = gpu_ctx.hash_join_chunked(t, bcols, 0, pcols, 0, chunk)
    k = (npr + chunk - 1) // chunk
    assert taken == k and total == len(hit) and gpu_ctx.last_kernel() == "join_probe_emit<0>"
    assert np.array_equal(rows, np.bincount(hit // chunk, minlength=k).astype(np.uint64))
    assert not nulls.any()
    starts = np.concatenate([[0], np.cumsum(rows)])
    keys_out, build_out = outs[0], outs[1]
    for b in (0, 1, k // 2, k - 1):
        lo, r = int(starts[b]), int(rows[b])
        want_p = hit[(hit >= b * chunk) & (hit < (b + 1) * chunk)]
        assert np.array_equal(keys_out.slice(lo, r).download().logical_values(), pkeys[want_p])
        assert np.array_equal(build_out.slice(lo, r).download().logical_values(), order[np.searchsorted(sk, pkeys[want_p])])
    t.free()
