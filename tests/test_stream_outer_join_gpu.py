"""GPU suite: rv_hash_join_chunked_kind, the window call of the streaming outer, semi and anti joins.  Output batch b must equal
rv_hash_join_kind of the whole build side against probe batch b alone (tests/outer_join_model.py): rows per batch, cells at AnyValue
level, dtypes and null counts."""
import numpy as np
import pytest

from join_model import comparable
from outer_join_model import FULL_OUTER, INNER, KIND_NAMES, PROBE_ANTI, PROBE_OUTER, PROBE_SEMI, join_pairs, materialize_kind
from rivulus_amd.capi import RV_FLOAT64, RV_INT64, RV_NULL, RV_STRING, RvError
from test_join_gpu import cells_of, payloads, random_keys, upload

pytestmark = pytest.mark.gpu

RV_ERR_UNSUPPORTED, RV_ERR_INVALID_ARG = 5, 1
STREAMED = (PROBE_OUTER, PROBE_SEMI, PROBE_ANTI)


def run_chunked_kind(ctx, kind, probe_frame, build_frame, build_key, probe_key, chunk, max_pairs=0, eager_batches=2, first_row=0):
    """rv_hash_join_chunked_kind over the probe rows from `first_row` on against the model, batch by batch, and against
    rv_hash_join_kind on the first `eager_batches` batch slices; returns (rows per batch, batches taken, the call's last_kernel, the table's longest list)."""
    probe_frame = [(n, d, c[first_row:]) for n, d, c in probe_frame]
    bcols = [upload(ctx, d, c) for _, d, c in build_frame]
    pcols = [upload(ctx, d, c) for _, d, c in probe_frame]
    bi = [n for n, _, _ in build_frame].index(build_key)
    pi = [n for n, _, _ in probe_frame].index(probe_key)
    table = ctx.join_build(bcols[bi])
    outs, rows, nulls, total, taken = ctx.hash_join_chunked(table, bcols, bi, pcols, pi, chunk, max_pairs, kind=kind)
    kernel = ctx.last_kernel()
    n = len(probe_frame[0][2])
    k = (n + chunk - 1) // chunk
    assert len(rows) == k and (taken >= 1 if k else taken == 0)
    assert total == int(rows[:taken].sum())
    got = [cells_of(o.download()) for o in outs]
    at = 0
    for b in range(k):
        lo = b * chunk
        sl = [(name, dtype, cells[lo:lo + chunk]) for name, dtype, cells in probe_frame]
        pairs = join_pairs(kind, build_frame[bi][1], build_frame[bi][2], sl[pi][1], sl[pi][2])
        assert int(rows[b]) == len(pairs), (KIND_NAMES[kind], b)  # every batch's count, taken or not
        if b >= taken:
            continue
        want = materialize_kind(kind, sl, build_frame, build_key, pairs)
        assert len(outs) == len(want)
        r = len(pairs)
        for j, (o, (name, dtype, cells)) in enumerate(zip(outs, want)):
            assert o.info().dtype == dtype, name
            assert comparable(dtype, got[j][at:at + r]) == comparable(dtype, cells), (KIND_NAMES[kind], b, name)
            assert nulls[b, j] == sum(c is None for c in cells), (KIND_NAMES[kind], b, name)
        if b < eager_batches:  # the eager call on the batch slice alone
            eo, er = ctx.hash_join(bcols, bi, [c.slice(lo, min(chunk, n - lo)) for c in pcols], pi, kind=kind)
            assert er == r
            for j in range(len(outs)):
                d = want[j][1]  # compared as AnyValue: a NaN by its bits
                assert comparable(d, cells_of(eo[j].download())) == comparable(d, got[j][at:at + r])
        at += r
    assert all(o.length == at for o in outs)
    longest = table.info()[2]
    table.free()
    return rows, taken, kernel, longest


def frames(rng, nb, npr, distinct, longest=1):
    bk = random_keys(rng, RV_INT64, nb, distinct, 0.05) + [distinct + 5] * (longest - 1)
    build = [("k", RV_INT64, bk)] + payloads(rng, len(bk), "b")
    probe = payloads(rng, npr, "p") + [("k", RV_INT64, random_keys(rng, RV_INT64, npr, 2 * distinct, 0.05))]
    return build, probe


# ---- both count passes, batches inside and across tiles ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", STREAMED, ids=[KIND_NAMES[k] for k in STREAMED])
@pytest.mark.parametrize("chunk", [1024, 1000, 4097])
def test_batch_equals_the_eager_join_of_the_batch(gpu_ctx, kind, chunk):
    """1024: the FAST count pass (four batches per tile); 1000 and 4097: the general one, batches ending inside tiles and spanning them."""
    rng = np.random.default_rng(chunk + kind)
    build, probe = frames(rng, 1500, 9001, 1200)
    rows, taken, kernel, longest = run_chunked_kind(gpu_ctx, kind, probe, build, "k", "k", chunk)
    assert taken == len(rows) and rows.sum() > 0
    mode = 0 if kind != PROBE_OUTER or longest <= 1 else 1 if longest <= 32 else 2
    assert kernel == f"join_probe_emit<{mode},{KIND_NAMES[kind]}>"


@pytest.mark.parametrize("kind", STREAMED, ids=[KIND_NAMES[k] for k in STREAMED])
def test_long_lists_and_float_keys(gpu_ctx, kind):
    rng = np.random.default_rng(40 + kind)
    build, probe = frames(rng, 400, 5000, 300, longest=40)
    probe[-1] = ("k", RV_INT64, [c if i % 50 else 305 for i, c in enumerate(probe[-1][2])])  # the long list is hit
    for chunk in (1024, 1000):
        run_chunked_kind(gpu_ctx, kind, probe, build, "k", "k", chunk, eager_batches=1)
    bk = [0.0, -0.0, float("nan"), None, 1.5, 1.5, 2.5]
    pk = [bk[i] for i in rng.integers(0, len(bk), 3000)]
    build = [("k", RV_FLOAT64, bk), ("s", RV_STRING, [str(i) for i in range(len(bk))])]
    probe = [("k", RV_FLOAT64, pk), ("z", RV_NULL, [None] * 3000)]
    for chunk in (1024, 4097):
        run_chunked_kind(gpu_ctx, kind, probe, build, "k", "k", chunk, eager_batches=1)


@pytest.mark.parametrize("kind", STREAMED, ids=[KIND_NAMES[k] for k in STREAMED])
def test_empty_probe_empty_build_and_batches_without_rows(gpu_ctx, kind):
    build = [("k", RV_INT64, [1, 2, 3]), ("s", RV_STRING, ["a", "b", "c"])]
    rows, taken, kernel, _ = run_chunked_kind(gpu_ctx, kind, [("k", RV_INT64, [])], build, "k", "k", 1024)
    assert len(rows) == 0 and taken == 0 and kernel == "join_probe_count_batched"
    for chunk in (1024, 1000):
        rows, taken, _, _ = run_chunked_kind(gpu_ctx, kind, [("k", RV_INT64, [7] * 3000)], build, "k", "k", chunk)  # nothing matches
        assert rows.sum() == (0 if kind == PROBE_SEMI else 3000) and taken == len(rows)
        rows, taken, _, _ = run_chunked_kind(gpu_ctx, kind, [("k", RV_INT64, [2] * 3000)], [("k", RV_INT64, [])], "k", "k", chunk)  # empty build side
        assert rows.sum() == (0 if kind == PROBE_SEMI else 3000)


# ---- max_pairs cuts a prefix of batches; the caller resumes behind it ------------------------------------------------------------
@pytest.mark.parametrize("kind", STREAMED, ids=[KIND_NAMES[k] for k in STREAMED])
@pytest.mark.parametrize("chunk", [1024, 1000])
def test_max_pairs_cut_resumes(gpu_ctx, kind, chunk):
    rng = np.random.default_rng(chunk * 3 + kind)
    build, probe = frames(rng, 1500, 9001, 1200)
    n = 9001
    all_rows, taken, _, _ = run_chunked_kind(gpu_ctx, kind, probe, build, "k", "k", chunk)
    assert taken == len(all_rows)
    cap = int(all_rows[:3].sum()) + 1  # three batches fit, the fourth does not (every batch of this data has rows)
    assert all_rows[3] > 1
    first, seen = 0, []
    while first < n:
        rows, taken, _, _ = run_chunked_kind(gpu_ctx, kind, probe, build, "k", "k", chunk, max_pairs=cap, eager_batches=0, first_row=first)
        assert 1 <= taken <= len(rows)
        assert taken == len(rows) or int(rows[:taken].sum()) <= cap < int(rows[:taken + 1].sum())
        seen += rows[:taken].tolist()
        first += taken * chunk
    assert seen == all_rows.tolist()
    assert sum(seen) == len(join_pairs(kind, RV_INT64, build[0][2], RV_INT64, probe[-1][2]))  # out_rows sums to the whole join's total


def test_inner_kind_is_rv_hash_join_chunked(gpu_ctx):
    rng = np.random.default_rng(5)
    build, probe = frames(rng, 1500, 5000, 1200)
    bcols = [upload(gpu_ctx, d, c) for _, d, c in build]
    pcols = [upload(gpu_ctx, d, c) for _, d, c in probe]
    table = gpu_ctx.join_build(bcols[0])
    for chunk in (1024, 1000):
        a = gpu_ctx.hash_join_chunked(table, bcols, 0, pcols, len(pcols) - 1, chunk)
        ka = gpu_ctx.last_kernel()
        b = gpu_ctx.hash_join_chunked(table, bcols, 0, pcols, len(pcols) - 1, chunk, kind=INNER)
        assert gpu_ctx.last_kernel() == ka
        assert a[1].tolist() == b[1].tolist() and a[3] == b[3] and a[4] == b[4] and np.array_equal(a[2], b[2])
        for x, y in zip(a[0], b[0]):
            assert x.download().same_as(y.download()) is None
    table.free()


def test_full_outer_is_unsupported(gpu_ctx):
    a = upload(gpu_ctx, RV_INT64, [1, 2, 3])
    table = gpu_ctx.join_build(a)
    with pytest.raises(RvError) as e:
        gpu_ctx.hash_join_chunked(table, [a], 0, [a], 0, 1024, kind=FULL_OUTER)
    assert e.value.status == RV_ERR_UNSUPPORTED and "rv_hash_join_kind" in str(e.value)
    with pytest.raises(RvError) as e:
        gpu_ctx.hash_join_chunked(table, [a], 0, [a], 0, 1024, kind=7)
    assert e.value.status == RV_ERR_INVALID_ARG
    outs, rows, _, total, taken = gpu_ctx.hash_join_chunked(table, [a], 0, [a], 0, 1024, kind=PROBE_SEMI)  # the context still works
    assert rows.tolist() == [3] and total == 3 and taken == 1 and len(outs) == 1
    table.free()
