#!/usr/bin/env python3
"""The streaming inner join against its alternatives: one JSON line per shape (tools/README.md).  Same probe rows for all three:

  a_ms           rv_join_build + rv_hash_join_chunked over the whole probe frame in 1024-row batches, windows of the stream's
                 default (GpuHashJoinStream: 2^28 probe rows, 2^28 pairs), each window continuing from its out_batches
  b_ms           one rv_hash_join over the whole probe frame (builds its own table)
  c_ms_extrap    one rv_hash_join per 1024-row batch (each builds its table: the call a streaming caller has today), timed over
                 the first --per-batch-rows probe rows and EXTRAPOLATED linearly to the whole probe side (c_rows_timed says how many)
  c_probe_ms_extrap  the same with the table built once and rv_join_probe + rv_take_device per batch: the cheapest per-batch
                 pattern without the window call, also extrapolated
  a_over_b, c_over_a   the ratios the targets speak of (a within 1.25x of b; a at least 50x faster than c)
Both sides carry an Int64 payload column.  Times are wall clock around the whole loop (HIP events on an idle stream), the median
of --reps runs.  Kernel times: run under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rivulus_amd import capi  # noqa: E402
from rivulus_amd.capi import RV_INT64, Column, synth_spec  # noqa: E402

BATCH = 1024
WINDOW_ROWS = 1 << 28   # GpuHashJoinStream's defaults (rivulus_host.hpp)
MAX_PAIRS = 1 << 28


def timed(ctx, fn):
    ctx.synchronize()
    ctx.timer_start()
    r = fn()
    ms = ctx.timer_stop()
    return ms, r


def streamed(ctx, bcols, pcols):
    """(a): what GpuHashJoinStream does over a resident probe frame"""
    t = ctx.join_build(bcols[0])
    n = pcols[0].length
    at, pairs, batches = 0, 0, 0
    while at < n:
        length = min(n - at, WINDOW_ROWS)
        view = [c.slice(at, length) for c in pcols]
        outs, rows, _, total, taken = ctx.hash_join_chunked(t, bcols, 0, view, 0, BATCH, MAX_PAIRS)
        pairs += total
        batches += taken
        at += min(length, taken * BATCH)
        for o in outs:
            o.free()
    t.free()
    return pairs, batches


def per_batch_join(ctx, bcols, pcols, rows):
    pairs = 0
    for at in range(0, rows, BATCH):
        outs, r = ctx.hash_join(bcols, 0, [c.slice(at, min(BATCH, rows - at)) for c in pcols], 0)
        pairs += r
        for o in outs:
            o.free()
    return pairs


def per_batch_probe(ctx, bcols, pcols, rows):
    t = ctx.join_build(bcols[0])
    pairs = 0
    for at in range(0, rows, BATCH):
        key = pcols[0].slice(at, min(BATCH, rows - at))
        pi, bi, r = t.probe(key)
        outs = ctx.take_device([pcols[1].slice(at, min(BATCH, rows - at))], pi) + ctx.take_device([bcols[1]], bi)
        pairs += r
        for o in outs + [pi, bi]:
            o.free()
    t.free()
    return pairs


def shape(ctx, name, n_probe, n_keys, per_key, hit_share, reps, per_batch_rows):
    rng = np.random.default_rng(n_keys + per_key)
    bk = np.repeat(rng.permutation(n_keys).astype(np.int64), per_key)[rng.permutation(n_keys * per_key)]
    bcols = [ctx.upload(Column.from_numpy(bk)), ctx.upload(Column.from_numpy(np.arange(len(bk), dtype=np.int64)))]
    pcols = [ctx.generate(synth_spec(RV_INT64, seed=77, length=n_probe, modulus=int(round(n_keys / hit_share)))),
             ctx.generate(synth_spec(RV_INT64, seed=78, length=n_probe))]
    res = {"a": [], "b": [], "c": [], "cp": []}
    pairs = batches = 0
    for _ in range(reps):
        ms, (pairs, batches) = timed(ctx, lambda: streamed(ctx, bcols, pcols))
        res["a"].append(ms)
        ms, (outs, brows) = timed(ctx, lambda: ctx.hash_join(bcols, 0, pcols, 0))
        assert brows == pairs, (brows, pairs)
        res["b"].append(ms)
        for o in outs:
            o.free()
    c_rows = min(per_batch_rows, n_probe)
    ms, _ = timed(ctx, lambda: per_batch_join(ctx, bcols, pcols, c_rows))
    res["c"].append(ms * n_probe / c_rows)
    ms, _ = timed(ctx, lambda: per_batch_probe(ctx, bcols, pcols, c_rows))
    res["cp"].append(ms * n_probe / c_rows)
    med = {k: float(np.median(v)) for k, v in res.items()}
    line = {"shape": name, "probe_rows": n_probe, "batch_rows": BATCH, "batches": batches, "build_rows": n_keys * per_key, "keys": n_keys,
            "rows_per_key": per_key, "hit_share": hit_share, "pairs": pairs, "window_rows": WINDOW_ROWS, "max_pairs": MAX_PAIRS,
            "a_ms": round(med["a"], 3), "b_ms": round(med["b"], 3), "c_ms_extrap": round(med["c"], 1), "c_probe_ms_extrap": round(med["cp"], 1),
            "c_rows_timed": c_rows, "a_over_b": round(med["a"] / med["b"], 3), "c_over_a": round(med["c"] / med["a"], 1),
            "c_probe_over_a": round(med["cp"] / med["a"], 1), "reps": reps, "device": ctx.device_info()["name"]}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--probe-rows", type=int, default=10**8)
    ap.add_argument("--per-batch-rows", type=int, default=10**6, help="probe rows the per-batch alternatives (c) are timed over")
    args = ap.parse_args()
    n = args.probe_rows
    with capi.Context(0) as ctx:
        shape(ctx, "1e6_unique_10pct", n, 10**6, 1, 0.10, args.reps, args.per_batch_rows)
        shape(ctx, "1e6_unique_100pct", n, 10**6, 1, 1.00, args.reps, args.per_batch_rows)
        shape(ctx, "1e6_keys_x8_10pct", n, 10**6, 8, 0.10, args.reps, args.per_batch_rows)


if __name__ == "__main__":
    main()
