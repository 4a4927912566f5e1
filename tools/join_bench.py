#!/usr/bin/env python3
"""Inner hash join on the device: one JSON line per shape (tools/README.md).

  build_ms     rv_join_build (classify, stable radix sort, slot insert; host round trips included)
  probe_ms     rv_join_probe: count pass + tile scan + one read-back + emit pass
  gather_ms    rv_take_device of one Int64 probe payload by probe_idx and one Int64 build payload by build_idx (this call's
               bounds pre-pass included; rv_hash_join's own gather skips it)
  join_ms      rv_hash_join end to end over (key, payload) on both sides
  rows         pairs out
  probe_gbs    the probe's compulsory HBM traffic -- the probe keys read twice (count and emit: 16 B / probe row) + the two
               index outputs (16 B / pair) -- over probe_ms, and as a share of the 8 TB/s peak (table lookups not counted)
All times are wall clock around the call on an idle stream (HIP events), the median of --reps runs.  Kernel times: run
under `rocprofv3 --kernel-trace --stats` (profiles/r06_join_kernel_stats.csv)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rivulus_amd import capi  # noqa: E402
from rivulus_amd.capi import RV_INT64, Column, synth_spec  # noqa: E402

PEAK = 8.0e12


def timed(ctx, fn):
    ctx.synchronize()
    ctx.timer_start()
    r = fn()
    ms = ctx.timer_stop()
    return ms, r


def shape(ctx, name, n_probe, n_keys, per_key, hit_share, reps):
    rng = np.random.default_rng(n_keys + per_key)
    bk = np.repeat(rng.permutation(n_keys).astype(np.int64), per_key)[rng.permutation(n_keys * per_key)]
    build_key = ctx.upload(Column.from_numpy(bk))
    build_pay = ctx.upload(Column.from_numpy(np.arange(len(bk), dtype=np.int64)))
    # probe keys uniform over n_keys / hit_share values: hit_share of them are build keys
    probe_key = ctx.generate(synth_spec(RV_INT64, seed=77, length=n_probe, modulus=int(round(n_keys / hit_share))))
    probe_pay = ctx.generate(synth_spec(RV_INT64, seed=78, length=n_probe))
    res = {"build": [], "probe": [], "gather": [], "join": []}
    rows = 0
    for _ in range(reps):
        ms, t = timed(ctx, lambda: ctx.join_build(build_key))
        res["build"].append(ms)
        ms, (pi, bi, rows) = timed(ctx, lambda: t.probe(probe_key))
        res["probe"].append(ms)
        ms, outs = timed(ctx, lambda: ctx.take_device([probe_pay], pi) + ctx.take_device([build_pay], bi))
        res["gather"].append(ms)
        for o in outs:
            o.free()
        pi.free(), bi.free(), t.free()
        ms, (outs, jrows) = timed(ctx, lambda: ctx.hash_join([build_key, build_pay], 0, [probe_key, probe_pay], 0))
        assert jrows == rows
        res["join"].append(ms)
        for o in outs:
            o.free()
    med = {k: float(np.median(v)) for k, v in res.items()}
    gbs = (16 * n_probe + 16 * rows) / (med["probe"] * 1e-3) / 1e9
    line = {"shape": name, "probe_rows": n_probe, "build_rows": n_keys * per_key, "keys": n_keys, "rows_per_key": per_key,
            "hit_share": hit_share, "rows": rows, "build_ms": round(med["build"], 3), "probe_ms": round(med["probe"], 3),
            "gather_ms": round(med["gather"], 3), "join_ms": round(med["join"], 3), "probe_gbs": round(gbs, 1),
            "probe_of_peak": round(gbs * 1e9 / PEAK, 3), "reps": reps, "device": ctx.device_info()["name"]}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--probe-rows", type=int, default=10**9)
    args = ap.parse_args()
    n = args.probe_rows
    with capi.Context(0) as ctx:
        shape(ctx, "1e6_unique_10pct", n, 10**6, 1, 0.10, args.reps)
        shape(ctx, "1e6_unique_100pct", n, 10**6, 1, 1.00, args.reps)
        shape(ctx, "1e7_unique_10pct", n, 10**7, 1, 0.10, args.reps)
        shape(ctx, "1e7_unique_100pct", n, 10**7, 1, 1.00, args.reps)
        shape(ctx, "1e6_keys_x8_10pct", n, 10**6, 8, 0.10, args.reps)


if __name__ == "__main__":
    main()
