#!/usr/bin/env python3
"""Time the probe of every join kind against the inner join's and against a device copy.

At tools/join_bench.py's shapes -- 10^9 Int64 probe rows against 10^6 unique build keys, at 10 % and at 100 % hits -- and in one
process, on one build table per shape:
  inner        rv_join_probe
  kind=inner   rv_join_probe_kind(RV_JOIN_INNER)   (the same kernels through the new entry point)
  outer        RV_JOIN_PROBE_OUTER: every probe row, a null build index where it has no match
  full         RV_JOIN_FULL_OUTER: the same plus the marks, the build-row bitmap and the tail of unmatched build rows
  semi / anti  the probe index alone
Every line gives the rows out, the bytes of index output the call writes (16 per pair, 8 per row of a semi / anti join; validity
bitmaps included), the median time by the context's timer (HIP events on its stream around the whole call and nothing else: count
pass, scan, read-back, emit pass, and for outer / full the validity pass over the index columns; the outputs' null counts are read
and the outputs freed after the timer has stopped), that time over the inner join's, and the
time of hipMemcpyAsync device-to-device over as many bytes as the call writes, in the same process on the same stream and timer.
The copy is the yardstick, not the code under test: a kind whose time is a small multiple of its copy's is bound by its writes.

    python tools/outer_join_bench.py [--probe-rows N] [--out profiles/outer_join_bench.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rivulus_amd import capi  # noqa: E402
from rivulus_amd.capi import (RV_INT64, RV_JOIN_FULL_OUTER, RV_JOIN_INNER, RV_JOIN_PROBE_ANTI, RV_JOIN_PROBE_OUTER,  # noqa: E402
                              RV_JOIN_PROBE_SEMI, Column, synth_spec)

WARMUP, CALLS = 2, 7
HIP_MEMCPY_DEVICE_TO_DEVICE = 3
KINDS = [("inner", None), ("kind=inner", RV_JOIN_INNER), ("outer", RV_JOIN_PROBE_OUTER), ("full", RV_JOIN_FULL_OUTER),
         ("semi", RV_JOIN_PROBE_SEMI), ("anti", RV_JOIN_PROBE_ANTI)]


def timed(ctx, fn):
    """fn() is timed; what it returns, if callable, runs after the timer has stopped (reading counts, freeing outputs)."""
    ms = []
    for k in range(WARMUP + CALLS):
        ctx.synchronize()
        ctx.timer_start()
        after = fn()
        t = ctx.timer_stop()
        if callable(after):
            after()
        if k >= WARMUP:
            ms.append(t)
    return statistics.median(ms), min(ms), max(ms)


def written_bytes(kind, rows, nulls):
    """Index output of one probe: 8 bytes per row and column, plus a validity word per 64 rows of a column that has a null."""
    cols = 1 if kind in (RV_JOIN_PROBE_SEMI, RV_JOIN_PROBE_ANTI) else 2
    return rows * 8 * cols + sum((rows + 63) // 64 * 8 for z in nulls if z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probe-rows", type=int, default=10**9)
    ap.add_argument("--keys", type=int, default=10**6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, n_keys = args.probe_rows, args.keys
    lines = []
    with capi.Context(0) as ctx:
        info = ctx.device_info()
        device = " ".join(info["name"].split()) or "unnamed device"
        lines.append(f"# tools/outer_join_bench.py: {n} probe rows against {n_keys} unique Int64 keys, median of {CALLS} calls after {WARMUP} warm-ups, "
                     f"{device} ({info['compute_units']} CUs)")
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        hip.hipMemcpyAsync.restype = C.c_int
        stream = capi.load().rv_ctx_stream(ctx.handle)
        # the copy's two buffers: as large as the largest output (every probe row once, two index columns, two bitmaps)
        most = 2 * (n + n_keys) * 8 + 2 * ((n + n_keys + 63) // 64 * 8)
        src = ctx.generate(synth_spec(RV_INT64, seed=5, length=most // 8 + 1))
        dst = ctx.generate(synth_spec(RV_INT64, seed=6, length=most // 8 + 1))
        sp, dp = src.device_ptrs().values, dst.device_ptrs().values
        rng = np.random.default_rng(n_keys + 1)
        build_key = ctx.upload(Column.from_numpy(rng.permutation(n_keys).astype(np.int64)))
        for hit_share in (0.10, 1.00):
            probe_key = ctx.generate(synth_spec(RV_INT64, seed=77, length=n, modulus=int(round(n_keys / hit_share))))
            table = ctx.join_build(build_key)
            lines.append(f"## {int(hit_share * 100)} % of the probe rows hit")
            inner_ms = None
            for name, kind in KINDS:
                shape = {}

                def call():
                    pi, bi, rows = table.probe(probe_key, kind)

                    def after():  # outside the timed window
                        shape["rows"] = rows
                        shape["nulls"] = [pi.null_count(), bi.null_count() if bi is not None else 0]
                        pi.free()
                        if bi is not None:
                            bi.free()
                    return after

                med, lo, hi = timed(ctx, call)
                kernel = ctx.last_kernel()
                if inner_ms is None:
                    inner_ms = med
                nbytes = written_bytes(kind, shape["rows"], shape["nulls"])

                def copy():
                    assert hip.hipMemcpyAsync(dp, sp, nbytes, HIP_MEMCPY_DEVICE_TO_DEVICE, stream) == 0

                cmed, _, _ = timed(ctx, copy) if nbytes else (0.0, 0.0, 0.0)
                ratio = f"{med / cmed:6.1f} x its copy" if cmed else "   no output"
                lines.append(f"{name:<11} {kernel:<24} rows {shape['rows']:>11}  writes {nbytes / 1e9:7.3f} GB   {med:8.3f} ms (min {lo:.3f}, max {hi:.3f})   "
                             f"{med / inner_ms:5.2f} x inner   copy of the bytes {cmed:7.3f} ms   {ratio}")
            table.free()
            probe_key.free()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
