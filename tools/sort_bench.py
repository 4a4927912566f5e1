#!/usr/bin/env python3
"""Time rv_sort_indices against rocPRIM's pair sort and a device-to-device copy.

At 2^28 rows, by the context's timer (HIP events on the context's stream around the call), the median of CALLS calls after WARMUP
warm-ups, one key column per distribution:
    full random Int64; Int64 below 2^16; Int64 below 10; Float64 in [0, 1) with 5 % nulls; Int64 already sorted.
Every distribution runs under context option "sort_engine" 0 (the sort's own radix passes, which skip the digit positions all keys agree
on) and 1 (the pair sort through rocprim::radix_sort_pairs over all 64 bits; the key map, the null pass and the widening unchanged) in
the same process.  The ruler, on the same stream and timer: hipMemcpyAsync device-to-device over 16 bytes per row.  Per line: the
scatter passes engine 0 ran, the bytes per row the call moves by the derivation of K10 (20 for the map; 32 per value pass + 3 for its tile
counts through the scan, 4 less in the last pass, which writes no keys; 16 for the null pass; 12 for the widening when no pass runs), and
the rate that is.

    python tools/sort_bench.py [--rows N] [--out profiles/sort_bench.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rivulus_amd import capi  # noqa: E402
from rivulus_amd.capi import RV_FLOAT64, RV_INT64, synth_spec  # noqa: E402

WARMUP, CALLS = 2, 7
HIP_MEMCPY_DEVICE_TO_DEVICE = 3


def timed(ctx, fn, calls=CALLS):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(calls):
        ctx.timer_start()
        fn()
        ms.append(ctx.timer_stop())
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.rows
    lines = []
    with capi.Context(0) as ctx:
        info = ctx.device_info()
        device = " ".join(info["name"].split()) or "unnamed device"
        lines.append(f"# tools/sort_bench.py: rv_sort_indices, {n} rows, median of {CALLS} calls after {WARMUP} warm-ups, {device} ({info['compute_units']} CUs)")

        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        hip.hipMemcpyAsync.restype = C.c_int
        stream = capi.load().rv_ctx_stream(ctx.handle)
        scratch = [ctx.generate(synth_spec(RV_INT64, seed=s, length=n)) for s in (3, 4, 5, 6)]
        ptrs = [c.device_ptrs().values for c in scratch]

        def copy():
            assert hip.hipMemcpyAsync(ptrs[2], ptrs[0], n * 8, HIP_MEMCPY_DEVICE_TO_DEVICE, stream) == 0
            assert hip.hipMemcpyAsync(ptrs[3], ptrs[1], n * 8, HIP_MEMCPY_DEVICE_TO_DEVICE, stream) == 0

        copy_ms, lo, hi = timed(ctx, copy)
        lines.append(f"copy    device-to-device, 16 bytes per row                      {copy_ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})   {2 * n * 16 / copy_ms / 1e6:7.1f} GB/s of traffic   1.00 x the copy")
        for c in scratch:
            c.free()

        distributions = [
            ("random Int64, 64 bits", synth_spec(RV_INT64, seed=7, length=n, modulus=(1 << 64) - 1), False),
            ("Int64 below 2^16", synth_spec(RV_INT64, seed=7, length=n, modulus=1 << 16), False),
            ("Int64 below 10", synth_spec(RV_INT64, seed=7, length=n, modulus=10), False),
            ("Float64, 5 % nulls", synth_spec(RV_FLOAT64, seed=7, length=n, validity_seed=8, null_percent=5), True),
            ("Int64 already sorted", synth_spec(RV_INT64, seed=7, length=n, modulus=1 << 62, pattern="sorted"), False),
        ]
        for name, spec, nulls in distributions:
            key = ctx.generate(spec)
            result = {}
            for engine in (0, 1):
                ctx.set_option("sort_engine", engine)

                def call():
                    ctx.sort_indices(key).free()
                med, lo, hi = timed(ctx, call)
                result[engine] = med
                passes = ctx.get_option("sort_last_passes")
                note = ""
                if engine == 0:
                    value_passes = passes - (1 if nulls else 0)
                    per_row = 20 + 35 * value_passes + (16 if nulls else -4 if passes else 12)
                    note = f"   {passes} scatter passes, {per_row} bytes per row derived, {n * per_row / med / 1e6:7.1f} GB/s"
                lines.append(f"{name:<24} engine {engine}   {ctx.last_kernel():<40} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})   {med / copy_ms:7.2f} x the copy{note}")
            ctx.set_option("sort_engine", 0)
            ahead = "engine 0" if result[0] < result[1] else "engine 1 (rocPRIM)"
            lines.append(f"{'':<24} ahead: {ahead}, by {max(result.values()) / min(result.values()):.2f} x")
            key.free()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
