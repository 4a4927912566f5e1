#!/usr/bin/env python3
"""Time rv_hash_aggregate against a device-to-device copy.

At 2^28 rows, an Int64 key uniform at random over G values and one Int64 value column, `SUM + COUNT_ROWS`, for G = 10, 10^3, 10^6
and 10^8, plus one run with the keys sorted (G = 10^3), by the context's timer (HIP events on the context's stream around the call),
the median of CALLS calls after WARMUP warm-ups each.  Per configuration: the whole call, and the accumulate stage alone
(rv_ctx_kernel_stats under option "profile_kernels", in a second set of calls); the Float64 SUM path is timed on its own at G = 10^3
(one Float64 value column, `SUM`: the stage is then the sort of (group id, row) and the segmented sum).  In the same process, on the
same stream and timer: hipMemcpyAsync device-to-device over 16 bytes per row, the yardstick (key + value read once is the least any
group-by reads).  --sweep adds G on either side of rvt::kGroupAggLdsGroupsMost: the two forms of the accumulate kernel are picked by
G alone, so the sweep times each form where it is used -- a step at the switch would say the switch sits in the wrong place.

    python tools/group_agg_bench.py [--rows N] [--sweep] [--out profiles/group_agg_bench.txt]
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
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.rows
    lines = []
    with capi.Context(0) as ctx:
        info = ctx.device_info()
        device = " ".join(info["name"].split()) or "unnamed device"
        lines.append(f"# tools/group_agg_bench.py: {n} rows, median of {CALLS} calls after {WARMUP} warm-ups, {device} ({info['compute_units']} CUs)")
        value = ctx.generate(synth_spec(RV_INT64, seed=1, length=n, modulus=1000))
        fvalue = ctx.generate(synth_spec(RV_FLOAT64, seed=2, length=n))

        # the yardstick: 16 bytes per row copied by the runtime (two columns' worth, out of and into scratch columns)
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
        lines.append(f"copy    device-to-device, 16 bytes per row                        {copy_ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})   {2 * n * 16 / copy_ms / 1e6:7.1f} GB/s of traffic   1.00 x the copy")
        for c in scratch:
            c.free()

        def report(name, key, cols, specs, calls=CALLS):
            def call():
                outs, first, _ = ctx.hash_aggregate(key, cols, specs)
                for o in outs + [first]:
                    o.free()
            med, lo, hi = timed(ctx, call, calls)
            kernel = ctx.last_kernel()
            ctx.set_option("profile_kernels", 1)
            ctx.kernel_stats(reset=True)
            for _ in range(3):
                call()
            stage_ms, _launches = ctx.kernel_stats(reset=True)
            ctx.set_option("profile_kernels", 0)
            _, _, groups = ctx.hash_aggregate(key, cols, specs, want_first_row=False)
            lines.append(f"{name:<22} G = {groups:<10} {kernel:<40} call {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})   {med / copy_ms:6.2f} x the copy   "
                         f"accumulate stage {stage_ms / 3:9.3f} ms   {stage_ms / 3 / copy_ms:6.2f} x the copy")

        int_specs = [("sum", 0), ("count_rows", None)]
        for groups in (10, 1000, 10 ** 6, 10 ** 8):
            if groups > n:
                continue
            key = ctx.generate(synth_spec(RV_INT64, seed=7, length=n, modulus=groups))
            ctx.set_option("agg_max_groups", groups if groups > 1 << 26 else 0)  # G = 10^8 is past the default limit of 2^26 groups
            report("uniform keys", key, [value], int_specs)
            ctx.set_option("agg_max_groups", 0)
            if groups == 1000:
                report("uniform keys, f64 SUM", key, [fvalue], [("sum", 0)], calls=3)
            key.free()
        key = ctx.generate(synth_spec(RV_INT64, seed=7, length=n, modulus=1000, pattern="sorted"))
        report("sorted keys", key, [value], int_specs)
        key.free()
        if args.sweep:
            lines.append("# G across the LDS / global switch (rvt::kGroupAggLdsGroupsMost), uniform keys, SUM + COUNT_ROWS")
            for groups in (64, 512, 1024, 2048, 4096, 4097, 8192, 8193, 16384, 16385, 65536):
                key = ctx.generate(synth_spec(RV_INT64, seed=7, length=n, modulus=groups))
                report("uniform keys", key, [value], int_specs, calls=3)
                key.free()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
