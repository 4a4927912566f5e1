#!/usr/bin/env python3
"""Time rv_window_frames against rv_window's CUM_SUM, the sort chain and a device-to-device copy.

At 2^28 rows, by the context's timer (HIP events on the context's stream around the call), the median of CALLS calls after WARMUP
warm-ups, one process:
    SUM(Int64) over the frames (7, 0), (1000, 1000) and (UNBOUNDED, UNBOUNDED), in place (no partition, no order);
    the same three under tools/window_bench.py's case (a): partition Int64 below 10^3, order key random 64-bit;
    AVG(Float64) over (6, 0) and MIN(Int64) over (63, 0), in place and under (a).
The rulers, in the same process on the same stream and timer: rv_window's CUM_SUM over the same input, the rv_sort_indices chain alone
over (a)'s keys, and hipMemcpyAsync device-to-device over 16 bytes per row.  Next to every call's time stands the kernel time of the
window's own passes (context option "profile_kernels": the call's kernel time less the chain's).

    python tools/window_frame_bench.py [--rows N] [--out profiles/window_frame_bench.txt]
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
U = None


def timed(ctx, fn, calls=CALLS):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(calls):
        ctx.timer_start()
        fn()
        ms.append(ctx.timer_stop())
    return statistics.median(ms), min(ms), max(ms)


def kernel_ms(ctx, fn, calls=CALLS):
    """median of the kernel time rv_ctx_kernel_stats reports for one call of fn (option profile_kernels)"""
    ctx.set_option("profile_kernels", 1)
    fn()
    ms = []
    for _ in range(calls):
        ctx.kernel_stats(reset=True)
        fn()
        ms.append(ctx.kernel_stats(reset=True)[0])
    ctx.set_option("profile_kernels", 0)
    return statistics.median(ms)


def frame_name(p, f):
    return "(" + ", ".join("UNBOUNDED" if v is None else str(v) for v in (p, f)) + ")"


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
        lines.append(f"# tools/window_frame_bench.py: rv_window_frames, {n} rows, median of {CALLS} calls after {WARMUP} warm-ups, {device} ({info['compute_units']} CUs)")

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
        lines.append(f"copy   device-to-device, 16 bytes per row                 {copy_ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})   {2 * n * 16 / copy_ms / 1e6:7.1f} GB/s of traffic   1.00 x the copy")
        for c in scratch:
            c.free()

        part = ctx.generate(synth_spec(RV_INT64, seed=11, length=n, modulus=1000))
        wide = ctx.generate(synth_spec(RV_INT64, seed=12, length=n, modulus=(1 << 64) - 1))
        value = ctx.generate(synth_spec(RV_INT64, seed=13, length=n, modulus=1000))
        fvalue = ctx.generate(synth_spec(RV_FLOAT64, seed=14, length=n))
        cols = [part, wide, value, fvalue]

        def chain():
            first = ctx.sort_indices(wide)
            ctx.sort_indices(part, prior=first).free()
            first.free()

        chain_ms, lo, hi = timed(ctx, chain)
        chain_kernel = kernel_ms(ctx, chain)
        lines.append(f"sort chain of (a): order key, then partition column       {chain_ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})   {chain_ms / copy_ms:7.2f} x the copy")

        frames = [(7, 0), (1000, 1000), (U, U)]
        exprs = [("CUM_SUM(Int64) through rv_window", None)] + [(f"SUM(Int64) over {frame_name(p, f)}", ("sum", 2, p, f)) for p, f in frames] + \
            [("AVG(Float64) over (6, 0)", ("avg", 3, 6, 0)), ("MIN(Int64) over (63, 0)", ("min", 2, 63, 0))]
        cum = {}
        for where, partition_by, order_by in (("in place", [], []), ("under (a)", [0], [(1, 0)])):
            for name, e in exprs:
                def call():
                    outs = ctx.window(cols, partition_by, order_by, [("cum_sum", 2)]) if e is None else ctx.window_frames(cols, partition_by, order_by, [e])
                    for c in outs:
                        c.free()

                med, lo, hi = timed(ctx, call)
                kernel = ctx.last_kernel()
                own = kernel_ms(ctx, call) - (chain_kernel if order_by else 0.0)
                if e is None:
                    cum[where] = (med, own)
                note = f"{med / cum[where][0]:5.2f} x CUM_SUM's call, own passes {own / cum[where][1]:5.2f} x CUM_SUM's"
                if order_by:
                    note += f"; the call is {med / chain_ms:.2f} x the chain"
                lines.append(f"{name + ', ' + where:<57} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})   {med / copy_ms:7.2f} x the copy   {kernel:<12} own passes {own:8.3f} ms   {note}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
