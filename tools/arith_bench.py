#!/usr/bin/env python3
"""Time rv_eval_arith against a device-to-device copy.

At 2^28 rows, by the context's timer (HIP events on the context's stream around the call), 20 calls after 3 warm-ups each:
  a + b      Int64, no nulls
  a * b + c  Float64, 5 % nulls on two of the inputs
  a / b      Int64, both operands in [0, 1000) (b has zeros: those cells are null): the compiled division sees two zero high
             words and takes its 32-bit path
  a / b      Int64, both operands spread over [-2^62, 2^62): the full 64-bit division sequence on every lane
and, in the same process and on the same stream and timer, hipMemcpyAsync device-to-device over one 2^28-row column.  The copy is
the yardstick, not the code under test.  Every line gives the HBM traffic of one call (bytes read + bytes written, bitmaps
included), its median time, the traffic rate, and that rate as a share of the copy's.

    python tools/arith_bench.py [--rows N] [--out profiles/arith_bench.txt]
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

WARMUP, CALLS = 3, 20
HIP_MEMCPY_DEVICE_TO_DEVICE = 3


def timed(ctx, fn):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(CALLS):
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
        lines.append(f"# tools/arith_bench.py: {n} rows, median of {CALLS} calls after {WARMUP} warm-ups, {device} ({info['compute_units']} CUs)")
        ia = ctx.generate(synth_spec(RV_INT64, seed=1, length=n))
        ib = ctx.generate(synth_spec(RV_INT64, seed=2, length=n))

        # the yardstick: one column copied onto another by the runtime
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        hip.hipMemcpyAsync.restype = C.c_int
        stream = capi.load().rv_ctx_stream(ctx.handle)
        src, dst = ia.device_ptrs().values, ib.device_ptrs().values

        def copy():
            assert hip.hipMemcpyAsync(dst, src, n * 8, HIP_MEMCPY_DEVICE_TO_DEVICE, stream) == 0

        med, lo, hi = timed(ctx, copy)
        copy_rate = 2 * n * 8 / med / 1e6  # GB/s of traffic: every byte is read and written
        lines.append(f"copy   device-to-device, {n * 8} bytes   traffic {2 * n * 8 / 1e9:7.3f} GB   {med:7.3f} ms (min {lo:.3f}, max {hi:.3f})   {copy_rate:7.1f} GB/s   1.00 of the copy")
        ib.free()
        ib = ctx.generate(synth_spec(RV_INT64, seed=2, length=n))  # the copy overwrote it

        def report(name, cols, tree, traffic):
            def call():
                ctx.eval_arith(cols, tree).free()
            med, lo, hi = timed(ctx, call)
            rate = traffic / med / 1e6
            lines.append(f"{name:<16} {ctx.last_kernel():<16} traffic {traffic / 1e9:7.3f} GB   {med:7.3f} ms (min {lo:.3f}, max {hi:.3f})   {rate:7.1f} GB/s   "
                         f"{rate / copy_rate:.2f} of the copy")

        bitmap = (n + 63) // 64 * 8
        report("a + b", [ia, ib], ("+", ("col", 0), ("col", 1)), 3 * n * 8)
        report("a / b  small", [ia, ib], ("/", ("col", 0), ("col", 1)), 3 * n * 8 + bitmap)
        ia.free()
        ib.free()
        # operands of both signs with their high words in use: generated in [0, 2^63), moved down by 2^62 (on the device, by the
        # code under test: `x - 2^62`)
        wide = []
        for seed in (6, 7):
            raw = ctx.generate(synth_spec(RV_INT64, seed=seed, length=n, modulus=1 << 63))
            wide.append(ctx.eval_arith([raw], ("-", ("col", 0), ("lit", 1 << 62))))
            raw.free()
        report("a / b  wide", wide, ("/", ("col", 0), ("col", 1)), 3 * n * 8 + bitmap)
        for c in wide:
            c.free()
        fa = ctx.generate(synth_spec(RV_FLOAT64, seed=3, length=n, validity_seed=13, null_percent=5))
        fb = ctx.generate(synth_spec(RV_FLOAT64, seed=4, length=n, validity_seed=14, null_percent=5))
        fc = ctx.generate(synth_spec(RV_FLOAT64, seed=5, length=n))
        report("a * b + c", [fa, fb, fc], ("+", ("*", ("col", 0), ("col", 1)), ("col", 2)), 4 * n * 8 + 3 * bitmap)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
