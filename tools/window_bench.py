#!/usr/bin/env python3
"""Time rv_window against the sort chain it runs on top of and a device-to-device copy.

At 2^28 rows, by the context's timer (HIP events on the context's stream around the call), the median of CALLS calls after WARMUP
warm-ups, one process:
    (a) ROW_NUMBER + CUM_SUM(Int64), partition Int64 below 10^3, order key random 64-bit;
    (b) the same with the order key below 2^16;
    (c) the same expressions with no partition and no order: the in-place path, no sort and no gather;
    (d) LAG(1) of the Int64 column under (a).
The rulers, in the same process on the same stream and timer: the rv_sort_indices chain alone over the same keys (the order key, then the
partition column: what the window adds on top of ORDER BY is the difference), and hipMemcpyAsync device-to-device over 16 bytes per row.
A second round under context option "profile_kernels" reads rv_ctx_kernel_stats: the sorts time themselves there and rv_window adds its
own passes (heads, scans, shifts -- not the partition ids, not the final gather of a shift), so the call's kernel time less the chain's is
the time of the window's own passes; it is printed with the bytes per row those passes move by the derivation of K12 and the rate that is.

    python tools/window_bench.py [--rows N] [--out profiles/window_bench.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rivulus_amd import capi  # noqa: E402
from rivulus_amd.capi import RV_INT64, synth_spec  # noqa: E402

WARMUP, CALLS = 2, 7
HIP_MEMCPY_DEVICE_TO_DEVICE = 3
# bytes per row of the window's own passes, as K12 derives them (8-byte perm, ids, cells; the two head bitmaps are 2 bits):
HEADS = 8 + 16 + 16          # perm, the ids at perm[j] and perm[j - 1], the order cells at both rows
HEADS_IN_PLACE = 0           # no perm, no ids, no order key: two bits written
SCAN_NUMBER = 8 + 8          # apply: perm, the store at out[perm[j]] (tile_agg reads the head bits only)
SCAN_SUM = (8 + 8) * 2 + 8   # tile_agg and apply: perm + the cell at perm[j]; apply: the store
SCAN_NUMBER_IN_PLACE = 8     # the store
SCAN_SUM_IN_PLACE = 8 * 2 + 8
SHIFT = 8 + 16 + 8           # perm (its neighbour is the next lane's), the ids at both rows, the store at idx[perm[j]]


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
        lines.append(f"# tools/window_bench.py: rv_window, {n} rows, median of {CALLS} calls after {WARMUP} warm-ups, {device} ({info['compute_units']} CUs)")

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
        lines.append(f"copy   device-to-device, 16 bytes per row                         {copy_ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})   {2 * n * 16 / copy_ms / 1e6:7.1f} GB/s of traffic   1.00 x the copy")
        for c in scratch:
            c.free()

        part = ctx.generate(synth_spec(RV_INT64, seed=11, length=n, modulus=1000))
        wide = ctx.generate(synth_spec(RV_INT64, seed=12, length=n, modulus=(1 << 64) - 1))
        narrow = ctx.generate(synth_spec(RV_INT64, seed=12, length=n, modulus=1 << 16))
        value = ctx.generate(synth_spec(RV_INT64, seed=13, length=n, modulus=1000))
        number_and_sum = [("row_number", 0), ("cum_sum", 3)]
        cases = [
            ("(a) ROW_NUMBER + CUM_SUM, 64-bit order key", [0], [(1, 0)], number_and_sum, wide, HEADS + SCAN_NUMBER + SCAN_SUM),
            ("(b) ROW_NUMBER + CUM_SUM, order key < 2^16", [0], [(2, 0)], number_and_sum, narrow, HEADS + SCAN_NUMBER + SCAN_SUM),
            ("(c) ROW_NUMBER + CUM_SUM, in place", [], [], number_and_sum, None, HEADS_IN_PLACE + SCAN_NUMBER_IN_PLACE + SCAN_SUM_IN_PLACE),
            ("(d) LAG(1), 64-bit order key", [0], [(1, 0)], [("lag", 3, 1)], wide, SHIFT),
        ]
        cols = [part, wide, narrow, value]
        for name, partition_by, order_by, exprs, order_key, per_row in cases:
            def call():
                for c in ctx.window(cols, partition_by, order_by, exprs):
                    c.free()

            def chain():
                if order_key is None:
                    return
                first = ctx.sort_indices(order_key)
                ctx.sort_indices(part, prior=first).free()
                first.free()

            med, lo, hi = timed(ctx, call)
            kernel = ctx.last_kernel()
            lines.append(f"{name:<46} {kernel:<13} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})   {med / copy_ms:7.2f} x the copy")
            chain_ms = 0.0
            if order_key is not None:
                chain_ms, lo, hi = timed(ctx, chain)
                lines.append(f"{'':<46} {'sort chain':<13} {chain_ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})   {chain_ms / copy_ms:7.2f} x the copy; the window is {med / chain_ms:.2f} x the chain")
            own = kernel_ms(ctx, call) - (kernel_ms(ctx, chain) if order_key is not None else 0.0)
            lines.append(f"{'':<46} {'own passes':<13} {own:9.3f} ms of kernel time   {per_row} bytes per row derived, {n * per_row / own / 1e6:7.1f} GB/s"
                         f"   (the rest of the call: partition ids, the gather of a shift, waits: {med - chain_ms - own:.3f} ms)")
        # the passes of (a) apart: own(ROW_NUMBER) = heads + number scan, own(CUM_SUM) = heads + sum scan, own(both) = all three
        def own_of(exprs, partition_by, order_by):
            def call():
                for c in ctx.window(cols, partition_by, order_by, exprs):
                    c.free()

            def chain():
                first = ctx.sort_indices(wide)
                ctx.sort_indices(part, prior=first).free()
                first.free()
            return kernel_ms(ctx, call) - (kernel_ms(ctx, chain) if order_by else 0.0)

        for label, by, order, heads, number, total in (("(a)", [0], [(1, 0)], HEADS, SCAN_NUMBER, SCAN_SUM),
                                                       ("(c)", [], [], HEADS_IN_PLACE, SCAN_NUMBER_IN_PLACE, SCAN_SUM_IN_PLACE)):
            both, num, tot = own_of(number_and_sum, by, order), own_of(number_and_sum[:1], by, order), own_of(number_and_sum[1:], by, order)
            h, s_num, s_sum = num + tot - both, both - tot, both - num
            rate = lambda b, ms: f"{n * b / ms / 1e6:7.1f} GB/s" if b and ms > 0 else "      - "
            lines.append(f"passes of {label} by differences of kernel time: window_heads {h:7.3f} ms ({heads} B/row, {rate(heads, h)}), "
                         f"scan of ROW_NUMBER {s_num:7.3f} ms ({number} B/row, {rate(number, s_num)}), scan of CUM_SUM {s_sum:7.3f} ms ({total} B/row, {rate(total, s_sum)})")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
