#!/usr/bin/env python3
"""Time rv_hash_aggregate_keys against the packed single key and a device-to-device copy.

At 2^28 rows and one Int64 value column, `SUM + COUNT_ROWS`, by the context's timer (HIP events on the context's stream around the
call), the median of CALLS calls after WARMUP warm-ups each, all in one process on one stream:
  (a) two Int64 keys below 2^16 each, uniform at random, through rv_hash_aggregate_keys, at 10, 10^3 and 10^6 distinct tuples;
  (b) the same grouping through rv_hash_aggregate on the packed key a << 32 | b: what the single-key entry point can do for keys that
      small, and the yardstick of (a);
  (c) one Float64 key (10^3 values, halves) through rv_hash_aggregate_keys: the one-column instantiation of the tuple passes;
  (d) hipMemcpyAsync device-to-device over 16 bytes per row, the copy the other tools of this directory measure against.
Per group count the file reports (a) / (b) and (a) / (d).  The accumulate stage is the same code behind (a) and (b) (its time is listed:
rv_ctx_kernel_stats under option "profile_kernels"); what differs is the three passes in front of it, which read 8 x nkeys bytes per
row where (b) reads 8 and follow every slot they compare to nkeys cells instead of one.

    python tools/group_keys_bench.py [--rows N] [--out profiles/group_keys_bench.txt]
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
SPECS = [("sum", 0), ("count_rows", None)]
SHAPES = {10: (5, 2), 1000: (40, 25), 10 ** 6: (1000, 1000)}  # distinct tuples: values of a x values of b


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
        lines.append(f"# tools/group_keys_bench.py: {n} rows, SUM + COUNT_ROWS over one Int64 column, median of {CALLS} calls after {WARMUP} warm-ups, "
                     f"{device} ({info['compute_units']} CUs)")
        value = ctx.generate(synth_spec(RV_INT64, seed=1, length=n, modulus=1000))

        # (d) the yardstick: 16 bytes per row copied by the runtime (two columns' worth, out of and into scratch columns)
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
        lines.append(f"(d) copy    device-to-device, 16 bytes per row                                     {copy_ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})   "
                     f"{2 * n * 16 / copy_ms / 1e6:7.1f} GB/s of traffic")
        for c in scratch:
            c.free()

        def report(tag, name, aggregate, ids):
            """aggregate(want_first_row) makes one call; ids() the group-id entry point of the same keys"""
            def call():
                outs, first, _ = aggregate(True)
                for o in outs + [first]:
                    o.free()
            med, lo, hi = timed(ctx, call)
            kernel = ctx.last_kernel()
            ctx.set_option("profile_kernels", 1)
            ctx.kernel_stats(reset=True)
            for _ in range(3):
                call()
            stage_ms, _launches = ctx.kernel_stats(reset=True)
            ctx.set_option("profile_kernels", 0)
            outs, _, groups = aggregate(False)
            for o in outs:
                o.free()
            gids, first, _ = ids()
            passes = ctx.last_kernel()
            gids.free()
            first.free()
            lines.append(f"{tag} {name:<26} G = {groups:<8} {passes:<16} {kernel:<26} call {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})   "
                         f"accumulate stage {stage_ms / 3:8.3f} ms   in front of it {med - stage_ms / 3:8.3f} ms   {med / copy_ms:6.2f} x (d)")
            return med

        ratios = []
        for groups, (na, nb) in SHAPES.items():
            a = ctx.generate(synth_spec(RV_INT64, seed=7, length=n, modulus=na))
            b = ctx.generate(synth_spec(RV_INT64, seed=8, length=n, modulus=nb))
            packed = ctx.eval_arith([a, b], ("+", ("*", ("col", 0), ("lit", 1 << 32)), ("col", 1)))
            t_a = report("(a)", f"two Int64 keys, {na} x {nb}", lambda first: ctx.hash_aggregate_keys([a, b], [value], SPECS, want_first_row=first),
                         lambda: ctx.group_ids_keys([a, b]))
            t_b = report("(b)", "packed key a << 32 | b", lambda first: ctx.hash_aggregate(packed, [value], SPECS, want_first_row=first),
                         lambda: ctx.group_ids(packed))
            ratios.append((groups, t_a, t_b))
            if groups == 1000:
                fkey = ctx.eval_arith([packed], ("*", ("col", 0), ("lit", 0.5)))
                report("(c)", "one Float64 key", lambda first: ctx.hash_aggregate_keys([fkey], [value], SPECS, want_first_row=first),
                       lambda: ctx.group_ids_keys([fkey]))
                fkey.free()
            for c in (a, b, packed):
                c.free()
        lines.append("# distinct tuples   (a) / (b)   (a) / (d)")
        for groups, t_a, t_b in ratios:
            lines.append(f"ratio G = {groups:<10} {t_a / t_b:6.2f}      {t_a / copy_ms:6.2f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
