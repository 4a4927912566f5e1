#!/usr/bin/env python3
"""Time rv_top_k_indices against rv_sort_indices and a device-to-device copy.

By the context's timer (HIP events on the context's stream around the call), the median of CALLS calls after WARMUP warm-ups, one process.
At 2^28 rows, one key column per distribution:
    full random Int64; Int64 below 2^16; Int64 below 10 (heavy ties); Float64 in [0, 1) with 5 % nulls; Int64 already sorted,
each at k = 1, 100, 10^4 and 10^6, against rv_sort_indices over the same column in the same process.  The ruler, on the same stream and
timer: hipMemcpyAsync device-to-device of 8 bytes per row -- what ONE pass of the select over the key column reads.  Per line: the passes
over the key column the select ran (0: the whole sort ran), the candidates it sorted, and how far the call is from the sort in units of that
one pass ("behind by": the speed condition of K11 allows at most 1.00).

--sweep: rows from 2^10 to 2^28 at k = 100 over random Int64 with the select forced ("top_k_select_from_rows" = 1) against the whole sort
-- where the two cross is rvt::kTopKSelectFromRows -- and the refine divisor over {8, 32, 128} at 2^28 rows over keys whose
candidates fall between the three thresholds: Int64 below 3000 / 12000 (8.5 % / 2.1 % of the rows in the cut's bin, one byte left to sort)
and the largest Float64 cells in [0, 1) (3.1 %, six bytes left) (rvt::kTopKRefineDivisor).

    python tools/topk_bench.py [--rows N] [--sweep] [--out profiles/topk_bench.txt]
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
KS = (1, 100, 10 ** 4, 10 ** 6)


def timed(ctx, fn, calls=CALLS):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(calls):
        ctx.timer_start()
        fn()
        ms.append(ctx.timer_stop())
    return statistics.median(ms), min(ms), max(ms)


def distributions(n):
    return [
        ("random Int64, 64 bits", synth_spec(RV_INT64, seed=7, length=n, modulus=(1 << 64) - 1)),
        ("Int64 below 2^16", synth_spec(RV_INT64, seed=7, length=n, modulus=1 << 16)),
        ("Int64 below 10", synth_spec(RV_INT64, seed=7, length=n, modulus=10)),
        ("Float64, 5 % nulls", synth_spec(RV_FLOAT64, seed=7, length=n, validity_seed=8, null_percent=5)),
        ("Int64 already sorted", synth_spec(RV_INT64, seed=7, length=n, modulus=1 << 62, pattern="sorted")),
    ]


def copy_ruler(ctx, n):
    """(median, min, max) ms of a device-to-device copy of 8 bytes per row on the context's stream"""
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream = capi.load().rv_ctx_stream(ctx.handle)
    scratch = [ctx.generate(synth_spec(RV_INT64, seed=s, length=n)) for s in (3, 4)]
    ptrs = [c.device_ptrs().values for c in scratch]

    def copy():
        assert hip.hipMemcpyAsync(ptrs[1], ptrs[0], n * 8, HIP_MEMCPY_DEVICE_TO_DEVICE, stream) == 0

    result = timed(ctx, copy)
    for c in scratch:
        c.free()
    return result


def time_sort(ctx, key):
    return timed(ctx, lambda: ctx.sort_indices(key).free())


def time_top_k(ctx, key, k, flags=0):
    result = timed(ctx, lambda: ctx.top_k_indices(key, k, flags=flags).free())
    return result, ctx.get_option("top_k_last_passes"), ctx.get_option("top_k_last_candidates")


def shapes(ctx, n, lines):
    copy_ms, lo, hi = copy_ruler(ctx, n)
    lines.append(f"copy    device-to-device, 8 bytes per row: one pass over the key   {copy_ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})   {2 * n * 8 / copy_ms / 1e6:7.1f} GB/s of traffic")
    worst = None
    for name, spec in distributions(n):
        key = ctx.generate(spec)
        sort_ms, slo, shi = time_sort(ctx, key)
        lines.append(f"{name:<24} rv_sort_indices {'':<14} {sort_ms:9.3f} ms (min {slo:.3f}, max {shi:.3f})   {ctx.get_option('sort_last_passes')} scatter passes")
        for k in KS:
            (ms, lo, hi), passes, cands = time_top_k(ctx, key, k)
            behind = (ms - sort_ms) / copy_ms
            both_spreads = (hi - lo) + (shi - slo)
            verdict = "faster than the sort by more than both spreads" if sort_ms - ms > both_spreads else "within the spreads of the sort" if abs(sort_ms - ms) <= both_spreads else "slower than the sort"
            lines.append(f"{name:<24} rv_top_k_indices k = {k:<8} {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})   {passes} passes, {cands:>10} candidates   "
                         f"{sort_ms / ms:6.2f} x the sort   behind by {max(behind, 0.0):5.2f} passes   {verdict}")
            if worst is None or behind > worst[0]:
                worst = (behind, name, k)
        key.free()
    lines.append(f"# the (shape, k) furthest behind the sort: {worst[1]}, k = {worst[2]}: {worst[0]:.2f} passes of 8 bytes per row (the condition: at most 1.00)")


def sweep(ctx, lines):
    lines.append("# --sweep: k = 100 over random Int64, the select forced against the whole sort, by rows (sets rvt::kTopKSelectFromRows)")
    crossover = None
    for bits in range(10, 29):
        n = 1 << bits
        key = ctx.generate(synth_spec(RV_INT64, seed=7, length=n, modulus=(1 << 64) - 1))
        sort_ms, slo, shi = time_sort(ctx, key)
        ctx.set_option("top_k_select_from_rows", 1)
        (ms, lo, hi), passes, cands = time_top_k(ctx, key, 100)
        ctx.set_option("top_k_select_from_rows", 0)
        lines.append(f"rows 2^{bits:<3} sort {sort_ms:9.3f} ms (min {slo:.3f}, max {shi:.3f})   select {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})   "
                     f"{passes} passes, {cands:>8} candidates   select / sort {ms / sort_ms:5.2f}")
        if crossover is None and ms < sort_ms:
            crossover = bits
        key.free()
    lines.append(f"# the select is ahead from 2^{crossover} rows on")
    n = 1 << 28
    lines.append(f"# --sweep: the refine divisor at {n} rows (sets rvt::kTopKRefineDivisor)")
    # keys whose first pass leaves a bin of 8.5 % / 2.1 % of the rows with one more differing position below it: the divisors disagree there
    # ... and the largest of Float64 cells in [0, 1): nearly every cell shares the top byte, the next byte leaves 3.1 % of the rows, and those
    # candidates differ in all six bytes below -- the candidates whose sort costs what the derivation assumes
    refining = [("Int64 below 3000", synth_spec(RV_INT64, seed=7, length=n, modulus=3000), 0), ("Int64 below 12000", synth_spec(RV_INT64, seed=7, length=n, modulus=12000), 0),
                ("Float64 in [0, 1), desc.", synth_spec(RV_FLOAT64, seed=7, length=n), capi.RV_SORT_DESCENDING)]
    for name, spec, flags in refining:
        key = ctx.generate(spec)
        for k in (100, 10 ** 6):
            for divisor in (8, 32, 128):
                ctx.set_option("top_k_refine_divisor", divisor)
                (ms, lo, hi), passes, cands = time_top_k(ctx, key, k, flags)
                lines.append(f"{name:<24} k = {k:<8} divisor {divisor:<4} {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f})   {passes} passes, {cands:>10} candidates")
        ctx.set_option("top_k_refine_divisor", 0)
        key.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    with capi.Context(0) as ctx:
        info = ctx.device_info()
        device = " ".join(info["name"].split()) or "unnamed device"
        lines.append(f"# tools/topk_bench.py{' --sweep' if args.sweep else ''}: rv_top_k_indices, median of {CALLS} calls after {WARMUP} warm-ups, {device} ({info['compute_units']} CUs)")
        if args.sweep:
            sweep(ctx, lines)
        else:
            lines.append(f"# {args.rows} rows")
            shapes(ctx, args.rows, lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a" if args.sweep and os.path.exists(args.out) else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
