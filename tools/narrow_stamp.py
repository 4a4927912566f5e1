"""Diagnostic: per-phase cycle shares of the pass over narrow codes (the FF_STAMP | FF_NARROW16 instantiations, fused_narrow.hip) on
the headline shape, x > 899 -> [x] over 1e9 resident Int64 rows.  Shares only: a stamped build's run time is never quoted.
    python3 tools/narrow_stamp.py [rows] [--packed]   (RIVULUS_GPU_LIB=<other build> for a before / after on one box)
Per geometry (32 and 16 rows per lane, 16 waves; --packed: the packed 10-bit codes under option narrow_codes = 2, 48 and 24 rows per lane)
and ablation (option "debug": 1 = no output stores, 2 = no look-back) it prints wave 1's cycles per tile by phase and their shares:
    wait     the tile's codes are not there yet when the wave wants to evaluate them (part of eval)
    eval     unpack, compare, rank, stage (without the wait)
    barrier  from the end of the wave's own work to behind the tile's one barrier: waiting for the slowest wave
    publish  wave totals -> prefix, aggregate published, per-batch counts (wave 0 also resolves the output offset before the barrier)
    flush    the pending tile's staged survivors written out
The library prints the sums on stderr ("[stamp] ..."); each form runs in a child process whose stderr is read here."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if len(sys.argv) > 1 and sys.argv[1] == "--child":
    sys.path.insert(0, ROOT)
    from rivulus_amd import capi
    from rivulus_amd.capi import RV_INT64, Predicate, Term, synth_spec
    n, r, debug, mode = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    ctx = capi.Context(0)
    ctx.set_option("narrow_codes", mode)
    x = ctx.generate(synth_spec(RV_INT64, seed=42, length=n))
    pred = Predicate([Term(0, ">", 899)])
    for _ in range(3):  # the scan that packs, then passes over codes
        outs, rows, _ = ctx.filter_project([x], pred, [0])
        [o.free() for o in outs]
    ctx.set_option("rows_per_lane", r | (16 << 8))
    ctx.set_option("vec", 2)
    ctx.set_option("debug", debug)
    ctx.set_option("stamp", 1)
    outs, rows, _ = ctx.filter_project([x], pred, [0])
    print("kernel", ctx.last_kernel(), flush=True)
    sys.exit(0)

args = [a for a in sys.argv[1:] if a != "--packed"]
packed = "--packed" in sys.argv[1:]
n = int(args[0]) if args else 1_000_000_000
print(f"library: {os.environ.get('RIVULUS_GPU_LIB', 'the tree')}; {n} rows, x > 899 -> [x]; {'packed 10-bit codes' if packed else '2-byte codes'}")
for r in ((48, 24) if packed else (32, 16)):
    for debug, label in ((0, "as it runs"), (1, "no output stores"), (2, "no look-back")):
        # one form per process, each under its own time limit; the first that fails ends the run: nothing more is started on that card
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(r), str(debug), "2" if packed else "1"], capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            sys.exit(f"R={r} debug={debug}: no answer within 120 s; stopped")
        kernel = [q for q in p.stdout.splitlines() if q.startswith("kernel ")]
        wave1 = [q for q in p.stderr.splitlines() if q.startswith("[stamp] wave1 cycles/tile: eval")]
        wait = [q for q in p.stderr.splitlines() if q.startswith("[stamp] wave1 cycles/tile: of eval")]
        if p.returncode != 0 or not kernel or not wave1 or not wait:
            sys.exit(f"R={r} debug={debug}: exit status {p.returncode}, no stamps; stopped ({p.stderr[-300:]})")
        ev, barrier, publish, _, flush = (float(v) for v in re.findall(r"(?:wait\)|prefetch|lookback|barrierB|flush) (\d+)", wave1[-1]))
        w = float(re.search(r"load wait (\d+)", wait[-1]).group(1))
        tiles = int(re.search(r"tiles (\d+)", wave1[-1]).group(1))
        total = ev + barrier + publish + flush
        parts = (("wait", w), ("eval", ev - w), ("barrier", barrier), ("publish", publish), ("flush", flush))
        print(f"{kernel[-1].split()[1]} ({label}): {total:.0f} cycles/tile over {tiles} tiles of wave 1 | " +
              " | ".join(f"{k} {v:.0f} ({100 * v / total:.0f} %)" for k, v in parts), flush=True)
