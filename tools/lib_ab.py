"""The headline pass (x > 899 -> [x], 1e9 rows) and config 3 under TWO BUILDS of the library on one box, alternating processes (boxes
differ by +- 3 %, so a before / after needs the same box): kernel time by HIP events and wall per call.
    python3 tools/lib_ab.py tools/_ab/librivulus_gpu_r04.so [rounds] [config2|all|plain|calls] [other|tree]
(the other build: the tree's own; `plain`: config 2 with option narrow_codes = -1, the plain lean pass whatever the column's companion;
`calls`: one small call per pipeline breaker, 1024 rows, where the host path is the whole time -- microseconds per call, and after the
rounds each build's median and range per operator; last argument: the build that goes first in every round)
A build of another commit: `git worktree add X <commit>; make -C X/rivulus_amd/csrc; cp X/rivulus_amd/csrc/librivulus_gpu.so tools/_ab/`."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if len(sys.argv) > 1 and sys.argv[1] == "--child":
    sys.path.insert(0, ROOT)
    from rivulus_amd import capi
    from rivulus_amd.capi import RV_FLOAT64, RV_INT64, Predicate, Term, synth_spec
    ctx = capi.Context(0)
    if len(sys.argv) > 2 and sys.argv[2] == "calls":
        import numpy as np
        from rivulus_amd.capi import Column
        rng = np.random.default_rng(7)
        n = 1024
        f = [ctx.upload(Column.from_numpy(rng.integers(0, 7, n, dtype=np.int64), rng.random(n) >= 0.2)),
             ctx.upload(Column.from_numpy(rng.integers(-5, 5, n, dtype=np.int64), rng.random(n) >= 0.2)),
             ctx.upload(Column.from_numpy(rng.integers(-1000, 1000, n, dtype=np.int64), rng.random(n) >= 0.2)),
             ctx.upload(Column.from_numpy(rng.integers(-99, 99, n).astype(np.float64)))]
        strings = ctx.upload(Column.from_strings([f"s{i % 37}" for i in range(n)]))
        table = ctx.join_build(f[2])
        aggs = [("sum", 0), ("sum", 1), ("min", 0)]
        calls = {
            "sort_indices": lambda: ctx.sort_indices(f[2]),
            "sort": lambda: ctx.sort(f, [(1, 1), (2, 2)]),
            "top_k": lambda: ctx.top_k(f, [(3, 0), (1, 1)], 10),
            "hash_aggregate": lambda: ctx.hash_aggregate(f[0], f[2:], aggs),
            "hash_aggregate_keys": lambda: ctx.hash_aggregate_keys(f[:2], f[2:], aggs),
            "group_ids": lambda: ctx.group_ids(f[0]),
            "window": lambda: ctx.window(f, [0], [(1, 0)], [("cum_sum", 2), ("cum_min", 2), ("lag", 3, 1)]),
            "window_frames": lambda: ctx.window_frames(f, [0], [(1, 0)], [("sum", 2, 1, 1)]),
            "join_probe": lambda: table.probe(f[1]),
            "join_probe_full": lambda: table.probe(f[1], 2),
            "hash_join": lambda: ctx.hash_join(f, 2, f, 1),
            "hash_join_outer": lambda: ctx.hash_join(f, 2, f, 1, kind=1),
            "string_dict_build": lambda: ctx.string_dict_build(strings),
            "filter_agg": lambda: ctx.filter_agg(f, Predicate([Term(2, ">", 0)]), 3),
        }
        out = {}
        for name, call in calls.items():
            for _ in range(30):
                call()
            best = 1e9
            for _ in range(3):
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(100):
                    call()  # (the outputs are freed as their handles go)
                ctx.synchronize()
                best = min(best, (time.perf_counter() - t0) / 100 * 1e6)
            out[name] = round(best, 1)
        print(json.dumps(out))
        sys.exit(0)
    if len(sys.argv) > 2 and sys.argv[2] == "plain":
        ctx.set_option("narrow_codes", -1)
    n = 1_000_000_000
    x = ctx.generate(synth_spec(RV_INT64, seed=42, length=n))
    out = {}
    shapes = [("config2", [x], Predicate([Term(0, ">", 899)]), [0])]
    if len(sys.argv) > 2 and sys.argv[2] == "all":
        f = ctx.generate(synth_spec(RV_FLOAT64, seed=43, length=n, validity_seed=44))
        xv = ctx.generate(synth_spec(RV_INT64, seed=42, length=n, validity_seed=45))
        shapes.append(("config3", [f, xv], Predicate([Term(0, ">", 0.5), Term(1, "<", 200)]), [0, 1]))
    for name, cols, pred, proj in shapes:
        run = ctx.prepared_filter_project(cols, pred, proj)
        for _ in range(5):
            run()
        best = (1e9, 1e9)
        for _ in range(3):
            ctx.set_option("profile_kernels", 1)
            ctx.kernel_stats(reset=True)
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                run()
            ctx.synchronize()
            wall = (time.perf_counter() - t0) / 20 * 1e3
            ms, k = ctx.kernel_stats()
            ctx.set_option("profile_kernels", 0)
            best = min(best, (ms / 20, wall))
        out[name] = {"kernel_ms": round(best[0], 4), "call_ms": round(best[1], 4), "kernel": ctx.last_kernel()}
    print(json.dumps(out))
    sys.exit(0)

other = os.path.abspath(sys.argv[1])
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
what = sys.argv[3] if len(sys.argv) > 3 else "config2"
order = (("other", other), ("tree ", None))
if len(sys.argv) > 4 and sys.argv[4] == "tree":
    order = order[::-1]
seen = {"other": [], "tree ": []}
for r in range(rounds):
    for label, lib in order:
        env = dict(os.environ)
        if lib:
            env["RIVULUS_GPU_LIB"] = lib
        else:
            env.pop("RIVULUS_GPU_LIB", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what], env=env, capture_output=True, text=True, timeout=600)
        line = [q for q in p.stdout.splitlines() if q.startswith("{")]
        print(f"round {r} {label} {line[-1] if line else p.stderr[-300:]}", flush=True)
        if p.returncode != 0 or not line:  # nothing more is started on a card after a failure
            sys.exit(1)
        seen[label].append(json.loads(line[-1]))
if what == "calls":  # per operator: median and range of each build over the rounds, microseconds per call
    for name in seen["other"][0]:
        a, b = (sorted(q[name] for q in seen[label]) for label in ("other", "tree "))
        note = "" if a[0] <= b[len(b) // 2] <= a[-1] else "  <- outside the range of the other build"
        print(f"{name}: other {a[len(a) // 2]} ({a[0]}-{a[-1]}), tree {b[len(b) // 2]} ({b[0]}-{b[-1]}){note}")
