#!/usr/bin/env python3
"""The CSV scan, host stream against device stream: one JSON line per mode (tools/README.md).

A file of --rows rows and four columns (Int64, Float64, Boolean, String; 1 % nulls in the Int64 column) is written once
under --dir (reused when it is there), read once to warm the page cache, and then scanned end to end by tools/csv_bench.cpp
(compiled here with g++ against the C++ host layer):
  mode host     CsvFileStream, CsvScan::Host: getline + strtoll / strtod on one host core, each batch uploaded
  mode device   CsvFileStream, CsvScan::Device: pinned chunks, the kernels of csv_kernels.hpp
  mode stages   what the device pipeline is made of, each on its own: the file read into pinned memory (64 MiB reads) and
                the upload of as many bytes
Every line: rows/s, file GB/s, seconds.  The kernels' own time: run this under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_file(path, rows, seed=1):
    rng = np.random.default_rng(seed)
    step = 1_000_000
    with open(path, "w") as f:
        f.write("id,score,active,name\n")
        for s in range(0, rows, step):
            n = min(step, rows - s)
            ids = rng.integers(-10**12, 10**12, n).astype(str)
            ids = np.where(rng.random(n) < 0.01, "", ids)
            score = np.char.mod("%.4f", rng.standard_normal(n) * 100)
            active = np.where(rng.random(n) < 0.5, "true", "false")
            name = np.char.add("user", rng.integers(0, 10**6, n).astype(str))
            cols = [ids, score, active, name]
            line = cols[0]
            for c in cols[1:]:
                line = np.char.add(np.char.add(line, ","), c)
            f.write("\n".join(line) + "\n")


def build(tmp):
    exe = os.path.join(tmp, "csv_bench")
    lib = os.path.join(ROOT, "rivulus_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "csv_bench.cpp"), f"-L{lib}", "-lrivulus_gpu",
                    f"-Wl,-rpath,{lib}"], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--modes", default="stages,device,host")
    ap.add_argument("--reps", type=int, default=1, help="device runs, one line each")
    a = ap.parse_args()
    path = os.path.join(a.dir, f"csv_bench_{a.rows}.csv")
    if not os.path.exists(path):
        write_file(path, a.rows)
    size = os.path.getsize(path)
    with open(path, "rb") as f:  # warm page cache
        while f.read(64 << 20):
            pass
    exe = build(a.dir)
    for mode in a.modes.split(","):
        for rep in range(a.reps if mode == "device" else 1):
            r = subprocess.run([exe, path, mode, "ifbs"], capture_output=True, text=True, timeout=1800)
            if r.returncode != 0:
                sys.exit(f"{mode}: {r.stderr[-2000:]}")
            out = json.loads(r.stdout.strip().splitlines()[-1])
            out.update({"mode": mode, "rep": rep, "file_bytes": size, "rows_in_file": a.rows})
            if "seconds" in out:
                out["rows_per_s"] = out["rows"] / out["seconds"]
                out["file_gbs"] = size / out["seconds"] / 1e9
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
