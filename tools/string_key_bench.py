#!/usr/bin/env python3
"""String join keys through the device string dictionary: one JSON line per shape (tools/README.md).

Keys are 16-byte strings, "key-" + 12 digits, over the same numbers the Int64 yardstick joins on.

  dict_build_ms / dict_build_kernel_ms   rv_string_dict_build over `keys` distinct build keys (ids included): wall time of the call,
                                         and its kernels alone (str_dict_insert + str_dict_encode, rv_ctx_kernel_stats)
  encode_ms / encode_kernel_ms           rv_string_dict_encode of the probe keys (hit_share of them are build keys)
  encode_rows_per_s                      probe rows over encode_kernel_ms
  string_join_ms                         the whole String-key join as the host layer runs it: dictionary build + encode +
                                         rv_hash_join over (ids, payload) against (String key, payload, ids)
  int64_join_ms                          THE YARDSTICK: rv_hash_join over (Int64 key, payload) on both sides, the same numbers as keys,
                                         in the same process on the same device -- unchanged code
  string_over_int64                      string_join_ms / int64_join_ms
All times are wall clock around the call on an idle stream (HIP events), the median of --reps runs."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rivulus_amd import capi  # noqa: E402
from rivulus_amd.capi import RV_STRING, Column  # noqa: E402

_QUADS = np.array([list(b"%04d" % i) for i in range(10000)], dtype=np.uint8)
KEY_BYTES = 16


def string_keys(numbers: np.ndarray) -> Column:
    """"key-" + the number in 12 digits: one 16-byte cell per row, no nulls."""
    n = len(numbers)
    data = np.empty((n, KEY_BYTES), dtype=np.uint8)
    data[:, 0:4] = np.frombuffer(b"key-", dtype=np.uint8)
    data[:, 4:8] = _QUADS[numbers // 10**8]
    data[:, 8:12] = _QUADS[(numbers // 10**4) % 10**4]
    data[:, 12:16] = _QUADS[numbers % 10**4]
    offsets = (np.arange(n + 1, dtype=np.int64) * KEY_BYTES).astype(np.int32)
    return Column(RV_STRING, data.reshape(-1), None, 0, n, offsets)


def timed(ctx, fn):
    ctx.synchronize()
    ctx.timer_start()
    r = fn()
    ms = ctx.timer_stop()
    return ms, r


def timed_kernels(ctx, fn):
    ctx.kernel_stats(reset=True)
    ms, r = timed(ctx, fn)
    return ms, ctx.kernel_stats(reset=True)[0], r


def shape(ctx, name, n_probe, n_keys, hit_share, reps):
    assert n_probe * KEY_BYTES < 2**31, "a String column holds at most 2 GiB"
    rng = np.random.default_rng(n_keys)
    bk = rng.permutation(n_keys).astype(np.int64)
    pk = rng.integers(0, int(round(n_keys / hit_share)), n_probe, dtype=np.int64)  # hit_share of them are build keys
    b_int, p_int = ctx.upload(Column.from_numpy(bk)), ctx.upload(Column.from_numpy(pk))
    b_str, p_str = ctx.upload(string_keys(bk)), ctx.upload(string_keys(pk))
    b_pay = ctx.upload(Column.from_numpy(np.arange(n_keys, dtype=np.int64)))
    p_pay = ctx.upload(Column.from_numpy(np.arange(n_probe, dtype=np.int64)))
    del bk, pk
    res = {k: [] for k in ("build", "build_k", "encode", "encode_k", "sjoin", "ijoin")}
    rows = 0
    for _ in range(reps):
        ms, kms, (d, ids_b) = timed_kernels(ctx, lambda: ctx.string_dict_build(b_str))
        res["build"].append(ms), res["build_k"].append(kms)
        ms, kms, ids_p = timed_kernels(ctx, lambda: d.encode(p_str))
        res["encode"].append(ms), res["encode_k"].append(kms)
        ids_b.free(), ids_p.free(), d.free()

        def string_join():
            d, ids_b = ctx.string_dict_build(b_str)
            ids_p = d.encode(p_str)
            outs, jrows = ctx.hash_join([ids_b, b_pay], 0, [p_str, p_pay, ids_p], 2)
            d.free()
            return outs, jrows
        ms, (outs, srows) = timed(ctx, string_join)
        res["sjoin"].append(ms)
        for o in outs:
            o.free()
        ms, (outs, rows) = timed(ctx, lambda: ctx.hash_join([b_int, b_pay], 0, [p_int, p_pay], 0))
        res["ijoin"].append(ms)
        for o in outs:
            o.free()
        assert srows == rows, (srows, rows)
    med = {k: float(np.median(v)) for k, v in res.items()}
    line = {"shape": name, "probe_rows": n_probe, "keys": n_keys, "key_bytes": KEY_BYTES, "hit_share": hit_share, "rows": rows,
            "dict_build_ms": round(med["build"], 3), "dict_build_kernel_ms": round(med["build_k"], 3),
            "encode_ms": round(med["encode"], 3), "encode_kernel_ms": round(med["encode_k"], 3),
            "encode_rows_per_s": round(n_probe / (med["encode_k"] * 1e-3), 0) if med["encode_k"] > 0 else None,
            "string_join_ms": round(med["sjoin"], 3), "int64_join_ms": round(med["ijoin"], 3),
            "string_over_int64": round(med["sjoin"] / med["ijoin"], 2), "reps": reps, "device": ctx.device_info()["name"]}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--probe-rows", type=int, default=10**8)
    ap.add_argument("--keys", type=int, default=10**6)
    args = ap.parse_args()
    with capi.Context(0) as ctx:
        ctx.set_option("profile_kernels", 1)
        shape(ctx, f"{args.keys:.0e}_keys_10pct".replace("+0", ""), args.probe_rows, args.keys, 0.10, args.reps)
        shape(ctx, f"{args.keys:.0e}_keys_100pct".replace("+0", ""), args.probe_rows, args.keys, 1.00, args.reps)


if __name__ == "__main__":
    main()
