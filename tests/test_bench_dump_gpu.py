"""bench.py --dump-outputs on the device (-m gpu): every driver writes what its last timed step computed -- the same arrays for
the same result whichever way the rows were cut (one context, the stream seam, the single-process group, one process per rank,
a host-resident table) --, equal to the oracle's result at the sampled rows, and identical from run to run; `steps` in the line
is the --steps asked for."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from rivulus_amd.capi import RV_FLOAT64, RV_INT64, Predicate, Term, synth_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ROWS = 12_000_000   # ~1.2e6 survivors: more than bench.DUMP_SAMPLE_ROWS, so the sample is exercised


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _bench(out_dir, extra, launcher_ranks=0, steps=3):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(RV_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "1", "--no-cpu-baseline", "--no-end-to-end",
           "--dump-outputs", str(out_dir)] + extra
    if launcher_ranks:
        cmd = ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={launcher_ranks}", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port())] + cmd
    r = subprocess.run([sys.executable] + cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout + r.stderr[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["ms_per_step"] > 0, line
    files = sorted(f for f in os.listdir(out_dir) if f.endswith(".npy"))
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    return arrays


@pytest.fixture(scope="module")
def headline_expected(oracle):
    hx = oracle.generate(synth_spec(RV_INT64, seed=42, length=ROWS))
    got = oracle.filter_project([hx], Predicate([Term(0, ">", 899)]), [0])[0]
    return got.logical_values()


def _check_headline(arrays, want):
    assert sorted(arrays) == ["index", "rows", "x"]
    assert arrays["rows"].tolist() == [float(len(want))]
    idx = arrays["index"].astype(np.int64)
    assert len(idx) == min(len(want), 1 << 20) and np.all(np.diff(idx) > 0)
    assert np.array_equal(arrays["x"], want[idx].astype(np.float64))


@pytest.mark.parametrize("how", ["one_context", "seam_chunked", "seam_chunked_one_step", "group_2", "launcher_2", "host_table"])
def test_every_driver_dumps_the_same_headline_result(tmp_path, headline_expected, how):
    extra, ranks, steps = {"one_context": (["--rows", str(ROWS)], 0, 3),
                           "seam_chunked": (["--rows", str(ROWS), "--seam", "chunked:1024"], 0, 3),
                           # one step: the pass whose windows are kept for the dump is also the one whose survivors are reported
                           "seam_chunked_one_step": (["--rows", str(ROWS), "--seam", "chunked:1024"], 0, 1),
                           "group_2": (["--gpus", "2", "--rows", str(ROWS // 2), "--no-strong-1e9"], 0, 3),
                           "launcher_2": (["--gpus", "2", "--rows", str(ROWS // 2), "--no-strong-1e9"], 2, 3),
                           "host_table": (["--workload", "host_table", "--rows", str(ROWS)], 0, 3)}[how]
    _check_headline(_bench(tmp_path / "a", extra, ranks, steps), headline_expected)


@pytest.mark.parametrize("steps", [1, 2])
def test_a_seam_pass_of_several_windows_dumps_what_one_launch_computes(tmp_path, steps):
    """Seam windows hold 2^28 rows: 3e8 rows are two windows per pass, whose kept outputs are joined in row order."""
    rows = ["--rows", str(300_000_000)]
    seam = _bench(tmp_path / "seam", rows + ["--seam", "chunked:1024"], steps=steps)
    one = _bench(tmp_path / "one", rows)
    assert sorted(seam) == sorted(one) and all(np.array_equal(seam[k], one[k]) for k in one)
    assert len(one["index"]) == 1 << 20


def test_the_dump_is_the_same_from_run_to_run(tmp_path, headline_expected):
    a = _bench(tmp_path / "a", ["--rows", str(ROWS)])
    b = _bench(tmp_path / "b", ["--rows", str(ROWS)])
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert open(tmp_path / "a" / ".gitignore").read() == "*\n"


def test_nullable_outputs_dump_values_and_validity(tmp_path, oracle):
    n = 3_000_000
    arrays = _bench(tmp_path / "a", ["--workload", "and2_nulls", "--rows", str(n)])
    hf = oracle.generate(synth_spec(RV_FLOAT64, seed=43, length=n, validity_seed=44))
    hx = oracle.generate(synth_spec(RV_INT64, seed=42, length=n, validity_seed=45))
    want = oracle.filter_project([hf, hx], Predicate([Term(0, ">", 0.5), Term(1, "<", 200)]), [0, 1])
    assert sorted(arrays) == ["f", "f_valid", "index", "rows", "x", "x_valid"]
    idx = arrays["index"].astype(np.int64)
    assert arrays["rows"].tolist() == [float(want[0].length)] and len(idx) == want[0].length   # < 2^20 rows: all of them
    for name, col in zip(("f", "x"), want):
        assert np.array_equal(arrays[name], col.logical_values()[idx].astype(np.float64))
        valid = col.logical_valid()
        assert np.array_equal(arrays[name + "_valid"], np.ones(len(idx), np.float32) if valid is None else valid[idx].astype(np.float32))


def test_filter_agg_dumps_sum_and_count(tmp_path, headline_expected):
    arrays = _bench(tmp_path / "a", ["--workload", "filter_agg", "--rows", str(ROWS)])
    assert sorted(arrays) == ["count", "sum"]
    assert arrays["count"].tolist() == [float(len(headline_expected))]
    assert arrays["sum"].tolist() == [float(headline_expected.sum())]
