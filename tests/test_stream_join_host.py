"""The streaming HashJoin arm of the C++ host layer (StreamingPhysicalPlan::hash_join -> GpuHashJoinStream,
rivulus_amd/host/rivulus_host.hpp).  The cases live in tests/cpp/stream_join_host_tests.cpp; every case is one pytest item.
The users / orders fixture (tests/golden/join_users_orders.json) is handed to the binary as CSV files."""
import json
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rivulus_amd", "host")
BIN = os.path.join(HOST, "stream_join_host_tests")
SRC = open(os.path.join(ROOT, "tests", "cpp", "stream_join_host_tests.cpp")).read()
CPU_CASES = re.findall(r"^CPU_TEST\((\w+)\)", SRC, re.M)
GPU_CASES = re.findall(r"^GPU_TEST\((\w+)\)", SRC, re.M)
_cache = {}


def _csv(path, columns):
    """columns: [(name, cells)] -> a comma-separated file with a header line"""
    with open(path, "w") as f:
        f.write(",".join(name for name, _ in columns) + "\n")
        for row in zip(*(cells for _, cells in columns)):
            f.write(",".join(repr(x) if isinstance(x, float) else str(x) for x in row) + "\n")


def _fixture_dir():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "join_users_orders.json")))
    _cache["fixture"] = tempfile.TemporaryDirectory(prefix="stream_join_")  # removed with the module's cache
    d = _cache["fixture"].name
    _csv(os.path.join(d, "users.csv"), [(c["name"], c["cells"]) for c in g["users"]])
    _csv(os.path.join(d, "orders.csv"), [(c["name"], c["cells"]) for c in g["orders"]])
    _csv(os.path.join(d, "expected.csv"), list(zip(g["columns"], g["result"])))
    return d


def _run(cpu_only: bool):
    if cpu_only not in _cache:
        subprocess.run(["make", "-C", os.path.join(ROOT, "rivulus_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
        subprocess.run(["make", "-C", HOST, "stream_join_host_tests"], check=True, stdout=subprocess.DEVNULL)
        _cache[cpu_only] = subprocess.run([BIN] + (["--cpu"] if cpu_only else []) + [_fixture_dir()], capture_output=True, text=True,
                                          timeout=300)
    return _cache[cpu_only]


def _assert_case(result, case):
    for line in result.stdout.splitlines():
        if line.split()[1:2] == [case] or line.startswith(f"FAIL {case}:"):
            assert line.startswith("ok "), line
            return
    pytest.fail(f"case {case} produced no line; stderr: {result.stderr[-500:]}")


@pytest.mark.parametrize("case", CPU_CASES)
def test_stream_join_host_logic(case):
    _assert_case(_run(True), case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_stream_join_host_on_device(case):
    _assert_case(_run(False), case)
