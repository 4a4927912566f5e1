"""The streaming HashJoin arm of the C++ host layer (StreamingPhysicalPlan::hash_join -> GpuHashJoinStream,
rivulus_amd/host/rivulus_host.hpp).  The cases live in tests/cpp/stream_join_host_tests.cpp; every case is one pytest item.
The users / orders fixture (tests/golden/join_users_orders.json) is handed to the binary as CSV files."""
import json
import os
import tempfile

import pytest

from helpers import ROOT, assert_host_case, host_cases

CPU_CASES, GPU_CASES = host_cases("stream_join_host_tests")
_fixtures = []


def _csv(path, columns):
    """columns: [(name, cells)] -> a comma-separated file with a header line"""
    with open(path, "w") as f:
        f.write(",".join(name for name, _ in columns) + "\n")
        for row in zip(*(cells for _, cells in columns)):
            f.write(",".join(repr(x) if isinstance(x, float) else str(x) for x in row) + "\n")


def _fixture_dir():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "join_users_orders.json")))
    _fixtures.append(tempfile.TemporaryDirectory(prefix="stream_join_"))  # removed with the module
    d = _fixtures[-1].name
    _csv(os.path.join(d, "users.csv"), [(c["name"], c["cells"]) for c in g["users"]])
    _csv(os.path.join(d, "orders.csv"), [(c["name"], c["cells"]) for c in g["orders"]])
    _csv(os.path.join(d, "expected.csv"), list(zip(g["columns"], g["result"])))
    return d


@pytest.mark.parametrize("case", CPU_CASES)
def test_stream_join_host_logic(case):
    assert_host_case("stream_join_host_tests", case, True, arg=_fixture_dir)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_stream_join_host_on_device(case):
    assert_host_case("stream_join_host_tests", case, False, arg=_fixture_dir)
