"""The device CSV scan against the host CsvFileStream and the oracle's rvo::CsvFileStream, call by call (rv_csv_open /
rv_csv_next and CsvFileStream with CsvScan::Device, rivulus_amd/host/rivulus_host.hpp).  The cases live in
tests/cpp/csv_device_tests.cpp; every case is one pytest item."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rivulus_amd", "host")
BIN = os.path.join(HOST, "csv_device_tests")
SRC = open(os.path.join(ROOT, "tests", "cpp", "csv_device_tests.cpp")).read()
GPU_CASES = re.findall(r"^GPU_TEST\((\w+)\)", SRC, re.M)
_cache = {}


def _run():
    if "result" not in _cache:
        subprocess.run(["make", "-C", os.path.join(ROOT, "rivulus_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
        subprocess.run(["make", "-C", HOST, "csv_device_tests"], check=True, stdout=subprocess.DEVNULL)
        with tempfile.TemporaryDirectory(prefix="csv_device_") as d:
            _cache["result"] = subprocess.run([BIN, d], capture_output=True, text=True, timeout=600)
    return _cache["result"]


def test_every_case_is_collected():
    assert len(GPU_CASES) >= 7 and "csv_source_through_the_gpu_filter_project_plan_device_scan" in GPU_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_csv_device_scan_matches_the_host_stream(case):
    result = _run()
    for line in result.stdout.splitlines():
        if line.split()[1:2] == [case] or line.startswith(f"FAIL {case}:"):
            assert line.startswith("ok "), line
            return
    pytest.fail(f"case {case} produced no line; stdout: {result.stdout[-1000:]} stderr: {result.stderr[-1000:]}")
