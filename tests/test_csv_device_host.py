"""The device CSV scan against the host CsvFileStream and the oracle's rvo::CsvFileStream, call by call (rv_csv_open /
rv_csv_next and CsvFileStream with CsvScan::Device, rivulus_amd/host/rivulus_host.hpp).  The cases live in
tests/cpp/csv_device_tests.cpp; every case is one pytest item."""
import tempfile

import pytest

from helpers import assert_host_case, host_cases

GPU_CASES = host_cases("csv_device_tests")[1]
_scratch = []


def _scratch_dir():
    _scratch.append(tempfile.TemporaryDirectory(prefix="csv_device_"))  # removed with the module
    return _scratch[-1].name


def test_every_case_is_collected():
    assert len(GPU_CASES) >= 7 and "csv_source_through_the_gpu_filter_project_plan_device_scan" in GPU_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_csv_device_scan_matches_the_host_stream(case):
    assert_host_case("csv_device_tests", case, False, arg=_scratch_dir, timeout=600)
