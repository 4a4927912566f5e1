"""sort(keys) in the C++ host layer (rivulus_amd/host/rivulus_host.hpp): sort_schema, PhysicalPlan::sort and
StreamingPhysicalPlan::sort over rv_sort.  The cases live in tests/cpp/sort_host_tests.cpp; every case is one pytest item."""
import pytest

from helpers import assert_host_case, host_cases

CPU_CASES, GPU_CASES = host_cases("sort_host_tests")


@pytest.mark.parametrize("case", CPU_CASES)
def test_sort_host_logic(case):
    assert_host_case("sort_host_tests", case, True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_sort_host_on_device(case):
    assert_host_case("sort_host_tests", case, False)
