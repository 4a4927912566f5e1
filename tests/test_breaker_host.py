"""What the pipeline breakers of the C++ host layer (rivulus_amd/host/rivulus_host.hpp) share: GpuGroupByStream, GpuSortStream,
GpuTopKStream and GpuWindowStream over a frame, one batch and several batches, against the eager PhysicalPlan.  The cases live in
tests/cpp/breaker_host_tests.cpp; every case is one pytest item."""
import pytest

from helpers import assert_host_case, host_cases

CPU_CASES, GPU_CASES = host_cases("breaker_host_tests")


@pytest.mark.parametrize("case", CPU_CASES)
def test_breaker_host_logic(case):
    assert_host_case("breaker_host_tests", case, True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_breaker_host_on_device(case):
    assert_host_case("breaker_host_tests", case, False)
