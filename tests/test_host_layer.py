"""C++ host layer (rivulus_amd/host/rivulus_host.hpp): the mirror of the reference's RecordBatch /
DataStream / planner / eager-plan interfaces over the C ABI.  The cases live in
tests/cpp/host_tests.cpp (they re-express the reference's unit tests); every case is one pytest item."""
import pytest

from helpers import assert_host_case, host_cases

CPU_CASES, GPU_CASES = host_cases("host_tests")


@pytest.mark.parametrize("case", CPU_CASES)
def test_host_logic(case):
    assert_host_case("host_tests", case, True, timeout=600)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_host_layer_on_device(case):
    assert_host_case("host_tests", case, False, timeout=600)
