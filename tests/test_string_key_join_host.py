"""String join keys in the C++ host layer (rivulus_amd/host/rivulus_host.hpp): PhysicalPlan::hash_join and
StreamingPhysicalPlan::hash_join / GpuHashJoinStream over the device string dictionary.  The cases live in
tests/cpp/string_key_join_tests.cpp; every case is one pytest item."""
import pytest

from helpers import assert_host_case, host_cases

CPU_CASES, GPU_CASES = host_cases("string_key_join_tests")


@pytest.mark.parametrize("case", CPU_CASES)
def test_string_key_join_host_logic(case):
    assert_host_case("string_key_join_tests", case, True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_string_key_join_host_on_device(case):
    assert_host_case("string_key_join_tests", case, False)
