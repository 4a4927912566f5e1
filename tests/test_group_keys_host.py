"""group_by([k0, k1, ...]).agg([...]) in the C++ host layer (rivulus_amd/host/rivulus_host.hpp): the key-list forms of group_by_schema,
PhysicalPlan::group_by and StreamingPhysicalPlan::group_by over rv_hash_aggregate_keys.  The cases live in
tests/cpp/group_keys_host_tests.cpp; every case is one pytest item."""
import pytest

from helpers import assert_host_case, host_cases

CPU_CASES, GPU_CASES = host_cases("group_keys_host_tests")


@pytest.mark.parametrize("case", CPU_CASES)
def test_group_keys_host_logic(case):
    assert_host_case("group_keys_host_tests", case, True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_group_keys_host_on_device(case):
    assert_host_case("group_keys_host_tests", case, False)
