"""The join types of the C++ host layer (rivulus_amd/host/rivulus_host.hpp): JoinType { Inner, Left, Right, Outer, Semi, Anti }
through the eager and the streaming plan.  The cases live in tests/cpp/outer_join_host_tests.cpp; every case is one pytest item."""
import pytest

from helpers import assert_host_case, host_cases

CPU_CASES, GPU_CASES = host_cases("outer_join_host_tests")


@pytest.mark.parametrize("case", CPU_CASES)
def test_outer_join_host_logic(case):
    assert_host_case("outer_join_host_tests", case, True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_outer_join_host_on_device(case):
    assert_host_case("outer_join_host_tests", case, False)
