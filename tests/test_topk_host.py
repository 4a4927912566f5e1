"""top_k(keys, k) in the C++ host layer (rivulus_amd/host/rivulus_host.hpp): top_k_schema, PhysicalPlan::top_k and
StreamingPhysicalPlan::top_k (GpuTopKStream and its folds) over rv_top_k.  The cases live in tests/cpp/topk_host_tests.cpp; every case is
one pytest item."""
import pytest

from helpers import assert_host_case, host_cases

CPU_CASES, GPU_CASES = host_cases("topk_host_tests")


@pytest.mark.parametrize("case", CPU_CASES)
def test_topk_host_logic(case):
    assert_host_case("topk_host_tests", case, True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_topk_host_on_device(case):
    assert_host_case("topk_host_tests", case, False)
