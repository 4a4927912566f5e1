"""Arithmetic select and filter expressions in the C++ host layer (rivulus_amd/host/rivulus_host.hpp): lower_select_exprs,
lower_computed_predicate, PhysicalPlan::project / computed_filter and StreamingPhysicalPlan::project / computed_filter_project
over rv_eval_arith.  The cases live in tests/cpp/arith_host_tests.cpp; every case is one pytest item."""
import pytest

from helpers import assert_host_case, host_cases

CPU_CASES, GPU_CASES = host_cases("arith_host_tests")


@pytest.mark.parametrize("case", CPU_CASES)
def test_arith_host_logic(case):
    assert_host_case("arith_host_tests", case, True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_arith_host_on_device(case):
    assert_host_case("arith_host_tests", case, False)
