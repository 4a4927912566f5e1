"""Window frames in the C++ host layer (rivulus_amd/host/rivulus_host.hpp): the new WindowOps through window_schema, PhysicalPlan::window
and StreamingPhysicalPlan::window over rv_window_frames.  The cases live in tests/cpp/window_frame_host_tests.cpp; every case is one
pytest item."""
import pytest

from helpers import assert_host_case, host_cases

CPU_CASES, GPU_CASES = host_cases("window_frame_host_tests")


@pytest.mark.parametrize("case", CPU_CASES)
def test_window_frame_host_logic(case):
    assert_host_case("window_frame_host_tests", case, True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_window_frame_host_on_device(case):
    assert_host_case("window_frame_host_tests", case, False)
