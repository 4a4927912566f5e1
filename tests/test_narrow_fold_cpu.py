"""CPU test of the negate fold of the narrow pass's compare term (rivulus_amd/csrc/narrow_term.hpp, fold_negate): g++ builds the
stand-alone tests/cpp/narrow_fold_host_tests.cpp, plain and with AddressSanitizer + UBSan, and the binary runs as a program -- the
folded term against the unfolded one over every 2-byte code and around every edge of the 4-byte ones; the only term without an
interval is the empty set over 4-byte codes."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "narrow_fold_host_tests.cpp")
CSRC = os.path.join(ROOT, "rivulus_amd", "csrc")


@pytest.mark.parametrize("extra", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_narrow_fold(extra):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "narrow_fold_host_tests")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-o", exe, SRC], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    # 8 bases x at least 3 literals x 8 selector subsets x 65536 codes for the 2-byte width alone
    assert last[0] == "ok" and int(last[1]) > 8 * 3 * 8 * 65536, r.stdout[-500:]


def test_the_launch_folds_and_the_kernel_tests_one_interval():
    """The launch code lowers and folds in one place; the kernel's unrolled form for whole tiles tests the interval alone, and the
    flip is left in the second form only (for the one term fold_negate hands back negated)."""
    unit = open(os.path.join(CSRC, "fused_launch.hip")).read()
    assert unit.count("rvn::fold_negate(rvn::lower_term(") == 1 and unit.count("rvn::lower_term(") == 1
    kernel = open(os.path.join(CSRC, "fused_kernel.hpp")).read()
    assert kernel.count("ballot64(c0 - TLO <= TSPAN), m1 = ballot64(c1 - TLO <= TSPAN);") == 1  # the form every whole tile runs
    assert kernel.count("^ TNEG") == 2 and "full && project && !negated" in kernel  # the second form: both rows of a pair
