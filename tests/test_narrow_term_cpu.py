"""CPU test of the code-space lowering of the lean compare term (rivulus_amd/csrc/narrow_term.hpp): g++ builds the stand-alone
tests/cpp/narrow_term_host_tests.cpp, plain and with AddressSanitizer + UBSan, and the binary runs as a program -- every selector
subset, both code widths, bases at both ends of Int64, literals on and around every edge, against the plain Int64 comparison."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "narrow_term_host_tests.cpp")
CSRC = os.path.join(ROOT, "rivulus_amd", "csrc")


@pytest.mark.parametrize("extra", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_narrow_term(extra):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "narrow_term_host_tests")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-o", exe, SRC], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    # 5 bases x 8..9 literals x 8 selector subsets x 65536 codes for the 2-byte width alone
    assert last[0] == "ok" and int(last[1]) > 5 * 8 * 8 * 65536, r.stdout[-500:]


def test_term_header_is_the_one_the_library_lowers_by():
    """One definition of the lowering: the launch code calls the header the CPU program checks, and the kernel applies its form."""
    unit = open(os.path.join(CSRC, "fused_launch.hip")).read()
    assert '#include "narrow_term.hpp"' in unit
    for name in ("rvn::lower_term", "rvn::CodeTerm"):
        assert name in unit, name
    kernel = open(os.path.join(CSRC, "fused_kernel.hpp")).read()
    assert "c0 - TLO <= TSPAN" in kernel and "^ TNEG" in kernel
