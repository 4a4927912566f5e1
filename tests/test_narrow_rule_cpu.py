"""CPU test of the narrow companions' host-side rule (rivulus_amd/csrc/narrow_rule.hpp): g++ builds the stand-alone
tests/cpp/narrow_host_tests.cpp, plain and with AddressSanitizer + UBSan, and the binary runs as a program -- range arithmetic at the
ends of Int64, the code width, the alignment rule, eligibility, whole scans and both sides of the trigger's constants."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "narrow_host_tests.cpp")
CSRC = os.path.join(ROOT, "rivulus_amd", "csrc")


@pytest.mark.parametrize("extra", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_narrow_rule(extra):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "narrow_host_tests")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-o", exe, SRC], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 1000, r.stdout[-500:]


def test_rule_header_is_the_one_the_library_decides_by():
    """One definition of the rule: the runtime and narrow.hip use the header the CPU program checks, with the table's constants."""
    assert '#include "narrow_rule.hpp"' in open(os.path.join(CSRC, "runtime.hpp")).read()
    unit = open(os.path.join(CSRC, "narrow.hip")).read()
    for name in ("rvn::worth_building", "rvn::code_bytes", "rvn::value_range", "rvn::slice_aligned", "rvn::view_covered", "rvn::buffer_eligible",
                 "rvt::kNarrowAfterWholeScans", "rvt::kNarrowFromRows"):
        assert name in unit, name
