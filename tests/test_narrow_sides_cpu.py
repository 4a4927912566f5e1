"""CPU test of the one-sided classifier of a pass over packed codes (rivulus_amd/csrc/narrow_sides.hpp): g++ builds the stand-alone
tests/cpp/narrow_sides_host_tests.cpp, plain and with AddressSanitizer + UBSan, and the binary runs as a program -- for every companion
range up to 64 and every interval the launch's lowering and fold can produce, the class's test against the interval's own over every
code of the range; wrapped intervals are two-sided, single compares one-sided."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "narrow_sides_host_tests.cpp")


@pytest.mark.parametrize("extra", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_narrow_sides(extra):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "narrow_sides_host_tests")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-o", exe, SRC], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    # 65 ranges x 5 bases x at least 5 literals x 8 selector subsets, every code of the range for each
    assert last[0] == "ok" and int(last[1]) > 65 * 5 * 5 * 8, r.stdout[-500:]

