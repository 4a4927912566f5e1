"""CPU test of the packed layout of the narrow companions and of the rule around it (rivulus_amd/csrc/narrow_rule.hpp, narrow_term.hpp):
g++ builds the stand-alone tests/cpp/narrow_pack10_host_tests.cpp, plain and with AddressSanitizer + UBSan, and the binary runs as a
program -- the index arithmetic against a brute-force pack, padding, spare bits, companion size, the width and alignment edges, which
layout is built, which launch reads which, the second cover, and the folded compare terms over every 10-bit code."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "narrow_pack10_host_tests.cpp")
CSRC = os.path.join(ROOT, "rivulus_amd", "csrc")


@pytest.mark.parametrize("extra", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_packed_layout_and_rule(extra):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "narrow_pack10_host_tests")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-o", exe, SRC], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 100000, r.stdout[-500:]


def test_one_definition_of_the_layout():
    """The pack kernel, the pass's load, the launch code and the CPU program share narrow_rule.hpp's arithmetic and constants."""
    kernel = open(os.path.join(CSRC, "narrow_kernel.hpp")).read()
    assert '#include "narrow_rule.hpp"' in kernel
    for name in ("rvn::kPackGroup", "rvn::kPackMask"):
        assert name in kernel, name
    unit = open(os.path.join(CSRC, "narrow.hip")).read()
    for name in ("rvn::layout_to_build", "rvn::layout_to_read", "rvn::count_pass_in", "rvn::second_layout", "rvn::packed_bytes"):
        assert name in unit, name
    launch = open(os.path.join(CSRC, "fused_launch.hip")).read()
    assert "rvn::packed_bytes" in launch and "rvn::Layout::kPacked" in launch
