"""CPU test of the string dictionary's hash (rivulus_amd/csrc/string_hash.hpp, shared by the kernels and the host): g++ builds the
stand-alone tests/cpp/string_hash_tests.cpp with AddressSanitizer and UBSan and the binary runs as a program -- the same hash from
every start alignment, no read outside the 8-byte words a cell lies in, the length mixed in, byte equality."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "string_hash_tests.cpp")


def test_string_hash_under_the_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "string_hash_tests")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 1000, r.stdout[-500:]


def test_hash_header_is_the_one_the_kernels_include():
    """One definition of the hash: the kernels include the header the CPU program checks."""
    text = open(os.path.join(ROOT, "rivulus_amd", "csrc", "string_dict_kernel.hpp")).read()
    assert '#include "string_hash.hpp"' in text
    assert "rvstr::string_hash" in text and "rvstr::string_equal" in text
