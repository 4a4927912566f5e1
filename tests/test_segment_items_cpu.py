"""CPU test of the segmented bit count's work list (rivulus_amd/csrc/segment_items.hpp, shared by segment_popcount_kernel and its
host driver): g++ builds the stand-alone tests/cpp/segment_items_tests.cpp with AddressSanitizer and UBSan and the binary runs as a
program -- the items, read as the kernel reads them, count every range bit for bit and cover every word once."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "segment_items_tests.cpp")


def test_segment_items_under_the_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "segment_items_tests")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 1000, r.stdout[-500:]


def test_items_header_is_the_one_the_kernel_includes():
    """One definition of SegItem and kSegChunkWords: the kernel's header includes the one the CPU program checks."""
    text = open(os.path.join(ROOT, "rivulus_amd", "csrc", "aux_kernels.hpp")).read()
    assert '#include "segment_items.hpp"' in text
    assert "struct SegItem" not in text and "kSegChunkWords =" not in text
