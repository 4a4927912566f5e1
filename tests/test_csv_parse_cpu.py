"""CPU fuzz of the device CSV cell parsers (rivulus_amd/csrc/csv_parse.hpp): g++ builds tests/cpp/csv_parse_fuzz.cpp against the
parser header and the oracle's grammar, and the binary compares 10^7 generated cells, bit for bit, with the host CsvFileStream's
rule (strtoll / strtod behind the character pre-check).  It fails unless some random cells reach the exact slow path."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "csv_parse_fuzz.cpp")


def _build(tmp):
    exe = os.path.join(tmp, "csv_parse_fuzz")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC], check=True)
    return exe


def test_csv_cell_parsers_match_the_host_rule():
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([_build(tmp), "10000000"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) >= 10_000_000, r.stdout[-500:]


def test_pow5_table_is_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_pow5_table.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
