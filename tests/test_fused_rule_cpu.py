"""CPU test of the staged pass's launch rule (rivulus_amd/csrc/fused_rule.hpp): g++ builds the stand-alone tests/cpp/fused_rule_tests.cpp,
plain and with AddressSanitizer + UBSan, and the binary runs as a program over the real launch tables, read from the table sources in
registry order.  The program holds the rule to the scoring scan and the walk loop it replaced, for every combination of its inputs, and
prints how many it compared: the counts are worked out here from the tables, so none can have been skipped."""
import os
import re
import subprocess
import tempfile

import pytest

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fused_rule_tests.cpp")
CSRC = os.path.join(ROOT, "rivulus_amd", "csrc")
SOURCES = helpers.FUSED_SOURCES + (helpers.NARROW_SOURCE,)  # the registry's order (fused_table.hpp, fused_entries)
FF = helpers.kernel_flags()
MAX_WALK = 24  # kMaxWalk of the program


def registry():
    """(source index, ncols, r, vec, waves, flags) of every staged entry, in registry order."""
    return [(i,) + e[1:] for i, src in enumerate(SOURCES) for e in helpers.table_entries(src)]


def tall_rows():
    text = open(os.path.join(CSRC, "fused_table.hpp")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", text).group(1)) for name in ("kNarrowTallRows", "kPackedTallRows"))


def expected_counts(entries):
    """(picks, members, walks) the program must report: the products of its dimensions."""
    narrow = FF["FF_NARROW16"] | FF["FF_NARROW32"] | FF["FF_PACK10"]
    clearable = (FF["FF_VALIDITY"], FF["FF_BOOL"], FF["FF_XS"], FF["FF_SEL"])
    needs = set()
    for e in entries:
        for m in range(16):
            need = e[5]
            for b, bit in enumerate(clearable):
                if m >> b & 1:
                    need &= ~bit
            needs |= {need, need | FF["FF_SEL"]}
    rows = {e[2] for e in entries}
    forced = {0, 5 | 3 << 8} | {e[2] | e[4] << 8 for e in entries} | rows
    # ncols 0..4, vec 1 and 2, need, four `prefer`, three levels, below_r (2^30 and every rows-per-lane value), four `prefer_r`, forced
    picks = 5 * 2 * len(needs) * 4 * 3 * (len(rows) + 1) * 4 * len(forced)
    members = len({e[5] for e in entries if e[5] & narrow}) * len(forced)
    keys = [(e[1], e[3], e[5]) for e in entries]
    classes = {k for k in keys if keys.count(k) > 1}
    # four `prefer`, per-batch counts off and four batch sizes, selection bitmap deferred or not, two `forced`, 0..MAX_WALK crowded answers
    walks = len(classes) * 4 * 5 * 2 * 2 * (MAX_WALK + 1)
    return picks, members, walks


@pytest.mark.parametrize("extra", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_fused_rule(extra):
    entries = registry()
    assert len(entries) > 150 and {e[0] for e in entries} == set(range(len(SOURCES)))
    with tempfile.TemporaryDirectory() as tmp:
        tables = os.path.join(tmp, "tables.txt")
        with open(tables, "w") as f:
            for name, value in FF.items():
                f.write(f"flag {name} {value}\n")
            f.write("tall %d %d\n" % tall_rows())
            for e in entries:
                f.write("entry %d %d %d %d %d %d\n" % e)
        exe = os.path.join(tmp, "fused_rule_tests")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-o", exe, SRC], check=True)
        r = subprocess.run([exe, tables], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    got = {line.split()[0]: int(line.split()[1]) for line in lines}
    picks, members, walks = expected_counts(entries)
    assert (got["picks"], got["members"], got["walks"]) == (picks, members, walks), r.stdout[-500:]
    assert got["ok"] == picks + members + walks and picks > 1000000


def test_rule_header_is_the_one_the_library_decides_by():
    """One definition of the rule: the launch unit includes the header the CPU program checks and chooses through it; the scan is gone."""
    unit = open(os.path.join(CSRC, "fused_launch.hip")).read()
    assert '#include "fused_rule.hpp"' in unit
    for name in ("rvf::Walk<rvk::FusedEntry>", "walk.first()", "walk.next()", "walk.reclass(", "rvf::holds_exactly(", "rvk::fused_entries("):
        assert name in unit, name
    for name in ("find_fused", "pick_fused", "plain_twin", "narrow_instantiated"):
        assert name not in unit, name
    header = open(os.path.join(CSRC, "fused_rule.hpp")).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", header).lower() and "rv_ctx" not in header
