"""CPU test of the staged pass's per-tile arithmetic (rivulus_amd/csrc/tile_addr.hpp): g++ builds the stand-alone tests/cpp/tile_addr_tests.cpp,
plain and with AddressSanitizer + UBSan, and the binary runs as a program.  It holds the header to the per-tile expressions it replaced
(`first / 384 * 512`, `first * BYTES`, `tile_base + TILE <= n`, the `left` clamps) for every geometry of the narrow table, every code width,
view offsets up to byte offsets past 2^40, n on both sides of a tile, a wave range and a super-group, and tile ids 0, 1, ntiles - 1, ntiles
and 2^32 - 1, and prints how many it compared: the count is worked out here, so none can have been skipped."""
import os
import re
import subprocess
import tempfile

import pytest

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tile_addr_tests.cpp")
CSRC = os.path.join(ROOT, "rivulus_amd", "csrc")


def program_list(name):
    text = open(SRC).read()
    return re.search(rf"{name}\[\] = \{{([^}}]*)\}}", text).group(1)


def test_geometries_are_the_narrow_table():
    """The program's rows-per-lane list is what fused_narrow.hip instantiates, all of it."""
    rows = {e[2] for e in helpers.table_entries(helpers.NARROW_SOURCE)}
    assert rows == {int(x) for x in program_list("geometries").split(",")} == {48, 24, 12, 32, 16, 8, 4}


@pytest.mark.parametrize("extra", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_tile_addr(extra):
    geometries = [int(x) for x in program_list("geometries").split(",")]
    widths = [int(x) for x in program_list("widths").split(",")]
    assert widths == [0, 2, 4]
    offsets, ns, counts, tiles, waves = program_list("offsets").count(",") + 1, program_list("ns").count(",") + 1, 2, 5, 16
    assert (offsets, ns) == (6, 12)
    expected = sum(offsets * ns * counts * tiles * waves for r in geometries for cb in widths if cb or r % 6 == 0)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "tile_addr_tests")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-o", exe, SRC], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = {line.split()[0]: int(line.split()[1]) for line in r.stdout.strip().splitlines()}
    assert got == {"compared": expected, "failed": 0} and expected == 17 * 6 * 12 * 2 * 5 * 16


def test_header_is_the_one_the_kernel_and_the_launch_use():
    """One definition: the launch fills the walk through the header, the kernel asks it per tile, and the packed form's division is gone."""
    launch = open(os.path.join(CSRC, "fused_launch.hip")).read()
    kernel = open(os.path.join(CSRC, "fused_kernel.hpp")).read()
    loads = open(os.path.join(CSRC, "scan_frontend.hpp")).read()
    assert '#include "tile_addr.hpp"' in launch and '#include "tile_addr.hpp"' in kernel
    for name in ("rvtile::codes_walk(", "rvk::put_tile_walk("):
        assert name in launch, name
    for name in ("rvtile::tile_full(", "rvtile::wave_rows_left(", "rvtile::wave_byte_at(", "rvtile::wave_bytes_left("):
        assert name in kernel, name
    code = re.sub(r"//[^\n]*", "", kernel + loads)
    # (the passes over packed codes take the new loop; the 2- and 4-byte loaders and the other forms keep their expressions)
    assert "/ 384u * 512u" not in code
