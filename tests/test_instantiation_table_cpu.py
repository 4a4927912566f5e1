"""Cover of the filter kernels' launch tables is a property of the tables (no GPU): every instantiation the sources list has exactly
one case in tests/test_instantiations_gpu.py or a reason in its UNREACHED, so one added without a case fails here by name."""
import os
import re
from collections import Counter

import helpers
import test_instantiations_gpu as cases

FF = helpers.kernel_flags()
TABLES = helpers.FUSED_SOURCES + helpers.DIRECT_SOURCES
MOST_UNREACHED = 6  # a condition, not a measurement: more means the forcing options do not reach the tables


def macro_uses(name):
    """Entries the macros of a table source spell out, counted on the raw text (the two #define lines aside): RV_DIRECT3 is three."""
    with open(os.path.join(helpers.CSRC, name)) as f:
        body = "".join(line for line in f if not line.startswith("#define"))
    return body.count("RV_FUSED(") + body.count("RV_DIRECT(") + 3 * body.count("RV_DIRECT3(")


def test_reader_finds_every_macro_use():
    for name in TABLES:
        assert len(helpers.table_entries(name)) == macro_uses(name) > 0, name
    fused = sum(len(helpers.table_entries(name)) for name in helpers.FUSED_SOURCES)
    direct = sum(len(helpers.table_entries(name)) for name in helpers.DIRECT_SOURCES)
    assert all(e[0] == "fused_filter_compact" for name in helpers.FUSED_SOURCES for e in helpers.table_entries(name))
    assert all(e[0] == "fused_direct_compact" for name in helpers.DIRECT_SOURCES for e in helpers.table_entries(name))
    assert fused >= 100 and direct >= 50  # (the tables as they stand: 145 and 63)


def test_flags_and_aliases_are_evaluated():
    names = set(helpers.table_kernels())
    # FF_ALL; the alias F of fused_expr.hip; V | A | N of fused_roomy.hip; the third member of an RV_DIRECT3; FF_OUTVALID
    for name in ("fused_filter_compact<0,16,1,16,15>", "fused_filter_compact<3,4,1,16,523>", "fused_filter_compact<3,4,1,8,385>",
                 "fused_direct_compact<1,0,12,8,3>", "fused_direct_compact<1,0,16,8,2049>"):
        assert name in names, name
    assert FF["FF_ONE_I64"] == 32 and FF["FF_OUTVALID"] == 2048


def test_redo_reader_matches_the_switch():
    with open(os.path.join(helpers.CSRC, helpers.REDO_SOURCE)) as f:
        labels = len(re.findall(r"^\s*case \d+:", f.read(), re.M))
    redo = helpers.redo_entries()
    assert len(redo) == labels == len(set(redo)) > 0
    assert sorted(cases.REDO_CASES) == sorted(redo)
    for kernel in cases.REDO_CASES.values():
        assert kernel in helpers.table_kernels(), kernel


def test_every_instantiation_has_exactly_one_case():
    kernels = helpers.table_kernels()
    wanted = {name for name, e in kernels.items() if not e[5] & FF["FF_STAMP"]}
    named = Counter(cases.CASES) + Counter(cases.UNREACHED)
    missing = sorted(wanted - set(named))
    assert not missing, f"instantiations without a case in test_instantiations_gpu.py (or a reason in UNREACHED): {missing}"
    twice = sorted(k for k, c in named.items() if c > 1)
    assert not twice, f"named more than once: {twice}"
    unknown = sorted(set(named) - set(kernels))
    assert not unknown, f"cases that name no entry of the tables: {unknown}"
    stamped = sorted(k for k in named if kernels[k][5] & FF["FF_STAMP"])
    assert not stamped, f"diagnostic FF_STAMP entries are out of scope: {stamped}"


def test_unreached_is_short_and_reasoned():
    assert len(cases.UNREACHED) <= MOST_UNREACHED, sorted(cases.UNREACHED)
    for name, reason in cases.UNREACHED.items():
        assert re.search(r"\b(fused_launch|query)\.hip\b", reason) and len(reason) > 40, f"{name}: the reason names the selecting condition"


def test_many_tiles_cover_every_geometry():
    """One kernel per distinct (rows per lane, waves) pair of either table."""
    kernels = helpers.table_kernels()

    def geometry(name):
        e = kernels[name]
        return (e[0], e[2], e[4]) if e[0] == "fused_filter_compact" else (e[0], e[3], e[4])

    wanted = {geometry(name) for name, e in kernels.items() if not e[5] & FF["FF_STAMP"] and name not in cases.UNREACHED}
    listed = [geometry(name) for name in cases.MANY_TILES]
    assert sorted(set(listed)) == sorted(wanted) and len(listed) == len(set(listed))


def test_no_direct_entry_hides_behind_an_earlier_one():
    """find_direct (csrc/fused_launch.hip) takes the FIRST listed entry of the wanted geometry whose flags cover the launch's: an entry
    listed behind one of the same (columns, rows per lane, waves) with a superset of its flags is never picked, by any option."""
    listed = [e for name in helpers.DIRECT_SOURCES for e in helpers.table_entries(name)]
    stamp = FF["FF_STAMP"]
    for i, e in enumerate(listed):
        for earlier in listed[:i]:
            hides = earlier[1:5] == e[1:5] and (earlier[5] & e[5]) == e[5] and not (earlier[5] ^ e[5]) & stamp
            assert not hides, f"{helpers.kernel_name(e)} is listed behind {helpers.kernel_name(earlier)}, which covers it"
