"""Every pass over codes and its plain twin (csrc/fused_narrow.hip, RV_NARROW: an entry carries the lean Int64 instantiation of its
geometry, which re-runs the pass over the 8-byte values after an output overflow; -m gpu).  One case per entry of the narrow table, read
from the source, the diagnostic FF_STAMP entries aside: the entry's geometry is forced, the kernel that ran is the entry's by name, the
outputs are sized far too small, and the re-run's values and row count are numpy's."""
import numpy as np
import pytest

import helpers
from rivulus_amd import capi
from rivulus_amd.capi import Column, Predicate, Term

pytestmark = pytest.mark.gpu

FF = helpers.kernel_flags()
ENTRIES = [e for e in helpers.table_entries(helpers.NARROW_SOURCE) if not e[5] & FF["FF_STAMP"]]
WAVES = 16


def test_the_table_is_read():
    """2-byte codes at 16, 32, 8 and 4 rows per lane, 4-byte codes at 16, 8 and 4, packed ones at 48, 24 and 12."""
    n16, n32, packed = FF["FF_ONE_I64"] | FF["FF_NARROW16"], FF["FF_ONE_I64"] | FF["FF_NARROW32"], FF["FF_ONE_I64"] | FF["FF_NARROW16"] | FF["FF_PACK10"]
    assert sorted((e[5], e[2]) for e in ENTRIES) == sorted([(n16, r) for r in (16, 32, 8, 4)] + [(n32, r) for r in (16, 8, 4)] + [(packed, r) for r in (48, 24, 12)])
    assert all(e[:2] == ("fused_filter_compact", 1) and e[3:5] == (2, WAVES) for e in ENTRIES)


@pytest.mark.parametrize("entry", ENTRIES, ids=[helpers.kernel_name(e) for e in ENTRIES])
def test_overflow_rerun_by_the_plain_twin(entry):
    r, flags = entry[2], entry[5]
    is_packed = bool(flags & FF["FF_PACK10"])
    # the companion the entry reads: 10-bit codes packed (a range below 1024, option narrow_codes = 2), 2-byte codes (a range below 65536)
    # or 4-byte codes (a wider one)
    top = 999 if is_packed else (9999 if flags & FF["FF_NARROW16"] else 99999)
    n = 2 * WAVES * 64 * r + 77  # two whole tiles and a ragged third
    v = np.random.default_rng(r + flags).integers(0, top + 1, n, dtype=np.int64)
    v[0], v[n - 1], v[n - 2] = top, top, 0
    # out_sizing = 2 gives outputs of two rows per million + 1024: 10 % survive where that is more than twice as many, 40 % of the
    # few thousand rows of the small geometries
    lit = top - top // 10 if n >= 20000 else top - 4 * (top // 10)
    pred = Predicate([Term(0, ">", lit)])
    want = v[v > lit]
    assert len(want) > 2 * 1024
    ctx = capi.Context(0)
    try:
        ctx.set_option("narrow_codes", 2 if is_packed else 1)
        d = ctx.upload(Column.from_numpy(v))  # (the whole buffer: a packed view starts on a 384-row super-group)
        _, rows, _ = ctx.filter_project([d], Predicate([Term(0, "<", 0)]), [0])  # the whole scan that builds the companion
        assert rows == 0 and ctx.get_option("narrow_builds") == 1
        reruns = ctx.get_option("overflow_reruns")
        ctx.set_option("rows_per_lane", r | WAVES << 8)
        ctx.set_option("out_sizing", 2)
        outs, rows, _ = ctx.filter_project([d], pred, [0])
        assert ctx.last_kernel() == helpers.kernel_name(entry)
        assert ctx.get_option("overflow_reruns") == reruns + 1
        got = outs[0].download()
        assert rows == len(want) == got.length and got.logical_valid() is None
        assert np.array_equal(got.logical_values(), want)
    finally:
        ctx.close()
