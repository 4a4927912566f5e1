"""The device CSV reader through the Python binding (Context.csv_open -> rv_csv_open / rv_csv_next): argument errors,
rv_csv_reader_info, a context that stays usable after a parse error, and one scale case of 10^7 rows compared with a
Python restatement of the host CsvFileStream's batches."""
import os
import struct

import numpy as np
import pytest

from rivulus_amd import capi
from rivulus_amd.capi import RV_BOOLEAN, RV_FLOAT64, RV_INT64, RV_NULL, RV_STRING, RvError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with capi.Context(0) as c:
        yield c


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_bytes(text.encode() if isinstance(text, str) else text)
    return str(p)


def test_argument_errors(ctx, tmp_path):
    with pytest.raises(RvError) as e:
        ctx.csv_open(str(tmp_path / "missing.csv"), [RV_INT64])
    assert e.value.status == capi.RV_ERR_INVALID_ARG and e.value.message == "Failed to open file: No such file or directory"
    p = _write(tmp_path, "a.csv", "a\n1\n")
    with pytest.raises(RvError) as e:
        ctx.csv_open(p, [RV_NULL])
    assert e.value.status == capi.RV_ERR_UNSUPPORTED
    with pytest.raises(RvError) as e:
        ctx.csv_open(p, [7])
    assert e.value.status == capi.RV_ERR_INVALID_ARG
    lib = capi.load()
    arr = (capi.C.c_int * 1)(RV_INT64)
    out = capi.C.c_void_p()
    assert lib.rv_csv_open(ctx.handle, p.encode(), arr, 1, 300, 0, 0, 0, capi.C.byref(out)) == capi.RV_ERR_INVALID_ARG
    assert lib.rv_csv_open(ctx.handle, p.encode(), arr, 1, ord(","), 0, 4, 0, capi.C.byref(out)) == capi.RV_ERR_INVALID_ARG
    assert lib.rv_csv_open(ctx.handle, None, arr, 1, ord(","), 0, 0, 0, capi.C.byref(out)) == capi.RV_ERR_INVALID_ARG
    assert lib.rv_csv_next(None, None, None) == capi.RV_ERR_INVALID_ARG
    assert lib.rv_csv_reader_info(None, None, None, None) == capi.RV_ERR_INVALID_ARG
    assert lib.rv_status_name(capi.RV_ERR_PARSE) == b"RV_ERR_PARSE"


def test_reader_info_and_batches(ctx, tmp_path):
    p = _write(tmp_path, "b.csv", "a,b\n" + "".join(f"{i},{'x' * (i % 5)}\n" for i in range(10)) + "\n\n")
    with ctx.csv_open(p, [RV_INT64, RV_STRING], batch_rows=4) as r:
        assert r.info()[0] == 4
        sizes = []
        for b in r:
            sizes.append(b[0].length)
            assert b[0].length == b[1].length
        assert sizes == [4, 4, 2]
        rows, lines, read = r.info()
        assert rows == 4 and lines == 13 and read == os.path.getsize(p)
    # adaptive (calculate_adaptive_batch_size): 8 MiB / bytes per row, within [1000, 100000]
    with ctx.csv_open(p, [RV_INT64, RV_STRING]) as r:
        assert r.info()[0] == 100000
    with ctx.csv_open(p, [RV_STRING] * 3) as r:
        assert r.info()[0] == 8 * 1024 * 1024 // 96
    with ctx.csv_open(p, [RV_STRING] * 300) as r:
        assert r.info()[0] == 1000


def test_context_usable_after_a_parse_error(ctx, tmp_path):
    p = _write(tmp_path, "c.csv", "a,b\n1,true\nx2,false\n3,maybe\n4,t\n")
    r = ctx.csv_open(p, [RV_INT64, RV_BOOLEAN], batch_rows=10)
    with pytest.raises(RvError) as e:
        r.next_batch()
    assert e.value.status == capi.RV_ERR_PARSE and e.value.message == "Line 3, field 0: Cannot parse 'x2' as Int64"
    with pytest.raises(RvError) as e:
        r.next_batch()
    assert e.value.message == "Line 4, field 1: Cannot parse 'maybe' as Boolean"
    b = r.next_batch()
    assert b[0].length == 1 and list(b[0].download().logical_values()) == [4]
    assert r.next_batch() is None and r.next_batch() is None
    r.close()
    x = ctx.generate(capi.synth_spec(RV_INT64, seed=1, length=1000))  # the context still runs queries
    outs, rows, _ = ctx.filter_project([x], capi.Predicate([capi.Term(0, ">", 500)]), [0])
    assert 0 < rows < 1000


def _host_batches(n_rows, batch):
    """the host stream's batch sizes for a file without blank or bad lines"""
    return [min(batch, n_rows - s) for s in range(0, n_rows, batch)]


def test_ten_million_rows_against_the_host_rule(ctx, tmp_path):
    n = 10_000_000
    rng = np.random.default_rng(7)
    ints = rng.integers(-10**12, 10**12, n)
    floats = np.round(rng.standard_normal(n) * 1000, 3)
    bools = rng.integers(0, 2, n).astype(bool)
    null_i = rng.random(n) < 0.01
    p = str(tmp_path / "big.csv")
    with open(p, "w") as f:
        f.write("i,f,b\n")
        step = 1_000_000
        for s in range(0, n, step):
            e = min(n, s + step)
            si = np.where(null_i[s:e], "", ints[s:e].astype(str))
            sf = np.char.mod("%.3f", floats[s:e])
            sb = np.where(bools[s:e], "true", "false")
            f.write("\n".join(np.char.add(np.char.add(np.char.add(np.char.add(si, ","), sf), ","), sb)) + "\n")
    assert os.path.getsize(p) < 1 << 30
    batch = 1 << 20
    got = 0
    with ctx.csv_open(p, [RV_INT64, RV_FLOAT64, RV_BOOLEAN], batch_rows=batch, nulls_as_reference=False) as r:
        sizes = []
        for cols in r:
            k = cols[0].length
            ci, cf, cb = (c.download() for c in cols)
            want_null = null_i[got:got + k]
            vi = ci.logical_values()
            assert np.array_equal(vi[~want_null], ints[got:got + k][~want_null]) and np.all(vi[want_null] == 0)
            valid = ci.logical_valid()
            if want_null.any():
                assert valid is not None and np.array_equal(valid, ~want_null)
            else:
                assert valid is None
            want_f = np.array([float(x) for x in np.char.mod("%.3f", floats[got:got + k])])
            assert np.array_equal(cf.logical_values().view(np.uint64), want_f.view(np.uint64))
            assert np.array_equal(cb.logical_values().astype(bool), bools[got:got + k])
            sizes.append(k)
            got += k
    assert sizes == _host_batches(n, batch) and got == n
    os.remove(p)
