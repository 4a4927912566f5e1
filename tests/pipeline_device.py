"""The device side of the pipeline tests: the steps of tests/pipeline_model.py through the library's calls, every step consuming the
device columns the step before it wrote.  Hands-off by construction: nothing here calls info() or null_count() on a column (the row
count is carried along from the calls' own results); inspect() is the one place that looks, and the caller decides whether it runs."""
import ctypes as C

import numpy as np

import pipeline_model as pm
from helpers import const
from rivulus_amd import capi
from rivulus_amd.capi import DeviceColumn, Predicate, Term, pack_bits


def to_host(col):
    """pipeline_model.to_host, with a String column's bitmap attached whenever the model column has one (all valid included)."""
    c = pm.to_host(col)
    if col[0] == "str" and col[2] is not None and c.validity is None:
        c.validity = pack_bits(col[2])
    return c


def upload_frame(ctx, src, tmp_path=None):
    """The device columns of a source of tests/pipeline_cases.py: (columns, rows, what to close afterwards)."""
    n = pm.rows(src["frame"])
    if src["how"] == "csv":
        path = tmp_path / "source.csv"
        path.write_text(src["text"], encoding="utf-8")
        reader = ctx.csv_open(str(path), [pm.RV[c[0]] for c in src["frame"]], batch_rows=n + 7, nulls_as_reference=src["ref"])
        return reader.next_batch(), n, reader
    if src["how"] == "slice":
        return [ctx.upload(to_host(c)).slice(src["pad"], n) for c in src["padded"]], n, None
    return [ctx.upload(to_host(c)) for c in src["frame"]], n, None


def compare(ctx, col, op, literal):
    """Context.compare without its look at the column's dtype (literals here are Int64 / Float64)."""
    _p, keep = Predicate([Term(0, op, literal)]).as_struct()
    t = keep[0][0]
    out = C.c_void_p()
    capi._check(capi.load().rv_compare(ctx.handle, col.handle, t.op, t.lit_type, t.lit.i if t.lit_type != capi.RV_FLOAT64 else 0,
                                       t.lit.f if t.lit_type == capi.RV_FLOAT64 else 0.0, C.byref(out)))
    return DeviceColumn(ctx, out)


JOIN_KIND = {"outer": capi.RV_JOIN_PROBE_OUTER, "full": capi.RV_JOIN_FULL_OUTER, "semi": capi.RV_JOIN_PROBE_SEMI, "anti": capi.RV_JOIN_PROBE_ANTI}


def join_chunked(ctx, build, bk, probe, pk, n, chunk, kind=None):
    """rv_hash_join_chunked (kind: rv_hash_join_chunked_kind) over the whole probe frame of n rows: (output columns, rows)."""
    k = (n + chunk - 1) // chunk
    nout = capi.join_output_columns(kind or capi.RV_JOIN_INNER, len(probe), len(build))
    table = ctx.join_build(build[bk])
    out = (C.c_void_p * max(1, nout))()
    per_batch = np.zeros(max(1, k), np.uint64)
    total, taken = C.c_uint64(), C.c_uint64()
    head = (ctx.handle, table.handle, capi._handles(build), len(build), bk, capi._handles(probe), len(probe), pk)
    tail = (chunk, 0, out, per_batch.ctypes.data_as(capi._U64P), k, None, C.byref(total), C.byref(taken))
    try:
        if kind is None:
            capi._check(capi.load().rv_hash_join_chunked(*head, *tail))
        else:
            capi._check(capi.load().rv_hash_join_chunked_kind(*head, kind, *tail))
    finally:
        table.free()
    assert taken.value == k and int(per_batch[:k].sum()) == total.value
    return [DeviceColumn(ctx, C.c_void_p(out[i])) for i in range(nout)], total.value


def _mask(ctx, frame, step):
    masks = [compare(ctx, frame[int(c)], op, lit) for c, op, lit in step["terms"]]

    def ev(tree):
        if isinstance(tree, int):
            return masks[tree]
        op, *args = tree
        if op == "not":
            return ctx.boolean_not(ev(args[0]))
        vals = [ev(a) for a in args]
        acc = vals[0]
        for v in vals[1:]:
            acc = (ctx.boolean_and if op == "and" else ctx.boolean_or)(acc, v)
        return acc

    expr = step.get("expr")
    return ev(pm.tup(expr) if expr is not None else ("and", *range(len(masks))) if len(masks) > 1 else 0)


def _top_k(ctx, step, frame, n, model_frame):
    """rv_top_k, or rv_top_k_indices over the first key and take_device; then the context's account of the call against
    topk_model.select over the model's key column (tests/test_topk_gpu.py, assert_path): the proof that the select ran, or did not."""
    k = pm.topk_k(step, n)
    keys = pm.topk_keys(step)
    if step.get("select"):
        ctx.set_option("top_k_select_from_rows", 1)
    try:
        want = None if model_frame is None else pm.topk_select(step, model_frame, ctx.get_option("top_k_select_from_rows") or const("kTopKSelectFromRows"),
                                                               ctx.get_option("top_k_refine_divisor") or const("kTopKRefineDivisor"))
        if step.get("via") == "indices":
            outs = ctx.take_device(frame, ctx.top_k_indices(frame[keys[0][0]], k, flags=keys[0][1]))
        else:
            outs = ctx.top_k(frame, keys, k)
        got = (ctx.get_option("top_k_last_passes"), ctx.get_option("top_k_last_candidates"))
    finally:
        if step.get("select"):
            ctx.set_option("top_k_select_from_rows", 0)
    assert want is None or got == (want.passes, want.count), f"top-k over {n} rows, k {k}, keys {keys}: (passes, candidates) {got}, the model's select says {(want.passes, want.count)}"
    return outs, min(k, n)


def run_step(ctx, step, frame, n, dtypes, build=None, model_frame=None):
    """(output columns, rows) of one step over the device columns `frame` of n rows and model dtypes `dtypes`.  model_frame: the model's
    input frame of the step, which a top-k step's path check reads (None: the check is left out)."""
    kind = step["kind"]
    if kind == "window":
        cols, part, dicts = list(frame), [], []
        try:  # (the context is shared: a call that raises leaves no dictionary behind)
            for c in step["partition_by"]:
                if dtypes[c] == "str":
                    sdict, ids = ctx.string_dict_build(frame[c])
                    dicts.append(sdict)
                    cols.append(ids)
                    c = len(cols) - 1
                part.append(c)
            outs = ctx.window(cols, part, [(int(c), int(f)) for c, f in step["order_by"]], [tuple(e) for e in step["exprs"]])
        finally:
            for sdict in dicts:
                sdict.free()
        return list(frame) + outs, n
    if kind == "topk":
        return _top_k(ctx, step, frame, n, model_frame)
    if kind == "outer_join":
        cols, m = build
        probe, pk, bcols, bk = pm.join_sides(frame, step, cols)
        if step.get("chunked"):
            return join_chunked(ctx, bcols, bk, probe, pk, m if step.get("side") == "build" else n, pm.JOIN_CHUNK, JOIN_KIND[step["how"]])
        return ctx.hash_join(bcols, bk, probe, pk, kind=JOIN_KIND[step["how"]])
    if kind == "group_keys":
        keys, dicts = [], []
        try:
            for c in step["keys"]:
                if dtypes[c] == "str":
                    sdict, ids = ctx.string_dict_build(frame[c])
                    dicts.append(sdict)
                    keys.append(ids)
                else:
                    keys.append(frame[c])
            outs, first, groups = ctx.hash_aggregate_keys(keys, frame, [(op, c) for op, c in step["specs"]])
        finally:
            for sdict in dicts:
                sdict.free()
        for j, c in enumerate(step["keys"]):
            if dtypes[c] == "str":
                outs[j] = ctx.take_device([frame[c]], first)[0]
        return outs, groups
    if kind == "filter":
        outs, rows, sel = ctx.filter_project(frame, pm.predicate_of(step), list(range(len(frame))), step.get("via") == "selection")
        if sel is not None:
            outs = ctx.take_device(frame, ctx.selection_indices(sel))
        return outs, rows
    if kind == "mask":
        return ctx.filter(frame, _mask(ctx, frame, step))
    if kind == "arith":
        return list(frame) + [ctx.eval_arith(frame, pm.tup(step["tree"]))], n
    if kind == "join":
        cols, m = build
        probe, pk, bcols, bk = pm.join_sides(frame, step, cols)
        if step.get("chunked"):
            return join_chunked(ctx, bcols, bk, probe, pk, m if step.get("side") == "build" else n, pm.JOIN_CHUNK)
        return ctx.hash_join(bcols, bk, probe, pk)
    if kind == "group":
        key, specs = frame[step["key"]], [(op, c) for op, c in step["specs"]]
        if dtypes[step["key"]] != "str":
            outs, _, groups = ctx.hash_aggregate(key, frame, specs, want_first_row=False)
            return outs, groups
        sdict, ids = ctx.string_dict_build(key)
        try:
            outs, first, groups = ctx.hash_aggregate(ids, frame, specs)
        finally:
            sdict.free()
        return ctx.take_device([key], first) + outs[1:], groups
    if kind == "sort":
        keys = [(int(c), int(f)) for c, f in step["keys"]]
        if step.get("via") != "chain":
            return ctx.sort(frame, keys), n
        perm = None
        for c, f in reversed(keys):
            perm = ctx.sort_indices(frame[c], flags=f, prior=perm)
        return ctx.take_device(frame, perm), n
    assert kind == "reshape"
    how = step["how"]
    if how == "slice":
        off, length = pm.slice_bounds(n, step)
        return [c.slice(off, length) for c in frame], length
    if how == "concat":
        h = n * step["eighths"] // 8
        return [ctx.concat([c.slice(h, n - h), c.slice(0, h)]) for c in frame], n
    if how == "take_first":
        _, first, groups = ctx.group_ids(frame[step["col"]])
        return ctx.take_device(frame, first), groups
    assert how == "take_sorted"
    return ctx.take_device(frame, ctx.sort_indices(frame[step["col"]], flags=step["flags"])), n


def download(frame):
    return [pm.from_host(c.download()) for c in frame]


def inspect(frame, want, meta, what):
    """Every column of a device frame against the model's: metadata first (length, dtype, offset, a null count the column already
    claims to know, the bitmap where the header states a rule), then the cells, then null_count()."""
    assert len(frame) == len(want), f"{what}: {len(frame)} columns != {len(want)}"
    for j, (d, w, m) in enumerate(zip(frame, want, meta)):
        where = f"{what} column {j} ({w[0]})"
        i = d.info()
        nulls = pm.null_count(w)
        assert pm.DTYPE_OF_RV[i.dtype] == w[0], f"{where}: dtype {i.dtype}"
        assert i.length == len(w[1]), f"{where}: length {i.length} != {len(w[1])}"
        if m["offset"] is not None:
            assert i.offset == m["offset"], f"{where}: offset {i.offset} != {m['offset']}"
        assert i.null_count in (-1, nulls), f"{where}: the column claims {i.null_count} nulls, it has {nulls}"
        if m["bitmap"] is not None:
            assert bool(i.has_validity) == m["bitmap"], f"{where}: has_validity {i.has_validity}, the header's rule says {m['bitmap']} ({nulls} nulls)"
        diff = pm.column_diff(pm.from_host(d.download()), w)
        assert diff is None, f"{where}: {diff}"
        assert d.null_count() == nulls, f"{where}: null_count() {d.null_count()} != {nulls}"


def run_pipeline(ctx, source, steps, builds, model, build_models, look, what, tmp_path=None):
    """The pipeline on the device.  look=False: hands-off, only the final frame is downloaded; look=True: inspect() after the source and
    after every step.  Either way the final frame must be the model's.  source / builds[k]["source"]: sources of pipeline_cases;
    model / build_models: pipeline_model.run_case's intermediates.  Returns the final device frame."""
    closers = []
    try:
        built = {}
        for k, b in builds.items():
            cols, m, closer = upload_frame(ctx, b["source"], tmp_path)
            closers.append(closer)
            inter = build_models[k]
            for s, bstep in enumerate(b["steps"]):
                cols, m = run_step(ctx, bstep, cols, m, pm.dtypes(inter[s][0]), None, inter[s][0])
                if look:
                    inspect(cols, inter[s + 1][0], inter[s + 1][1], f"{what} join step {k}, build side step {s} ({bstep['kind']})")
            built[k] = (cols, m)
        frame, n, closer = upload_frame(ctx, source, tmp_path)
        closers.append(closer)
        if look:
            inspect(frame, model[0][0], model[0][1], f"{what} source ({source['how']})")
        for k, step in enumerate(steps):
            where = f"{what} step {k} ({step['kind']}{' ' + step['how'] if 'how' in step else ''})"
            try:
                frame, n = run_step(ctx, step, frame, n, pm.dtypes(model[k][0]), built.get(k), model[k][0])
            except capi.RvError as e:
                raise AssertionError(f"{where}: {e}") from e
            assert n == pm.rows(model[k + 1][0]), f"{where}: {n} rows != {pm.rows(model[k + 1][0])}"
            if look:
                inspect(frame, model[k + 1][0], model[k + 1][1], where)
        diff = pm.frame_diff(download(frame), model[-1][0])
        assert diff is None, f"{what} final frame after {[s['kind'] for s in steps]} ({'inspected' if look else 'hands-off'}): {diff}"
        return frame
    finally:
        for c in closers:
            if c is not None:
                c.close()
