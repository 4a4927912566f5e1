"""Model of the outer, semi and anti hash joins (rv_join_kind of include/rivulus_gpu.h), in plain Python for the tests.

The reference has the inner join only (its enum stops at Inner), so this file is the executable definition of the other kinds,
as tests/sort_model.py is for the sort.  It is built on join_model.any_key: key equality is AnyValue's -- Null meets Null, NaN meets
nothing, +0.0 and -0.0 are two keys, values of different dtypes never meet.  tests/golden/outer_join_cases.json holds hand-written
cases with literal expected outputs that check this model as well as the device.

Pairs are (probe_idx, build_idx) with None for "no partner"; a frame is a list of (name, dtype, cells)."""
from join_model import any_key

INNER, PROBE_OUTER, FULL_OUTER, PROBE_SEMI, PROBE_ANTI = range(5)
KINDS = (INNER, PROBE_OUTER, FULL_OUTER, PROBE_SEMI, PROBE_ANTI)
KIND_NAMES = {INNER: "inner", PROBE_OUTER: "outer", FULL_OUTER: "full", PROBE_SEMI: "semi", PROBE_ANTI: "anti"}


def join_pairs(kind: int, build_dtype: int, build_keys, probe_dtype: int, probe_keys):
    """The rows of a join of `kind`, in the order the header fixes: probe-row order, build rows ascending within a probe row, an
    unmatched probe row as (p, None) at its place (PROBE_OUTER, FULL_OUTER); then (None, b) for every build row no probe row met,
    ascending (FULL_OUTER).  PROBE_SEMI / PROBE_ANTI: (p, None) for the kept probe rows, ascending."""
    table = {}
    for r, x in enumerate(build_keys):
        k = any_key(build_dtype, x)
        if k is not None:
            table.setdefault(k, []).append(r)
    met = set()
    pairs = []
    for p, x in enumerate(probe_keys):
        k = any_key(probe_dtype, x)
        rows = table.get(k, ()) if k is not None else ()
        if kind == PROBE_SEMI:
            if rows:
                pairs.append((p, None))
        elif kind == PROBE_ANTI:
            if not rows:
                pairs.append((p, None))
        else:
            for b in rows:
                pairs.append((p, b))
            met.update(rows)
            if not rows and kind in (PROBE_OUTER, FULL_OUTER):
                pairs.append((p, None))
    if kind == FULL_OUTER:
        pairs.extend((None, b) for b in range(len(build_keys)) if b not in met)
    return pairs


def output_names(kind: int, probe_frame, build_frame, build_key: str):
    """join_output_fields' rule, extended: the probe names, then the build names -- without the key, except for FULL_OUTER, which
    keeps it at its place -- with `_right` on a build name the probe frame also has; a semi or anti join has the probe names only."""
    names = [name for name, _, _ in probe_frame]
    if kind in (PROBE_SEMI, PROBE_ANTI):
        return names
    probe_names = set(names)
    for name, _, _ in build_frame:
        if name == build_key and kind != FULL_OUTER:
            continue
        names.append(f"{name}_right" if name in probe_names else name)
    return names


def materialize_kind(kind: int, probe_frame, build_frame, build_key: str, pairs):
    """The output frame of rv_hash_join_kind: a cell of the side without a partner is null."""
    take = lambda cells, idx: [None if i is None else cells[i] for i in idx]
    pi = [p for p, _ in pairs]
    bi = [b for _, b in pairs]
    cols = [(dtype, take(cells, pi)) for _, dtype, cells in probe_frame]
    if kind not in (PROBE_SEMI, PROBE_ANTI):
        cols += [(dtype, take(cells, bi)) for name, dtype, cells in build_frame if name != build_key or kind == FULL_OUTER]
    names = output_names(kind, probe_frame, build_frame, build_key)
    assert len(names) == len(cols)
    return [(n, d, c) for n, (d, c) in zip(names, cols)]


# ---- the hand-written cases of tests/golden/outer_join_cases.json ---------------------------------------------------------------
def load_golden_cases():
    """The cases with their frames as (name, dtype code, cells) and "NaN" strings of Float64 columns as NaNs."""
    import json
    import os
    from rivulus_amd.capi import RV_BOOLEAN, RV_FLOAT64, RV_INT64, RV_NULL, RV_STRING
    codes = {"i64": RV_INT64, "f64": RV_FLOAT64, "bool": RV_BOOLEAN, "str": RV_STRING, "null": RV_NULL}

    def frame(cols):
        out = []
        for name, dtype, cells in cols:
            if dtype == "f64":
                cells = [float("nan") if c == "NaN" else (None if c is None else float(c)) for c in cells]
            out.append((name, codes[dtype], cells))
        return out

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outer_join_cases.json")) as f:
        raw = json.load(f)["cases"]
    cases = []
    for c in raw:
        pairs = {}
        for kind in KINDS:
            got = c["pairs"][KIND_NAMES[kind]]
            pairs[kind] = [(p, None) for p in got] if kind in (PROBE_SEMI, PROBE_ANTI) else [tuple(x) for x in got]
        frames = {kind: frame(c["frames"][KIND_NAMES[kind]]) for kind in KINDS if KIND_NAMES[kind] in c.get("frames", {})}
        cases.append({"name": c["name"], "build": frame(c["build"]), "build_key": c["build_key"], "probe": frame(c["probe"]),
                      "probe_key": c["probe_key"], "pairs": pairs, "frames": frames})
    return cases
