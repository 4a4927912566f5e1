"""What keeps tests/test_pipeline_ops_gpu.py from being vacuous, on a machine without a device: conditions on the second generator
(pipeline_cases.case_ops: window, top-k, outer / semi / anti joins and multi-key grouping among the older kinds), each over its 216
default seeds and on the model alone; the composed model against pipelines worked out by hand (tests/golden/pipeline_ops_cases.json);
and the digest that pins the first generator's 200 cases."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest

import pipeline_cases as pc
import pipeline_model as pm
from helpers import const

N_CASES = pc.N_CASES_OPS  # the default of tests/test_pipeline_ops_gpu.py: the assertions below are about that set
STATES = ("null_count_unknown", "bitmap_no_nulls", "all_null", "zero_rows")
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pipeline_ops_cases.json")
DIGEST = os.path.join(HERE, "golden", "pipeline_cases_digest.json")


# ---- the first generator is what it was ----------------------------------------------------------------------------------------------
def _hash_column(h, col):
    dtype, values, valid = col
    h.update(dtype.encode())
    h.update(json.dumps(values, ensure_ascii=True).encode() if dtype == "str" else np.ascontiguousarray(values).tobytes())
    h.update(b"-" if valid is None else np.ascontiguousarray(valid, bool).tobytes())


def _hash_source(h, src):
    h.update(json.dumps([src["how"], src["pad"], src["ref"]]).encode())
    for col in list(src["frame"]) + list(src["padded"]):
        _hash_column(h, col)


def cases_digest(n):
    """SHA-256 over case(0) .. case(n - 1): the JSON of the steps and, per source and build column (the logical frame and what is
    uploaded before the slice), the dtype, the values' bytes and the validity bytes."""
    h = hashlib.sha256()
    for seed in range(n):
        c = pc.case(seed)
        h.update(json.dumps([c["seed"], c["n"], c["steps"]]).encode())
        _hash_source(h, c["source"])
        for k in sorted(c["builds"]):
            h.update(json.dumps([k, c["builds"][k]["steps"]]).encode())
            _hash_source(h, c["builds"][k]["source"])
    return h.hexdigest()


def test_the_first_generator_is_unchanged():
    with open(DIGEST, encoding="utf-8") as f:
        want = json.load(f)
    assert pm.KINDS == ("filter", "mask", "arith", "join", "group", "sort", "reshape")
    assert cases_digest(want["cases"]) == want["sha256"], "pipeline_cases.case() no longer generates the cases it did"


# ---- the second generator --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    """[(case, intermediates, build intermediates, padded marks)] of the default seeds: the model alone."""
    out = []
    for seed in range(N_CASES):
        case = pc.case_ops(seed)
        inter, builds = pm.run_case(case)
        out.append((case, inter, builds, pm.padded_run(case, inter, builds)))
    return out


def test_cases_are_deterministic_and_sized():
    a, b = pc.case_ops(17), pc.case_ops(17)
    assert a["steps"] == b["steps"] and pm.frame_diff(a["source"]["frame"], b["source"]["frame"]) is None
    assert len(pc.PAIRS_OPS) == 72 and N_CASES == 3 * 72 and len(set(pc.PAIRS_OPS)) == 72
    assert all(a in pm.NEW_KINDS or b in pm.NEW_KINDS for a, b in pc.PAIRS_OPS)
    sizes = collections.Counter()
    hows = collections.Counter()
    for seed in range(N_CASES):
        c = pc.case_ops(seed)
        assert 2 <= len(c["steps"]) <= 5 and 2 <= len(c["source"]["frame"]) <= 6
        assert json.loads(json.dumps(c["steps"])) == json.loads(json.dumps(pm.tup(c["steps"]))), "a step list is JSON"
        sizes[c["n"]] += 1
        hows[c["source"]["how"], c["source"]["ref"]] += 1
    assert set(pc.SIZES) | {pc.LARGE} <= set(sizes), sizes
    assert 3 <= sizes[pc.LARGE] <= 8 and max(sizes) == pc.LARGE  # as rarely as in the first set
    assert min(hows["upload", False], hows["slice", False], hows["csv", False], hows["csv", True]) >= 5, hows


def test_every_new_kind_follows_and_feeds_every_kind(runs):
    pairs = collections.Counter()
    for case, *_ in runs:
        kinds = [s["kind"] for s in case["steps"]]
        pairs.update(set(zip(kinds, kinds[1:])))
    thin = {p: pairs[p] for p in pc.PAIRS_OPS if pairs[p] < 3}
    assert not thin, f"(producer, consumer) pairs with fewer than 3 cases: {thin}"
    print("cases per pair: min", min(pairs[p] for p in pc.PAIRS_OPS), "max", max(pairs[p] for p in pc.PAIRS_OPS))


def _inputs(case, inter, builds, k):
    """[(column, meta)] the device calls of step k read, the second frame of a join included"""
    step = case["steps"][k]
    frame, meta = inter[k]
    cols = [(frame[j], meta[j]) for j in pm.touched(step, frame)]
    if step["kind"] in pm.JOINS:
        cols += list(zip(*builds[k][-1]))
    return cols


def _state_counts(runs, first_step, made_only):
    """{(consumer kind, state): cases} over the steps from `first_step` on; made_only: only input columns an operator wrote count"""
    seen = collections.Counter()
    for case, inter, builds, _ in runs:
        found = set()
        for k, step in enumerate(case["steps"]):
            if k < first_step:
                continue
            for c, m in _inputs(case, inter, builds, k):
                if m["made"] or not made_only:
                    found |= {(step["kind"], s) for s in pm.column_states(c, m)}
        seen.update(found)
    return seen


def test_every_new_consumer_sees_every_irregular_input(runs):
    """tests/test_pipeline_cpu.py's three counts (every step; the steps behind the first; there the columns an operator wrote alone, without
    null_count_unknown for the reason given there), each at least 3 CASES per (new consumer kind, state)."""
    for first_step, made_only, states in ((0, False, STATES), (1, False, STATES), (1, True, STATES[1:])):
        seen = _state_counts(runs, first_step, made_only)
        print(f"from step {first_step}, made_only={made_only}:", {f"{k}/{s}": seen[k, s] for k in pm.NEW_KINDS for s in states})
        thin = {(k, s): seen[k, s] for k in pm.NEW_KINDS for s in states if seen[k, s] < 3}
        assert not thin, f"(consumer, input state) with fewer than 3 cases from step {first_step} on, made_only={made_only}: {thin}"


def test_every_kind_consumes_a_padded_column(runs):
    """padded: the column holds a null that an "outer" or "full" join put there (pipeline_model.padded_after carries the marks)."""
    seen = collections.Counter()
    for case, inter, builds, pads in runs:
        found = set()
        for k, step in enumerate(case["steps"]):
            if any(pads[k][j].any() for j in pm.touched(step, inter[k][0])):
                found.add(step["kind"])
        seen.update(found)
    print("cases in which the kind reads a padded column:", dict(seen))
    thin = {k: seen[k] for k in pm.KINDS_ALL if seen[k] < 3}
    assert not thin, f"kinds that consume a padded column in fewer than 3 cases: {thin}"


def test_top_k_takes_every_arm(runs):
    """By topk_model.select with the library's own thresholds (a step with "select" runs with top_k_select_from_rows = 1)."""
    selected = made_nulls = whole = 0
    for case, inter, builds, _ in runs:
        for k, step in enumerate(case["steps"]):
            if step["kind"] != "topk":
                continue
            frame, meta = inter[k]
            s = pm.topk_select(step, frame, const("kTopKSelectFromRows"), const("kTopKRefineDivisor"))
            c = pm.topk_keys(step)[0][0]
            if s.selected and s.passes >= 1:
                selected += 1
                made_nulls += bool(meta[c]["made"] and 0 < pm.null_count(frame[c]))
            elif pm.topk_k(step, pm.rows(frame)) > 0 and pm.rows(frame) > 0:
                whole += 1
    print(f"top-k steps: select ran {selected}, of those over an operator-written first key with nulls {made_nulls}, whole sort {whole}")
    assert selected >= 12 and made_nulls >= 4 and whole >= 3, (selected, made_nulls, whole)


def test_every_join_kind_has_an_answer(runs):
    count, mixed = collections.Counter(), collections.Counter()
    for case, inter, builds, _ in runs:
        for k, step in enumerate(case["steps"]):
            if step["kind"] != "outer_join":
                continue
            assert not (step["how"] == "full" and step["chunked"]), "FULL_OUTER has no chunked form"
            probe, pk, build, bk = pm.join_sides(inter[k][0], step, builds[k][-1][0])
            pi, _ = pm.outer_join_indices(probe, pk, build, bk, "semi")
            count[step["how"]] += 1
            mixed[step["how"]] += 0 < len(pi) < pm.rows(probe)
    print("outer_join steps by how:", dict(count), "with matched and unmatched probe rows:", dict(mixed))
    for how in pc.HOWS:
        assert count[how] >= 8 and 2 * mixed[how] >= count[how], (how, count[how], mixed[how])


def test_degenerate_results_are_capped(runs):
    final = sum(pm.rows(inter[-1][0]) == 0 for _, inter, _, _ in runs)
    anywhere = sum(any(pm.rows(f) == 0 for f, _ in inter[1:]) for _, inter, _, _ in runs)
    print(f"{final} of {len(runs)} cases end with zero rows, {anywhere} have a zero-row intermediate")
    assert final <= 0.15 * len(runs), f"{final} of {len(runs)} cases end with a zero-row frame"
    assert anywhere <= 0.30 * len(runs), f"{anywhere} of {len(runs)} cases have a zero-row intermediate"


def test_float_sums_are_exact_in_any_order(runs):
    """tests/test_pipeline_cpu.py's condition for every Float64 column a SUM of `group` or `group_keys` or a CUM_SUM reads: multiples of
    2^SCALE whose absolute values add up to less than 2^53 * 2^SCALE, no special -- every partial sum of any order is representable."""
    checked = 0
    for case, inter, builds, _ in runs:
        pipelines = [(case["steps"], inter)] + [(case["builds"][k]["steps"], builds[k]) for k in builds]
        for steps, frames in pipelines:
            for k, step in enumerate(steps):
                if step["kind"] in ("group", "group_keys"):
                    read = [c for op, c in step["specs"] if op == "sum"]
                elif step["kind"] == "window":
                    read = [e[1] for e in step["exprs"] if e[0] == "cum_sum"]
                else:
                    continue
                for c in read:
                    col = frames[k][0][c]
                    if col[0] != "f64":
                        continue
                    cells = np.asarray(col[1])[pm.valid_of(col)]
                    assert np.isfinite(cells).all(), f"seed {case['seed']} step {k}"
                    scaled = np.ldexp(cells, -pc.SCALE)
                    assert (scaled == np.round(scaled)).all() and np.abs(scaled).sum() < 2.0 ** 53, f"seed {case['seed']} step {k}"
                    checked += 1
    assert checked >= 5


# ---- directed pipelines -------------------------------------------------------------------------------------------------------------------
IDENTITIES = ("row_number_inverts_the_sort", "gids_as_partition_key", "lag_of_strings_into_dictionary_join", "semi_plus_anti_is_the_probe_frame")
EXTRA = ("group_keys_string_and_nan_key",)  # a String key and a NaN / -0.0 / +0.0 key of group_keys: no directed pipeline's own
SAME_FIELDS = ("how", "side", "chunked", "via", "select", "nulls", "offset")  # what a toy's step shares with its directed pipeline's

with open(GOLDEN, encoding="utf-8") as _f:
    _GOLDEN = json.load(_f)


def _frame(cols):
    """A golden frame: a name of the file's `frames`, or columns, a name among them standing for that frame's columns."""
    if isinstance(cols, str):
        cols = _GOLDEN["frames"][cols]
    out = []
    for c in cols:
        out += _frame(c) if isinstance(c, str) else [pm.column_of(*c)]
    return out


def _steps(steps, name):
    """Golden steps: a name of the file's `steps`, [name, {fields replaced}], or the step itself; "AT" slices at the offset `name` ends in."""
    out = []
    for s in steps:
        if isinstance(s, list):
            s = dict(_GOLDEN["steps"][s[0]], **s[1])
        elif isinstance(s, str):
            s = dict(_GOLDEN["steps"][s], **({"offset": int(name.rsplit("_", 1)[1])} if s == "AT" else {}))
        out.append(s)
    return out


def _toys():
    """[(id, directed name, case)] of the golden file: a case with several names once under each"""
    out = []
    for c in _GOLDEN["cases"]:
        for name in c["name"] if isinstance(c["name"], list) else [c["name"]]:
            out.append((name + ("-" + c["part"] if "part" in c else ""), name, c))
    return out


TOYS = _toys()


def _run_toy(name, case):
    """(steps, every intermediate frame) of a toy through the composed model"""
    builds = {}
    for k, b in case.get("builds", {}).items():
        b = _GOLDEN["frames"][b] if isinstance(b, str) else b
        b = b if isinstance(b, dict) else {"frame": b, "steps": []}
        frame = _frame(b["frame"])
        assert pm.rows(frame) <= 12
        builds[int(k)] = pm.run((frame, pm.source_meta(frame)), _steps(b["steps"], name))
    frame = _frame(case["frame"])
    assert pm.rows(frame) <= 12
    steps = _steps(case["steps"], name)
    return steps, [f for f, _ in pm.run((frame, pm.source_meta(frame)), steps, builds)]


def _flags(step):
    return [f for _, f in step["keys"]] if step["kind"] in ("topk", "sort") else None


@pytest.mark.parametrize("name, case", [t[1:] for t in TOYS], ids=[t[0] for t in TOYS])
def test_model_reproduces_the_hand_written_pipelines(name, case):
    """The composed model gives the frame written out by hand; and the toy is its directed pipeline's: the same kinds of steps in the
    same order, with the same join kind, side and chunking, top-k path, slice offset, null policy and key flag words."""
    steps, frames = _run_toy(name, case)
    diff = pm.frame_diff(frames[-1], _frame(case["expected"]))
    assert diff is None, f"{name}: {diff}"
    if name in pc.DIRECTED_OPS:
        directed = pc.directed_ops(name, 12)[1]
        assert [s["kind"] for s in steps] == [s["kind"] for s in directed]
        for toy, big in zip(steps, directed):
            assert {f: toy.get(f) for f in SAME_FIELDS if f in big} == {f: big[f] for f in SAME_FIELDS if f in big}, (name, toy, big)
            assert _flags(toy) == _flags(big), (name, toy, big)


def test_golden_file_holds_every_directed_pipeline():
    """Every name of pipeline_cases.DIRECTED_OPS and every identity of tests/test_pipeline_ops_gpu.py has a hand-written toy under its own
    name, nothing else is in the file but EXTRA, and the file stays small."""
    names = collections.Counter(name for _, name, _ in TOYS)
    assert set(names) == set(pc.DIRECTED_OPS) | set(IDENTITIES) | set(EXTRA), set(names) ^ (set(pc.DIRECTED_OPS) | set(IDENTITIES) | set(EXTRA))
    assert len(set(pc.DIRECTED_OPS)) == len(pc.DIRECTED_OPS) == 56
    assert all(n == (2 if name == "semi_plus_anti_is_the_probe_frame" else 1) for name, n in names.items()), names
    assert os.path.getsize(GOLDEN) <= 16 * 1024


def _toy(name, part=None):
    (found,) = [(n, c) for _, n, c in TOYS if n == name and c.get("part") == part]
    return _run_toy(*found)


def test_row_number_inverts_the_sort_on_the_model():
    """The identity of the GPU test of this name, on the hand-written toy: take(sorted frame, row_number - 1) is the source frame."""
    steps, frames = _toy("row_number_inverts_the_sort")
    ordered = pm.step_sort(frames[0], {"keys": steps[0]["order_by"]})
    place = frames[-1][-1]
    assert sorted(place[1].tolist()) == list(range(pm.rows(frames[0]))) and pm.null_count(place) == 0
    assert pm.frame_diff(pm.take_frame(ordered, place[1]), frames[0]) is None


def test_gids_as_partition_key_on_the_model():
    """The gids of the key tuple as the single partition key give the window columns partition_by = keys gives, and MAX of ROW_NUMBER
    per group is COUNT_ROWS."""
    steps, frames = _toy("gids_as_partition_key")
    source, keys, n = frames[0], steps[0]["partition_by"], len(frames[0])
    gids = pm.group_keys_result(source, {"keys": keys, "specs": [("count_rows", None)]})["gids"]
    assert len(set(gids.tolist())) == 3
    by_gids = pm.step_window(source + [("i64", np.asarray(gids, np.int64), None)], dict(steps[0], partition_by=[n]))
    assert pm.frame_diff(by_gids[n + 1:], frames[-1][n:]) is None
    got = pm.step_group_keys(frames[-1], {"keys": keys, "specs": [("max", n), ("count_rows", None)]})
    assert pm.column_diff(got[-2], got[-1]) is None and got[-1][1].tolist() == [2, 1, 1]


def test_lag_of_strings_into_dictionary_join_on_the_model():
    """The sliced LAG column's dictionary ids and the PROBE_OUTER join over them, against the cells written out by hand."""
    _, case = [(n, c) for _, n, c in TOYS if n == "lag_of_strings_into_dictionary_join"][0]
    _, frames = _toy("lag_of_strings_into_dictionary_join")
    lagged = frames[-1][-1]
    ids = pm.string_ids(lagged)
    assert pm.column_diff(ids, pm.column_of(*case["ids"])) is None
    step = {"kind": "outer_join", "how": "outer", "probe_key": 0, "build_key": 0, "side": "probe"}
    assert pm.frame_diff(pm.step_outer_join([ids, lagged], step, _frame(case["other"])), _frame(case["joined"])) is None


def test_semi_plus_anti_is_the_probe_frame_on_the_model():
    """The two hand-written outputs, concatenated and sorted by the row-number column, are the probe frame (the null quotients and the
    genuine 0 on the SEMI side: the build side holds key 0 and a null key)."""
    (_, semi), (_, anti) = _toy("semi_plus_anti_is_the_probe_frame", "semi"), _toy("semi_plus_anti_is_the_probe_frame", "anti")
    assert pm.frame_diff(semi[1], anti[1]) is None
    both = [pm.column_of(a[0], pm.cells(a) + pm.cells(b)) for a, b in zip(semi[-1], anti[-1])]
    assert pm.frame_diff(pm.step_sort(both, {"keys": [(2, 0)]}), semi[1]) is None


def test_directed_pipelines_run_through_the_model_at_toy_size():
    for name in pc.DIRECTED_OPS:
        case = pc.directed_ops_case(name, 12)
        inter, _ = pm.run_case(case)
        assert len(inter) == len(case["steps"]) + 1
        pc.assert_point(name, case)
