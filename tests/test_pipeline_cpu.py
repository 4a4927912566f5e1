"""What keeps tests/test_pipeline_gpu.py from being vacuous, on a machine without a device: the generated cases cover every
producer -> consumer pair and every irregular input state, stay clear of degenerate results, and the composed model of
tests/pipeline_model.py reproduces pipelines worked out by hand (tests/golden/pipeline_cases.json); every predicate the generator emits
keeps the same rows through helpers.host_survivors and through the C++ oracle."""
import collections
import json
import os

import numpy as np
import pytest

import pipeline_cases as pc
import pipeline_model as pm

N_CASES = 200  # the default of tests/test_pipeline_gpu.py: the assertions below are about that set
STATES = ("null_count_unknown", "bitmap_no_nulls", "all_null", "zero_rows")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_cases.json")


@pytest.fixture(scope="module")
def runs():
    """[(case, intermediates, build intermediates)] of the default seeds: the model alone."""
    out = []
    for seed in range(N_CASES):
        case = pc.case(seed)
        out.append((case, *pm.run_case(case)))
    return out


def test_cases_are_deterministic_and_sized():
    a, b = pc.case(17), pc.case(17)
    assert a["steps"] == b["steps"] and pm.frame_diff(a["source"]["frame"], b["source"]["frame"]) is None
    sizes = collections.Counter()
    hows = collections.Counter()
    for seed in range(N_CASES):
        c = pc.case(seed)
        assert 2 <= len(c["steps"]) <= 5 and 2 <= len(c["source"]["frame"]) <= 6
        sizes[c["n"]] += 1
        hows[c["source"]["how"], c["source"]["ref"]] += 1
    assert set(pc.SIZES) | {pc.LARGE} <= set(sizes), sizes
    assert 3 <= sizes[pc.LARGE] <= 8 and max(sizes) == pc.LARGE
    assert min(hows["upload", False], hows["slice", False], hows["csv", False], hows["csv", True]) >= 5, hows


def test_every_kind_follows_every_kind(runs):
    pairs = collections.Counter()
    for case, _, _ in runs:
        kinds = [s["kind"] for s in case["steps"]]
        pairs.update(zip(kinds, kinds[1:]))
    thin = {(a, b): pairs[a, b] for a in pm.KINDS for b in pm.KINDS if pairs[a, b] < 3}
    assert not thin, f"(producer, consumer) pairs with fewer than 3 cases: {thin}"


def _state_counts(runs, first_step, made_only):
    """{(consumer kind, state): cases} over the steps from `first_step` on; made_only: only input columns an operator wrote count"""
    seen = collections.Counter()
    for case, inter, builds in runs:
        for k, step in enumerate(case["steps"]):
            if k < first_step:
                continue
            frame, meta = inter[k]
            cols = [(frame[j], meta[j]) for j in pm.touched(step, frame)]
            if step["kind"] == "join":
                cols += list(zip(*builds[k][-1]))
            states = set()
            for c, m in cols:
                if m["made"] or not made_only:
                    states |= pm.column_states(c, m)
            seen.update((step["kind"], s) for s in states)
    return seen


def test_every_consumer_sees_every_irregular_input(runs):
    """Three counts, each at least 3 per (consumer kind, state): over every step; over the steps behind the first, whose inputs another
    step handed on; and there over the columns an operator WROTE alone (not an upload passed through).  The last leaves out
    null_count_unknown: every operator knows the count of what it writes, so only a slice of such a column is in that state, and the
    default seeds hold too few of those for every consumer (0 to 5)."""
    for first_step, made_only, states in ((0, False, STATES), (1, False, STATES), (1, True, STATES[1:])):
        seen = _state_counts(runs, first_step, made_only)
        thin = {(k, s): seen[k, s] for k in pm.KINDS for s in states if seen[k, s] < 3}
        assert not thin, f"(consumer, input state) with fewer than 3 cases from step {first_step} on, made_only={made_only}: {thin}"


def test_degenerate_results_are_capped(runs):
    final = sum(pm.rows(inter[-1][0]) == 0 for _, inter, _ in runs)
    anywhere = sum(any(pm.rows(f) == 0 for f, _ in inter[1:]) for _, inter, _ in runs)
    assert final <= 0.15 * len(runs), f"{final} of {len(runs)} cases end with a zero-row frame"
    assert anywhere <= 0.30 * len(runs), f"{anywhere} of {len(runs)} cases have a zero-row intermediate"


def test_float_sums_are_exact_in_any_order(runs):
    """Every Float64 column a generated SUM reads holds multiples of 2^SCALE whose absolute values add up to less than 2^53 * 2^SCALE, and
    no special: every partial sum of any reduction tree is then representable, which is what lets the GPU test compare bits."""
    for case, inter, builds in runs:
        pipelines = [(case["steps"], inter)] + [(case["builds"][k]["steps"], builds[k]) for k in builds]
        for steps, frames in pipelines:
            for k, step in enumerate(steps):
                if step["kind"] != "group":
                    continue
                for op, c in step["specs"]:
                    col = frames[k][0][c] if c is not None else None
                    if op == "sum" and col[0] == "f64":
                        cells = np.asarray(col[1])[pm.valid_of(col)]
                        assert np.isfinite(cells).all(), f"seed {case['seed']} step {k}"
                        scaled = np.ldexp(cells, -pc.SCALE)
                        assert (scaled == np.round(scaled)).all() and np.abs(scaled).sum() < 2.0 ** 53, f"seed {case['seed']} step {k}"


def _frame(cols):
    return [pm.column_of(d, cells) for d, cells in cols]


with open(GOLDEN, encoding="utf-8") as _f:
    GOLDEN_CASES = json.load(_f)["cases"]


@pytest.mark.parametrize("case", GOLDEN_CASES, ids=[c["name"] for c in GOLDEN_CASES])
def test_model_reproduces_the_hand_written_pipelines(case):
    assert pm.rows(_frame(case["frame"])) <= 12
    builds = {}
    for k, b in case["builds"].items():
        frame = _frame(b["frame"])
        builds[int(k)] = pm.run((frame, pm.source_meta(frame)), b["steps"])
    frame = _frame(case["frame"])
    got = pm.run((frame, pm.source_meta(frame)), case["steps"], builds)[-1][0]
    diff = pm.frame_diff(got, _frame(case["expected"]))
    assert diff is None, f"{case['name']}: {diff}"


def test_golden_file_holds_every_directed_edge():
    names = {c["name"] for c in GOLDEN_CASES}
    want = {"div_probe_key", "div_build_key", "div_group_key", "div_sort_key_0", "div_sort_key_1", "div_sort_key_2", "div_sort_key_3", "minmax_null_groups",
            "bitmap_without_nulls_arith", "bitmap_without_nulls_sort", "bitmap_without_nulls_group", "bitmap_without_nulls_join_probe",
            "bitmap_without_nulls_join_build", "first_row_as_index_then_group_by_it", "sort_indices_chain_and_selection_indices", "join_string_payload_sliced",
            "empty_then_group_and_join", "empty_build_side", "null_columns_ride_along", "csv_reference_batch_into_group_and_sort"}
    assert want <= names and os.path.getsize(GOLDEN) < 16 * 1024


def test_directed_pipelines_run_through_the_model_at_toy_size():
    for name in pc.DIRECTED:
        if name.startswith("bitmap_without_nulls_"):
            pc.assert_consumer_met_bitmap_without_nulls(pc.directed_case(name, 12))
        inter, _ = pm.run_case(pc.directed_case(name, 12))
        assert len(inter) == len(pc.directed(name, 12)[1]) + 1
        if name.startswith("empty_"):
            assert pm.rows(inter[-1][0]) == 0


def test_generated_predicates_keep_the_oracles_rows(runs, oracle):
    """helpers.host_survivors against the C++ oracle, used as tests/test_fuzz_gpu.py uses it, for every filter and mask step emitted."""
    checked = 0
    for case, inter, builds in runs:
        pipelines = [(case["steps"], inter)] + [(case["builds"][k]["steps"], builds[k]) for k in builds]
        for steps, frames in pipelines:
            for k, step in enumerate(steps):
                frame = frames[k][0]
                if step["kind"] not in ("filter", "mask") or pm.rows(frame) == 0:
                    continue
                sel, count = oracle.eval_predicate(pm.predicate_columns(frame), pm.predicate_of(step))
                keep = pm.survivors(frame, step)
                assert count == int(keep.sum()) and np.array_equal(sel.logical_values().astype(bool), keep), f"seed {case['seed']} step {k}: {step}"
                checked += 1
    assert checked >= 100
