"""CPU suite: the join reference model (tests/join_model.py) against hand-worked cases of the reference's
PhysicalPlan::HashJoin (plan.rs:174-284), and the join's additions to the C ABI.  No GPU."""
import os

from join_model import NULL_KEY, any_key, comparable, inner_join_pairs, materialize
from rivulus_amd import capi
from rivulus_amd.capi import RV_BOOLEAN, RV_FLOAT64, RV_INT64, RV_NULL, RV_STRING

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def test_duplicates_on_both_sides_run_in_probe_order_then_build_order():
    build = [7, 3, 7, 9, 7]
    probe = [7, 1, 3, 7]
    assert inner_join_pairs(RV_INT64, build, RV_INT64, probe) == [(0, 0), (0, 2), (0, 4), (2, 1), (3, 0), (3, 2), (3, 4)]


def test_null_meets_every_null_and_nothing_else():
    build = [None, 1, None, 0]
    probe = [0, None, None]
    assert inner_join_pairs(RV_INT64, build, RV_INT64, probe) == [(0, 3), (1, 0), (1, 2), (2, 0), (2, 2)]


def test_nan_never_matches_even_the_same_bits():
    build = [NAN, 1.5, NAN]
    probe = [NAN, 1.5]
    assert any_key(RV_FLOAT64, NAN) is None
    assert inner_join_pairs(RV_FLOAT64, build, RV_FLOAT64, probe) == [(1, 1)]


def test_signed_zeros_are_two_keys():
    build = [0.0, -0.0]
    probe = [-0.0, 0.0, 0.0]
    assert inner_join_pairs(RV_FLOAT64, build, RV_FLOAT64, probe) == [(0, 1), (1, 0), (2, 0)]


def test_int64_against_float64_meets_null_to_null_only():
    build = [1, None, 2]
    probe = [1.0, 2.0, None]
    assert inner_join_pairs(RV_INT64, build, RV_FLOAT64, probe) == [(2, 1)]


def test_boolean_keys_and_an_all_null_key_column():
    assert inner_join_pairs(RV_BOOLEAN, [True, False, True], RV_BOOLEAN, [False, True]) == [(0, 1), (1, 0), (1, 2)]
    assert any_key(RV_NULL, 5) == NULL_KEY
    assert inner_join_pairs(RV_NULL, [None, None], RV_INT64, [None, 3]) == [(0, 0), (0, 1)]


def test_empty_result_keeps_the_columns_and_their_dtypes():
    probe = [("id", RV_INT64, [1, 2]), ("v", RV_FLOAT64, [0.5, 1.5])]
    build = [("id", RV_INT64, [3]), ("name", RV_STRING, ["x"])]
    pairs = inner_join_pairs(RV_INT64, [3], RV_INT64, [1, 2])
    assert pairs == []
    out = materialize(probe, build, "id", pairs)
    assert [(n, d, c) for n, d, c in out] == [("id", RV_INT64, []), ("v", RV_FLOAT64, []), ("name", RV_STRING, [])]


def test_users_orders_demo():
    """The reference demo's join (main.rs, queries 6 and 7): users (left, build) joined with orders (right, probe) on
    user_id.  The golden fixture was worked out by hand from plan.rs:174-284."""
    import json
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "join_users_orders.json")))
    users = [(c["name"], getattr(capi, c["dtype"]), c["cells"]) for c in g["users"]]
    orders = [(c["name"], getattr(capi, c["dtype"]), c["cells"]) for c in g["orders"]]
    bk = [c for n, _, c in users if n == "user_id"][0]
    pk = [c for n, _, c in orders if n == "user_id"][0]
    pairs = inner_join_pairs(RV_INT64, bk, RV_INT64, pk)
    assert [list(p) for p in pairs] == g["pairs"]
    out = materialize(orders, users, "user_id", pairs)
    assert [n for n, _, _ in out] == g["columns"]
    for (n, d, cells), want in zip(out, g["result"]):
        assert comparable(d, cells) == comparable(d, want), n


def test_c_abi_declares_the_join():
    text = open(os.path.join(ROOT, "include", "rivulus_gpu.h")).read()
    assert "inner hash join (PhysicalPlan::HashJoin)" in text
    for sym in ("rv_join_build", "rv_join_probe", "rv_join_table_free", "rv_join_table_info", "rv_hash_join"):
        assert sym in capi.PROTOTYPES
    assert "rv_join_table" in open(os.path.join(ROOT, "tools", "gen_rust_ffi.py")).read()
    assert "pub struct RvJoinTable" in open(os.path.join(ROOT, "rust_shim", "ffi.rs")).read()
