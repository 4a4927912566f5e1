// group_by([k0, k1, ...]).agg([...]) in the host layer (rivulus_amd/host/rivulus_host.hpp): the key-list forms of group_by_schema,
// PhysicalPlan::group_by (eager, one rv_hash_aggregate_keys) and StreamingPhysicalPlan::group_by (a pipeline breaker that emits exactly one
// batch), over Int64, Float64, Boolean, String and Null keys.  Run by tests/test_group_keys_host.py; the scaffold is host_test_main.hpp.
#include <cmath>
#include <map>
#include <optional>
#include <tuple>

#include "host_test_main.hpp"
#include "join_test_cells.hpp"

using namespace rivulus;
using namespace rivulus::execution;
using namespace rivulus::expressions;
using namespace rivulus::physical_plan;

namespace {

using Keys = std::vector<std::string>;
const std::vector<AggSpec> kAggs = {{AggOp::Sum, "v", "total"}, {AggOp::CountRows, "", "rows"}};

Schema wide_schema() {
    return Schema({Field{"i", DataType::Int64, false}, Field{"f", DataType::Float64, true}, Field{"b", DataType::Boolean, true}, Field{"s", DataType::String, true},
                   Field{"z", DataType::Null, true}, Field{"v", DataType::Int64, true}});
}

// the frame of the plan tests: a Int64 over `na` values with nulls, b Boolean with nulls, v Int64
struct Rows {
    std::vector<std::optional<int64_t>> a;
    std::vector<std::optional<bool>> b;
    std::vector<int64_t> v;
};
Rows make_rows(size_t n, size_t na) {
    Rows r;
    for (size_t i = 0; i < n; ++i) {
        r.a.push_back(i % 13 == 5 ? std::nullopt : std::optional<int64_t>(static_cast<int64_t>((i * 7919 + i / 3) % na) * 1000003 - 5));
        r.b.push_back(i % 7 == 2 ? std::nullopt : std::optional<bool>((i * 31 + i / 5) % 2 == 0));
        r.v.push_back(static_cast<int64_t>((i * 104729) % 2001) - 1000);
    }
    return r;
}
DeviceFrame frame_of(const Rows &r) {
    const size_t n = r.v.size();
    std::vector<int64_t> av(n);
    std::vector<bool> avalid(n);
    for (size_t i = 0; i < n; ++i) {
        avalid[i] = r.a[i].has_value();
        av[i] = r.a[i].value_or(777);  // something lies under a null
    }
    DeviceFrame df;
    df.names = {"a", "b", "v"};
    df.columns = {Int64Array::create(ctx(), av, std::optional<std::vector<bool>>(avalid)), BooleanArray::create(ctx(), r.b), Int64Array::from_values(ctx(), r.v)};
    return df;
}
std::string text(const std::optional<int64_t> &x) { return x ? std::to_string(*x) : "null"; }
std::string text(const std::optional<bool> &x) { return x ? (*x ? "true" : "false") : "null"; }
// group_by({a, b}).agg(kAggs) over the rows `keep` leaves, as text; sorted: by (a, b) ascending (no nulls among the rows kept), else
// the groups in the order of their first rows
Table expected(const Rows &r, bool sorted, const std::function<bool(size_t)> &keep = [](size_t) { return true; }) {
    struct G {
        std::string a, b;
        int64_t total = 0, rows = 0;
    };
    std::vector<G> groups;
    std::map<std::pair<std::string, std::string>, size_t> at;
    std::map<std::pair<int64_t, bool>, size_t> order;
    for (size_t i = 0; i < r.v.size(); ++i) {
        if (!keep(i)) continue;
        const auto key = std::make_pair(text(r.a[i]), text(r.b[i]));
        auto it = at.find(key);
        if (it == at.end()) {
            it = at.emplace(key, groups.size()).first;
            groups.push_back(G{key.first, key.second});
            if (sorted) order.emplace(std::make_pair(*r.a[i], *r.b[i]), it->second);
        }
        groups[it->second].total += r.v[i];
        ++groups[it->second].rows;
    }
    std::vector<size_t> seq;
    if (sorted)
        for (auto &o : order) seq.push_back(o.second);
    else
        for (size_t g = 0; g < groups.size(); ++g) seq.push_back(g);
    Table t(4);
    for (size_t g : seq) {
        t[0].push_back(groups[g].a);
        t[1].push_back(groups[g].b);
        t[2].push_back(std::to_string(groups[g].total));
        t[3].push_back(std::to_string(groups[g].rows));
    }
    return t;
}
std::vector<RecordBatch> batches_of(const DeviceFrame &df, size_t batch) {  // zero-copy slices: the nulls stay
    auto schema = std::make_shared<Schema>(frame_schema(df));
    std::vector<RecordBatch> out;
    for (size_t lo = 0; lo < df.height(); lo += batch) {
        std::vector<ArrayRef> cols;
        for (auto &c : df.columns) cols.push_back(c->slice(lo, std::min(batch, df.height() - lo)));
        out.push_back(RecordBatch::try_new(schema, std::move(cols)));
    }
    return out;
}

}  // namespace

// ---- planning (no device) -----------------------------------------------------------------------------------------------------------
CPU_TEST(output_schema_is_the_keys_in_the_order_given_then_the_aggregates) {
    const Keys keys = {"s", "f", "z", "b", "i"};
    SchemaRef s = group_by_schema(wide_schema(), keys, kAggs);
    CHECK(s->num_fields() == 7);
    const DataType want[] = {DataType::String, DataType::Float64, DataType::Null, DataType::Boolean, DataType::Int64};
    for (size_t k = 0; k < keys.size(); ++k) {
        CHECK(s->field(k).name() == keys[k] && s->field(k).data_type() == want[k]);
        CHECK(s->field(k).is_nullable());  // "i" is not nullable in the input: a key of the output is
    }
    CHECK(s->field(5).name() == "total" && s->field(5).data_type() == DataType::Int64 && s->field(6).name() == "rows");
    // one name: how a Float64 or a Boolean key is grouped; a key may be aggregated too
    for (const char *one : {"f", "b", "i", "s", "z"}) {
        SchemaRef t = group_by_schema(wide_schema(), Keys{one}, {{AggOp::Max, "i", "top"}, {AggOp::Count, "s", "n_s"}});
        CHECK(t->num_fields() == 3 && t->field(0).name() == one && t->field(0).data_type() == wide_schema().field_by_name(one)->data_type());
    }
    CHECK(group_by_schema(wide_schema(), Keys{"i", "f", "b", "s", "z", "v"}, {{AggOp::CountRows, "", "rows"}})->num_fields() == 7);
}

CPU_TEST(planning_errors_of_the_key_list) {
    const Schema s = wide_schema();
    auto why = [&](const Keys &keys, std::vector<AggSpec> aggs) { return thrown<GroupByPlanError>([&] { group_by_schema(s, keys, aggs); }); };
    CHECK(why({}, kAggs) == "group_by: no key columns");
    CHECK(why({"i", "zz"}, kAggs) == "group_by: unknown key column 'zz'");
    CHECK(why({"i", "f", "i"}, kAggs) == "group_by: key column 'i' is named twice");
    CHECK(why({"i", "f", "b", "s", "z", "v", "i", "f", "b"}, kAggs) == "group_by: 9 key columns; at most 8 are grouped");
    CHECK(why({"i", "f"}, {{AggOp::Sum, "v", "f"}}) == "group_by: duplicate output name 'f'");  // an aggregate named like a key
    CHECK(why({"i", "f"}, {{AggOp::Sum, "v", "x"}, {AggOp::Min, "v", "x"}}) == "group_by: duplicate output name 'x'");
    CHECK(why({"i"}, {}) == "group_by: no aggregates");
    CHECK(why({"i"}, {{AggOp::Sum, "nope", "x"}}) == "group_by: aggregate 'x' reads the unknown column 'nope'");
    CHECK(why({"i"}, {{AggOp::Sum, "s", "x"}}) == "group_by: SUM over column 's' of dtype String");
    CHECK(why({"f", "b"}, {{AggOp::Min, "b", "x"}}) == "group_by: MIN over column 'b' of dtype Boolean");
    CHECK(why({"f", "b"}, kAggs).empty());
    // the single-key form keeps its refusals, word for word
    auto one = [&](const std::string &key) { return thrown<GroupByPlanError>([&] { group_by_schema(s, key, kAggs); }); };
    CHECK(one("f") == "group_by: key column 'f' is Float64; only Int64 and String keys are grouped");
    CHECK(one("b") == "group_by: key column 'b' is Boolean; only Int64 and String keys are grouped");
    CHECK(one("i").empty());
}

// ---- on the device ------------------------------------------------------------------------------------------------------------------
GPU_TEST(eager_group_by_a_string_and_an_int64_key) {
    DeviceFrame df;
    df.names = {"s", "i", "v"};
    df.columns = {StringArray::create(ctx(), {"", std::nullopt, "a", "", std::nullopt, "a", "", std::nullopt}),
                  Int64Array::create(ctx(), {1, 1, 1, 1, 2, 1, 5, 1}, std::vector<bool>{true, true, true, true, true, true, false, true}),
                  Int64Array::from_values(ctx(), {1, 2, 4, 8, 16, 32, 64, 128})};
    DeviceFrame got = PhysicalPlan::group_by(PhysicalPlan::source(df), Keys{"s", "i"}, kAggs)->execute();
    CHECK((got.names == Keys{"s", "i", "total", "rows"}));
    CHECK(got.columns[0]->data_type() == DataType::String && got.columns[1]->data_type() == DataType::Int64);
    // null strings and "" are different keys; (null, 1) and (null, 2) are; ("", 1) and ("", null) are
    CHECK((cells(got.columns, 0, got.height()) ==
           Table{{"''", "null", "'a'", "null", "''"}, {"1", "1", "1", "2", "null"}, {"9", "130", "36", "16", "64"}, {"2", "2", "2", "1", "1"}}));
    // the keys the other way round: the same groups, the columns swapped
    DeviceFrame swapped = PhysicalPlan::group_by(PhysicalPlan::source(df), Keys{"i", "s"}, kAggs)->execute();
    CHECK((swapped.names == Keys{"i", "s", "total", "rows"}));
    CHECK(cell(swapped.columns[1], 4) == "''" && cell(swapped.columns[0], 4) == "null" && cell(swapped.columns[2], 1) == "130");
    // two String keys, each through a dictionary of its own
    df.names = {"s", "t", "v"};
    df.columns[1] = StringArray::create(ctx(), {"x", "x", "", "x", "x", std::nullopt, "y", "x"});
    DeviceFrame two = PhysicalPlan::group_by(PhysicalPlan::source(df), Keys{"s", "t"}, kAggs)->execute();
    CHECK((cells(two.columns, 0, two.height()) ==
           Table{{"''", "null", "'a'", "'a'", "''"}, {"'x'", "'x'", "''", "null", "'y'"}, {"9", "146", "4", "32", "64"}, {"2", "3", "1", "1", "1"}}));
}

GPU_TEST(float64_and_boolean_single_keys_through_the_key_list) {
    uint64_t neg_nan_bits = 0xFFF800000000BEEFull;
    double neg_nan;
    std::memcpy(&neg_nan, &neg_nan_bits, 8);
    DeviceFrame df;
    df.names = {"f", "b", "v"};
    df.columns = {Float64Array::create(ctx(), {std::nan(""), 0.0, -0.0, neg_nan, 1.5, 99.0, 0.0}, std::vector<bool>{true, true, true, true, true, false, true}),
                  BooleanArray::create(ctx(), {true, false, std::nullopt, true, false, std::nullopt, false}), Int64Array::from_values(ctx(), {1, 2, 4, 8, 16, 32, 64})};
    DeviceFrame by_f = PhysicalPlan::group_by(PhysicalPlan::source(df), Keys{"f"}, kAggs)->execute();
    CHECK((by_f.names == Keys{"f", "total", "rows"}) && by_f.columns[0]->data_type() == DataType::Float64);
    // every NaN one group, -0.0 and +0.0 two, the null one of its own
    CHECK((cells(by_f.columns, 0, by_f.height()) == Table{{f17(std::nan("")), f17(0.0), f17(-0.0), f17(1.5), "null"}, {"9", "66", "4", "16", "32"}, {"2", "2", "1", "1", "1"}}));
    DeviceFrame by_b = PhysicalPlan::group_by(PhysicalPlan::source(df), Keys{"b"}, kAggs)->execute();
    CHECK(by_b.columns[0]->data_type() == DataType::Boolean);
    CHECK((cells(by_b.columns, 0, by_b.height()) == Table{{"true", "false", "null"}, {"9", "82", "36"}, {"2", "3", "2"}}));
    // the single-key form still refuses both, and the context stays usable
    CHECK(thrown<GroupByPlanError>([&] { PhysicalPlan::group_by(PhysicalPlan::source(df), "f", kAggs)->execute(); }) ==
          "group_by: key column 'f' is Float64; only Int64 and String keys are grouped");
    CHECK(thrown<GroupByPlanError>([&] { PhysicalPlan::group_by(PhysicalPlan::source(df), Keys{"f", "f"}, kAggs)->execute(); }) == "group_by: key column 'f' is named twice");
    CHECK(thrown<GroupByPlanError>([&] { PhysicalPlan::group_by(PhysicalPlan::source(df), Keys{}, kAggs)->execute(); }) == "group_by: no key columns");
    DeviceFrame both = PhysicalPlan::group_by(PhysicalPlan::source(df), Keys{"b", "f"}, kAggs)->execute();
    CHECK(both.height() == 5 && cell(both.columns[2], 0) == "9" && cell(both.columns[2], 1) == "66");  // (true, NaN) and (false, 0.0) twice each
}

GPU_TEST(a_null_typed_key_beside_an_int64_key) {
    DeviceFrame df;
    df.names = {"z", "i", "v"};
    df.columns = {NullArray::create(ctx(), 5), Int64Array::from_values(ctx(), {4, 3, 4, 3, 4}), Int64Array::from_values(ctx(), {1, 10, 100, 1000, 10000})};
    DeviceFrame got = PhysicalPlan::group_by(PhysicalPlan::source(df), Keys{"z", "i"}, kAggs)->execute();
    CHECK(got.columns[0]->data_type() == DataType::Null && got.columns[0]->len() == 2);
    CHECK((cells(got.columns, 0, got.height()) == Table{{"null", "null"}, {"4", "3"}, {"10101", "1010"}, {"3", "2"}}));
}

GPU_TEST(a_stream_over_a_multi_batch_source_emits_exactly_one_batch) {
    const Rows r = make_rows(2500, 9);
    DeviceFrame df = frame_of(r);
    const Table want = expected(r, false);
    CHECK(want[0].size() == 30);  // (9 values + null) x (true, false, null)
    DeviceFrame eager = PhysicalPlan::group_by(PhysicalPlan::source(df), Keys{"a", "b"}, kAggs)->execute();
    CHECK(cells(eager.columns, 0, eager.height()) == want);
    for (size_t batch : {size_t{1024}, size_t{2500}, size_t{333}}) {
        auto stream = StreamingPhysicalPlan::group_by(StreamingPhysicalPlan::memory_source(batches_of(df, batch)), Keys{"a", "b"}, kAggs)->execute();
        CHECK(stream->schema()->num_fields() == 4 && stream->schema()->field(1).name() == "b" && stream->schema()->field(1).data_type() == DataType::Boolean);
        auto got = stream->collect();
        CHECK(got.size() == 1 && *got[0].schema() == *stream->schema());
        CHECK(got[0].num_rows() == want[0].size() && cells(got[0].columns(), 0, got[0].num_rows()) == want);
        CHECK(!stream->next_batch());
    }
    // planning errors reach execute()
    auto bad = StreamingPhysicalPlan::group_by(StreamingPhysicalPlan::memory_source(batches_of(df, 1024)), Keys{"a", "nope"}, kAggs);
    CHECK(thrown<GroupByPlanError>([&] { bad->execute(); }) == "group_by: unknown key column 'nope'");
}

GPU_TEST(an_input_without_rows_gives_one_zero_row_batch_with_the_schema) {
    const Rows none = make_rows(0, 1);
    auto got = StreamingPhysicalPlan::group_by(StreamingPhysicalPlan::dataframe_source(frame_of(none), 1024), Keys{"b", "a"}, kAggs)->collect_batches();
    CHECK(got.size() == 1 && got[0].num_rows() == 0 && got[0].num_columns() == 4);
    CHECK(got[0].schema()->field(0).data_type() == DataType::Boolean && got[0].column(1)->data_type() == DataType::Int64 && got[0].column(2)->len() == 0);
    DeviceFrame eager = PhysicalPlan::group_by(PhysicalPlan::source(frame_of(none)), Keys{"b", "a"}, kAggs)->execute();
    CHECK(eager.height() == 0 && (eager.names == Keys{"b", "a", "total", "rows"}) && eager.columns[0]->data_type() == DataType::Boolean);
    // a filter that keeps nothing: whatever batches it yields, the group_by yields one without rows
    const Rows r = make_rows(2000, 9);
    auto filtered = StreamingPhysicalPlan::gpu_filter_project(StreamingPhysicalPlan::memory_source(batches_of(frame_of(r), 512)),
                                                              lower_predicate(Expr::col("v").gt(Expr::lit(5000))), {"a", "b", "v"});
    auto empty = StreamingPhysicalPlan::group_by(filtered, Keys{"a", "b"}, kAggs)->collect_batches();
    CHECK(empty.size() == 1 && empty[0].num_rows() == 0 && empty[0].num_columns() == 4 && empty[0].column(1)->data_type() == DataType::Boolean);
}

// every operator takes the columns the one before it made on the device
GPU_TEST(filter_then_group_by_two_keys_then_sort) {
    Rows r = make_rows(4000, 17);
    for (size_t i = 0; i < r.v.size(); ++i) {  // no nulls in the keys: the sort refuses none of them and the order is plain
        r.a[i] = r.a[i].value_or(-1);
        r.b[i] = r.b[i].value_or(true);
    }
    DeviceFrame df = frame_of(r);
    df.names = {"a", "b", "v", "c"};  // an Int64 image of b: the sort takes no Boolean key
    std::vector<int64_t> c;
    for (auto &b : r.b) c.push_back(*b ? 1 : 0);
    df.columns.push_back(Int64Array::from_values(ctx(), c));
    const auto keep = [&](size_t i) { return r.v[i] > 250; };
    const Table want = expected(r, true, keep);
    CHECK(want[0].size() == 36);
    auto filtered = PhysicalPlan::filter(PhysicalPlan::source(df), CompareTerm{"v", RV_GT, Literal(int64_t{250})});
    auto grouped = PhysicalPlan::group_by(filtered, Keys{"a", "c", "b"}, kAggs);
    DeviceFrame got = PhysicalPlan::sort(grouped, {SortKey{"a"}, SortKey{"c"}})->execute();
    CHECK((got.names == Keys{"a", "c", "b", "total", "rows"}));
    const Table all = cells(got.columns, 0, got.height());
    CHECK((Table{all[0], all[2], all[3], all[4]} == want));
    // the same through the streaming plan: filter -> group_by -> sort, one batch
    auto sfiltered = StreamingPhysicalPlan::gpu_filter_project(StreamingPhysicalPlan::dataframe_source(df, 1024), lower_predicate(Expr::col("v").gt(Expr::lit(250))),
                                                               {"a", "b", "v", "c"});
    auto batches = StreamingPhysicalPlan::sort(StreamingPhysicalPlan::group_by(sfiltered, Keys{"a", "c", "b"}, kAggs), {SortKey{"a"}, SortKey{"c"}})->collect_batches();
    CHECK(batches.size() == 1);
    const Table sall = cells(batches[0].columns(), 0, batches[0].num_rows());
    CHECK((Table{sall[0], sall[2], sall[3], sall[4]} == want));
}
