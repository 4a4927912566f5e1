// group_by(key).agg([...]) in the host layer (rivulus_amd/host/rivulus_host.hpp): group_by_schema, PhysicalPlan::group_by (eager, one
// rv_hash_aggregate) and StreamingPhysicalPlan::group_by (a pipeline breaker that emits exactly one batch), over Int64 and String keys.
// Run by tests/test_group_agg_host.py; the scaffold is host_test_main.hpp.
#include <map>
#include <optional>

#include "host_test_main.hpp"
#include "join_test_cells.hpp"

using namespace rivulus;
using namespace rivulus::execution;
using namespace rivulus::expressions;
using namespace rivulus::physical_plan;

namespace {

const std::vector<AggSpec> kAggs = {{AggOp::CountRows, "", "rows"}, {AggOp::Count, "v", "n_v"}, {AggOp::Sum, "v", "sum_v"}, {AggOp::Min, "v", "min_v"},
                                    {AggOp::Max, "v", "max_v"},    {AggOp::Sum, "f", "sum_f"}, {AggOp::Max, "f", "max_f"}, {AggOp::Count, "s", "n_s"}};
const std::vector<std::string> kOutNames = {"k", "rows", "n_v", "sum_v", "min_v", "max_v", "sum_f", "max_f", "n_s"};

// the rows of the test frame on the host: k an Int64 key or (string_key) a String key over `groups` values, v Int64, f Float64 in
// quarters (every sum exact in any order), s String; nulls in k, v and s where `nulls`
struct Rows {
    std::vector<std::optional<std::string>> k;  // the key as text: "7" / "key-7"
    std::vector<std::optional<int64_t>> v;
    std::vector<double> f;
    std::vector<std::optional<std::string>> s;
};
Rows make_rows(size_t n, size_t groups, bool nulls, bool string_key) {
    Rows r;
    for (size_t i = 0; i < n; ++i) {
        const size_t g = (i * 7919 + i / 3) % groups;
        if (nulls && i % 11 == 4) r.k.push_back(std::nullopt);
        else r.k.push_back(string_key ? (g == 2 ? std::string() : "key-" + std::to_string(g)) : std::to_string(static_cast<int64_t>(g) * 1000003 - 5));
        r.v.push_back(nulls && i % 5 == 3 ? std::nullopt : std::optional<int64_t>(static_cast<int64_t>((i * 104729) % 2001) - 1000));
        r.f.push_back(static_cast<double>((i * 31) % 801) * 0.25 - 100.0);
        r.s.push_back(nulls && i % 4 == 1 ? std::nullopt : std::optional<std::string>(i % 8 ? "s" + std::to_string(i % 13) : ""));
    }
    return r;
}
DeviceFrame frame_of(const Rows &r, bool string_key) {
    const size_t n = r.k.size();
    DeviceFrame df;
    df.names = {"k", "v", "f", "s"};
    std::vector<int64_t> kv(n), vv(n);
    std::vector<bool> kvalid(n), vvalid(n);
    bool knull = false, vnull = false;
    for (size_t i = 0; i < n; ++i) {
        kvalid[i] = r.k[i].has_value();
        kv[i] = kvalid[i] && !string_key ? std::stoll(*r.k[i]) : 0;
        vvalid[i] = r.v[i].has_value();
        vv[i] = r.v[i].value_or(0);
        knull |= !kvalid[i];
        vnull |= !vvalid[i];
    }
    ArrayRef key = string_key ? ArrayRef(StringArray::create(ctx(), r.k)) : ArrayRef(Int64Array::create(ctx(), kv, knull ? std::optional<std::vector<bool>>(kvalid) : std::nullopt));
    df.columns = {key, Int64Array::create(ctx(), vv, vnull ? std::optional<std::vector<bool>>(vvalid) : std::nullopt), Float64Array::from_values(ctx(), r.f),
                  StringArray::create(ctx(), r.s)};
    return df;
}
// kAggs over `r`, as text, the groups in the order of their first rows; `keep`: the rows a filter left
Table expected(const Rows &r, bool string_key, const std::function<bool(size_t)> &keep = [](size_t) { return true; }) {
    struct G {
        std::string key;
        int64_t rows = 0, n_v = 0, sum_v = 0, n_s = 0;
        std::optional<int64_t> min_v, max_v;
        double sum_f = 0.0, max_f = -1e300;
    };
    std::vector<G> groups;
    std::map<std::string, size_t> at;
    for (size_t i = 0; i < r.k.size(); ++i) {
        if (!keep(i)) continue;
        const std::string key = r.k[i] ? (string_key ? "'" + *r.k[i] + "'" : *r.k[i]) : "null";
        auto it = at.find(key);
        if (it == at.end()) {
            it = at.emplace(key, groups.size()).first;
            groups.emplace_back();
            groups.back().key = key;
        }
        G &g = groups[it->second];
        ++g.rows;
        if (r.v[i]) {
            ++g.n_v;
            g.sum_v += *r.v[i];
            g.min_v = g.min_v ? std::min(*g.min_v, *r.v[i]) : *r.v[i];
            g.max_v = g.max_v ? std::max(*g.max_v, *r.v[i]) : *r.v[i];
        }
        g.sum_f += r.f[i];
        g.max_f = std::max(g.max_f, r.f[i]);
        g.n_s += r.s[i].has_value();
    }
    Table t(kOutNames.size());
    for (auto &g : groups) {
        t[0].push_back(g.key);
        t[1].push_back(std::to_string(g.rows));
        t[2].push_back(std::to_string(g.n_v));
        t[3].push_back(std::to_string(g.sum_v));
        t[4].push_back(g.min_v ? std::to_string(*g.min_v) : "null");
        t[5].push_back(g.max_v ? std::to_string(*g.max_v) : "null");
        t[6].push_back(f17(g.sum_f + 0.0));
        t[7].push_back(f17(g.max_f));
        t[8].push_back(std::to_string(g.n_s));
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
Schema kvfs_schema(DataType key) {
    return Schema({Field{"k", key, true}, Field{"v", DataType::Int64, true}, Field{"f", DataType::Float64, true}, Field{"s", DataType::String, true},
                   Field{"b", DataType::Boolean, true}});
}

}  // namespace

// ---- planning (no device) -----------------------------------------------------------------------------------------------------------
CPU_TEST(output_schema_is_the_key_then_every_aggregate_under_its_name) {
    for (DataType key : {DataType::Int64, DataType::String}) {
        SchemaRef s = group_by_schema(kvfs_schema(key), "k", kAggs);
        CHECK(s->num_fields() == kOutNames.size());
        for (size_t i = 0; i < kOutNames.size(); ++i) CHECK(s->field(i).name() == kOutNames[i]);
        CHECK(s->field(0).data_type() == key);
        const DataType want[] = {DataType::Int64, DataType::Int64, DataType::Int64, DataType::Int64, DataType::Int64, DataType::Float64, DataType::Float64, DataType::Int64};
        for (size_t i = 0; i < 8; ++i) CHECK(s->field(1 + i).data_type() == want[i]);
    }
    // COUNT takes any column; the key may be aggregated too
    SchemaRef s = group_by_schema(kvfs_schema(DataType::Int64), "k", {{AggOp::Count, "b", "n_b"}, {AggOp::Count, "s", "n_s"}, {AggOp::Max, "k", "top"}});
    CHECK(s->num_fields() == 4 && s->field(3).data_type() == DataType::Int64);
}

CPU_TEST(planning_errors_say_which_column) {
    const Schema s = kvfs_schema(DataType::Int64);
    auto why = [&](const std::string &key, std::vector<AggSpec> aggs) { return thrown<GroupByPlanError>([&] { group_by_schema(s, key, aggs); }); };
    CHECK(why("zz", kAggs) == "group_by: unknown key column 'zz'");
    CHECK(why("k", {{AggOp::Sum, "nope", "x"}}) == "group_by: aggregate 'x' reads the unknown column 'nope'");
    CHECK(why("k", {{AggOp::Sum, "v", "x"}, {AggOp::Min, "v", "x"}}) == "group_by: duplicate output name 'x'");
    CHECK(why("k", {{AggOp::Sum, "v", "k"}}) == "group_by: duplicate output name 'k'");  // the key's own name is taken
    CHECK(why("k", {{AggOp::Sum, "s", "x"}}) == "group_by: SUM over column 's' of dtype String");
    CHECK(why("k", {{AggOp::Min, "b", "x"}}) == "group_by: MIN over column 'b' of dtype Boolean");
    CHECK(why("k", {{AggOp::Max, "s", "x"}}) == "group_by: MAX over column 's' of dtype String");
    CHECK(why("f", kAggs) == "group_by: key column 'f' is Float64; only Int64 and String keys are grouped");
    CHECK(why("b", kAggs) == "group_by: key column 'b' is Boolean; only Int64 and String keys are grouped");
    CHECK(why("k", {}) == "group_by: no aggregates");
    CHECK(why("k", {{AggOp::CountRows, "nope", "rows"}}).empty());  // COUNT(*) reads no column
}

// ---- on the device ------------------------------------------------------------------------------------------------------------------
GPU_TEST(eager_group_by_over_int64_and_string_keys) {
    for (bool string_key : {false, true})
        for (bool nulls : {false, true}) {
            const Rows r = make_rows(3000, 37, nulls, string_key);
            DeviceFrame got = PhysicalPlan::group_by(PhysicalPlan::source(frame_of(r, string_key)), "k", kAggs)->execute();
            CHECK(got.names == kOutNames);
            CHECK(got.columns[0]->data_type() == (string_key ? DataType::String : DataType::Int64));
            const Table want = expected(r, string_key);
            CHECK(got.height() == want[0].size() && got.height() == (nulls ? 38u : 37u));
            CHECK(cells(got.columns, 0, got.height()) == want);
            CHECK(!got.columns[1]->has_null_bitmap() && !got.columns[3]->has_null_bitmap());  // counts and sums carry no bitmap
        }
}

GPU_TEST(null_strings_are_one_group_and_the_empty_string_is_a_value) {
    DeviceFrame df;
    df.names = {"k", "v"};
    df.columns = {StringArray::create(ctx(), {"", std::nullopt, "a", "", std::nullopt, "a", "b"}), Int64Array::from_values(ctx(), {1, 2, 4, 8, 16, 32, 64})};
    DeviceFrame got = PhysicalPlan::group_by(PhysicalPlan::source(df), "k", {{AggOp::Sum, "v", "total"}, {AggOp::CountRows, "", "rows"}})->execute();
    CHECK((cells(got.columns, 0, got.height()) == Table{{"''", "null", "'a'", "'b'"}, {"9", "18", "36", "64"}, {"2", "2", "2", "1"}}));
}

GPU_TEST(planning_errors_reach_execute_and_the_context_stays_usable) {
    const Rows r = make_rows(50, 5, true, false);
    DeviceFrame df = frame_of(r, false);
    CHECK(thrown<GroupByPlanError>([&] { PhysicalPlan::group_by(PhysicalPlan::source(df), "zz", kAggs)->execute(); }) == "group_by: unknown key column 'zz'");
    CHECK(thrown<GroupByPlanError>([&] { PhysicalPlan::group_by(PhysicalPlan::source(df), "k", {{AggOp::Sum, "s", "x"}})->execute(); }) ==
          "group_by: SUM over column 's' of dtype String");
    auto plan = StreamingPhysicalPlan::group_by(StreamingPhysicalPlan::memory_source(batches_of(df, 16)), "k", {{AggOp::Sum, "v", "x"}, {AggOp::Max, "f", "x"}});
    CHECK(thrown<GroupByPlanError>([&] { plan->execute(); }) == "group_by: duplicate output name 'x'");
    DeviceFrame got = PhysicalPlan::group_by(PhysicalPlan::source(df), "k", kAggs)->execute();
    CHECK(cells(got.columns, 0, got.height()) == expected(r, false));
}

GPU_TEST(a_stream_emits_exactly_one_batch) {
    for (bool string_key : {false, true}) {
        const Rows r = make_rows(2500, 23, true, string_key);
        DeviceFrame df = frame_of(r, string_key);
        const Table want = expected(r, string_key);
        // batches that keep their nulls (a MemoryStream): the eager result, in one batch
        for (size_t batch : {size_t{1024}, size_t{2500}}) {
            auto stream = StreamingPhysicalPlan::group_by(StreamingPhysicalPlan::memory_source(batches_of(df, batch)), "k", kAggs)->execute();
            CHECK(stream->schema()->num_fields() == kOutNames.size() && stream->schema()->field(6).name() == "sum_f");
            auto got = stream->collect();
            CHECK(got.size() == 1 && *got[0].schema() == *stream->schema());
            CHECK(got[0].num_rows() == want[0].size() && cells(got[0].columns(), 0, got[0].num_rows()) == want);
            CHECK(!stream->next_batch());
        }
    }
    // a resident frame is taken whole after the null fill of dataframe_to_batches: Int64 nulls are 0 there, String nulls stay
    Rows r = make_rows(2500, 23, true, true);
    DeviceFrame df = frame_of(r, true);
    auto got = StreamingPhysicalPlan::group_by(StreamingPhysicalPlan::dataframe_source(df, 1024), "k", kAggs)->collect_batches();
    for (auto &v : r.v) v = v.value_or(0);
    CHECK(got.size() == 1 && cells(got[0].columns(), 0, got[0].num_rows()) == expected(r, true));
}

GPU_TEST(an_empty_input_gives_one_zero_row_batch_with_the_schema) {
    const Rows none = make_rows(0, 1, false, false);
    for (bool string_key : {false, true}) {
        // a resident frame without rows
        auto got = StreamingPhysicalPlan::group_by(StreamingPhysicalPlan::dataframe_source(frame_of(none, string_key), 1024), "k", kAggs)->collect_batches();
        CHECK(got.size() == 1 && got[0].num_rows() == 0 && got[0].num_columns() == kOutNames.size());
        CHECK(got[0].schema()->field(0).data_type() == (string_key ? DataType::String : DataType::Int64));
        CHECK(got[0].column(6)->data_type() == DataType::Float64 && got[0].column(4)->data_type() == DataType::Int64 && got[0].column(4)->len() == 0);
        // the eager plan over it
        DeviceFrame eager = PhysicalPlan::group_by(PhysicalPlan::source(frame_of(none, string_key)), "k", kAggs)->execute();
        CHECK(eager.height() == 0 && eager.names == kOutNames && eager.columns[7]->data_type() == DataType::Float64);
    }
    // a filter that keeps nothing: whatever batches it yields, the group_by yields one without rows
    const Rows r = make_rows(2000, 9, false, false);
    auto filtered = StreamingPhysicalPlan::gpu_filter_project(StreamingPhysicalPlan::memory_source(batches_of(frame_of(r, false), 512)),
                                                              lower_predicate(Expr::col("v").gt(Expr::lit(5000))), {"k", "v", "f", "s"});
    auto got = StreamingPhysicalPlan::group_by(filtered, "k", kAggs)->collect_batches();
    CHECK(got.size() == 1 && got[0].num_rows() == 0 && got[0].num_columns() == kOutNames.size() && got[0].column(0)->data_type() == DataType::Int64);
}

GPU_TEST(filter_then_group_by) {
    const Rows r = make_rows(4000, 41, false, false);
    DeviceFrame df = frame_of(r, false);
    const Table want = expected(r, false, [&](size_t i) { return *r.v[i] > 250; });
    CHECK(want[0].size() == 41);
    DeviceFrame eager = PhysicalPlan::group_by(PhysicalPlan::filter(PhysicalPlan::source(df), CompareTerm{"v", RV_GT, Literal(int64_t{250})}), "k", kAggs)->execute();
    CHECK(cells(eager.columns, 0, eager.height()) == want);
    auto filtered = StreamingPhysicalPlan::gpu_filter_project(StreamingPhysicalPlan::dataframe_source(df, 1024), lower_predicate(Expr::col("v").gt(Expr::lit(250))),
                                                              {"k", "v", "f", "s"});
    auto got = StreamingPhysicalPlan::group_by(filtered, "k", kAggs)->collect_batches();
    CHECK(got.size() == 1 && cells(got[0].columns(), 0, got[0].num_rows()) == want);
}

// the reference demo's users / orders (tests/golden/join_users_orders.json): orders joined to users, then "per customer"
GPU_TEST(hash_join_then_group_by_on_users_and_orders) {
    DeviceFrame users, orders;
    users.names = {"user_id", "name", "city"};
    users.columns = {Int64Array::from_values(ctx(), {1, 2, 3, 4}), StringArray::from_strings(ctx(), {"Alice", "Bob", "Charlie", "Diana"}),
                     StringArray::from_strings(ctx(), {"NYC", "LA", "Chicago", "Boston"})};
    orders.names = {"order_id", "user_id", "amount"};
    orders.columns = {Int64Array::from_values(ctx(), {101, 102, 103, 104, 105}), Int64Array::from_values(ctx(), {1, 2, 1, 3, 99}),
                      Float64Array::from_values(ctx(), {25.99, 15.50, 99.99, 45.00, 12.99})};
    const std::vector<AggSpec> aggs = {{AggOp::Sum, "amount", "spent"}, {AggOp::CountRows, "", "orders"}, {AggOp::Max, "order_id", "last_order"}};
    const Table by_name = {{"'Alice'", "'Bob'", "'Charlie'"}, {f17(25.99 + 99.99), f17(15.50), f17(45.00)}, {"2", "1", "1"}, {"103", "102", "104"}};
    auto joined = PhysicalPlan::hash_join(PhysicalPlan::source(users), PhysicalPlan::source(orders), "user_id", "user_id");
    DeviceFrame got = PhysicalPlan::group_by(joined, "name", aggs)->execute();
    CHECK((got.names == std::vector<std::string>{"name", "spent", "orders", "last_order"}));
    CHECK(cells(got.columns, 0, got.height()) == by_name);
    // by the Int64 key, and as a stream
    DeviceFrame by_id = PhysicalPlan::group_by(joined, "user_id", aggs)->execute();
    CHECK((cells(by_id.columns, 0, by_id.height()) == Table{{"1", "2", "3"}, by_name[1], by_name[2], by_name[3]}));
    auto sjoined = StreamingPhysicalPlan::hash_join(StreamingPhysicalPlan::dataframe_source(users, 1024), StreamingPhysicalPlan::dataframe_source(orders, 2), "user_id", "user_id");
    auto batches = StreamingPhysicalPlan::group_by(sjoined, "name", aggs)->collect_batches();
    CHECK(batches.size() == 1 && cells(batches[0].columns(), 0, batches[0].num_rows()) == by_name);
}
