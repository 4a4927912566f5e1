// sort(keys) in the host layer (rivulus_amd/host/rivulus_host.hpp): sort_schema, PhysicalPlan::sort (eager, one rv_sort) and
// StreamingPhysicalPlan::sort (a pipeline breaker that emits exactly one batch), with String and Boolean columns riding along.
// Run by tests/test_sort_host.py; the scaffold is host_test_main.hpp.
#include <algorithm>
#include <map>
#include <numeric>
#include <optional>

#include "host_test_main.hpp"
#include "join_test_cells.hpp"

using namespace rivulus;
using namespace rivulus::execution;
using namespace rivulus::expressions;
using namespace rivulus::physical_plan;

namespace {

const std::vector<std::string> kNames = {"k", "v", "f", "s", "b"};

// the rows of the test frame on the host: k Int64 over few values with nulls, v Int64 without nulls, f Float64 in quarters with nulls,
// s String with nulls, b Boolean with nulls
struct Rows {
    std::vector<std::optional<int64_t>> k;
    std::vector<int64_t> v;
    std::vector<std::optional<double>> f;
    std::vector<std::optional<std::string>> s;
    std::vector<std::optional<bool>> b;
    size_t size() const { return v.size(); }
};
Rows make_rows(size_t n) {
    Rows r;
    for (size_t i = 0; i < n; ++i) {
        r.k.push_back(i % 11 == 4 ? std::nullopt : std::optional<int64_t>(static_cast<int64_t>((i * 7919 + i / 3) % 9) - 4));
        r.v.push_back(static_cast<int64_t>((i * 104729) % 2001) - 1000);
        r.f.push_back(i % 7 == 2 ? std::nullopt : std::optional<double>(static_cast<double>((i * 31) % 13) * 0.25 - 1.0));
        r.s.push_back(i % 4 == 1 ? std::nullopt : std::optional<std::string>(i % 8 ? "s" + std::to_string(i % 13) : ""));
        r.b.push_back(i % 5 == 3 ? std::nullopt : std::optional<bool>(i % 3 == 0));
    }
    return r;
}
template <class T>
std::shared_ptr<const PrimitiveArray<T>> nullable(const std::vector<std::optional<T>> &cells) {
    std::vector<T> values;
    std::vector<bool> valid;
    bool any_null = false;
    for (auto &c : cells) {
        values.push_back(c.value_or(T{}));
        valid.push_back(c.has_value());
        any_null |= !c.has_value();
    }
    return PrimitiveArray<T>::create(ctx(), values, any_null ? std::optional<std::vector<bool>>(valid) : std::nullopt);
}
DeviceFrame frame_of(const Rows &r) {
    DeviceFrame df;
    df.names = kNames;
    df.columns = {nullable<int64_t>(r.k), Int64Array::from_values(ctx(), r.v), nullable<double>(r.f), StringArray::create(ctx(), r.s), BooleanArray::create(ctx(), r.b)};
    return df;
}
// -1 / 0 / 1 of two cells under one key: nulls first unless nulls_last, `descending` turns the values round and leaves the nulls
template <class T>
int compare_cells(const std::optional<T> &a, const std::optional<T> &b, const SortKey &key) {
    if (!a || !b) {
        if (!a && !b) return 0;
        const int null_side = key.nulls_last ? 1 : -1;
        return !a ? null_side : -null_side;
    }
    const int c = *a < *b ? -1 : *a > *b ? 1 : 0;
    return key.descending ? -c : c;
}
// the rows of `r` that `keep` leaves, in the order sort(keys) gives them: a stable sort of the row numbers
std::vector<size_t> sorted_rows(const Rows &r, const std::vector<SortKey> &keys, const std::function<bool(size_t)> &keep = [](size_t) { return true; }) {
    std::vector<size_t> rows;
    for (size_t i = 0; i < r.size(); ++i)
        if (keep(i)) rows.push_back(i);
    std::stable_sort(rows.begin(), rows.end(), [&](size_t x, size_t y) {
        for (auto &key : keys) {
            int c = 0;
            if (key.column == "k") c = compare_cells(r.k[x], r.k[y], key);
            else if (key.column == "v") c = compare_cells(std::optional<int64_t>(r.v[x]), std::optional<int64_t>(r.v[y]), key);
            else c = compare_cells(r.f[x], r.f[y], key);
            if (c) return c < 0;
        }
        return false;
    });
    return rows;
}
Table table_of(const Rows &r, const std::vector<size_t> &rows) {
    Table t(kNames.size());
    for (size_t i : rows) {
        t[0].push_back(r.k[i] ? std::to_string(*r.k[i]) : "null");
        t[1].push_back(std::to_string(r.v[i]));
        t[2].push_back(r.f[i] ? f17(*r.f[i]) : "null");
        t[3].push_back(r.s[i] ? "'" + *r.s[i] + "'" : "null");
        t[4].push_back(r.b[i] ? (*r.b[i] ? "true" : "false") : "null");
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
Schema kvfsb_schema() {
    return Schema({Field{"k", DataType::Int64, true}, Field{"v", DataType::Int64, true}, Field{"f", DataType::Float64, true}, Field{"s", DataType::String, true},
                   Field{"b", DataType::Boolean, true}});
}

}  // namespace

// ---- planning (no device) -----------------------------------------------------------------------------------------------------------
CPU_TEST(the_schema_is_the_inputs) {
    const Schema in = kvfsb_schema();
    SchemaRef s = sort_schema(in, {{"k", false, false}, {"f", true, true}});
    CHECK(*s == in);
}

CPU_TEST(planning_errors_say_which_column) {
    const Schema s = kvfsb_schema();
    auto why = [&](std::vector<SortKey> keys) { return thrown<SortPlanError>([&] { sort_schema(s, keys); }); };
    CHECK(why({}) == "sort: no sort keys");
    CHECK(why({{"zz", false, false}}) == "sort: unknown key column 'zz'");
    CHECK(why({{"k", false, false}, {"nope", true, false}}) == "sort: unknown key column 'nope'");
    CHECK(why({{"s", false, false}}) == "sort: key column 's' is String; only Int64 and Float64 keys are sorted");
    CHECK(why({{"v", false, false}, {"b", false, true}}) == "sort: key column 'b' is Boolean; only Int64 and Float64 keys are sorted");
    CHECK(why({{"k", true, true}, {"f", false, false}, {"v", true, false}}).empty());
}

// ---- on the device ------------------------------------------------------------------------------------------------------------------
GPU_TEST(eager_sort_over_one_and_two_keys_with_string_and_boolean_columns_riding_along) {
    const Rows r = make_rows(3000);
    const DeviceFrame df = frame_of(r);
    const std::vector<std::vector<SortKey>> key_lists = {{{"v", false, false}}, {{"k", true, false}}, {{"f", false, true}}, {{"k", false, true}, {"f", true, false}},
                                                         {{"f", true, true}, {"k", false, false}}};
    for (auto &keys : key_lists) {
        DeviceFrame got = PhysicalPlan::sort(PhysicalPlan::source(df), keys)->execute();
        CHECK(got.names == kNames && got.height() == r.size());
        for (size_t c = 0; c < kNames.size(); ++c) CHECK(got.columns[c]->data_type() == df.columns[c]->data_type());
        CHECK(cells(got.columns, 0, got.height()) == table_of(r, sorted_rows(r, keys)));
    }
}

GPU_TEST(planning_errors_reach_execute_and_the_context_stays_usable) {
    const Rows r = make_rows(100);
    const DeviceFrame df = frame_of(r);
    CHECK(thrown<SortPlanError>([&] { PhysicalPlan::sort(PhysicalPlan::source(df), {{"zz", false, false}})->execute(); }) == "sort: unknown key column 'zz'");
    CHECK(thrown<SortPlanError>([&] { PhysicalPlan::sort(PhysicalPlan::source(df), {})->execute(); }) == "sort: no sort keys");
    auto plan = StreamingPhysicalPlan::sort(StreamingPhysicalPlan::memory_source(batches_of(df, 16)), {{"s", false, false}});
    CHECK(thrown<SortPlanError>([&] { plan->execute(); }) == "sort: key column 's' is String; only Int64 and Float64 keys are sorted");
    const std::vector<SortKey> keys = {{"k", false, false}};
    DeviceFrame got = PhysicalPlan::sort(PhysicalPlan::source(df), keys)->execute();
    CHECK(cells(got.columns, 0, got.height()) == table_of(r, sorted_rows(r, keys)));
}

GPU_TEST(sort_after_group_by_ranks_the_groups_by_an_aggregate) {
    const Rows r = make_rows(4000);
    const std::vector<AggSpec> aggs = {{AggOp::Sum, "v", "total"}, {AggOp::CountRows, "", "rows"}};
    auto grouped = PhysicalPlan::group_by(PhysicalPlan::source(frame_of(r)), "k", aggs);
    DeviceFrame got = PhysicalPlan::sort(grouped, {{"total", true, false}})->execute();
    CHECK((got.names == std::vector<std::string>{"k", "total", "rows"}));
    // the groups in first-row order, then ranked by their sum, descending, ties in that order
    struct G {
        std::string key;
        int64_t total = 0, rows = 0;
    };
    std::vector<G> groups;
    std::map<std::string, size_t> at;
    for (size_t i = 0; i < r.size(); ++i) {
        const std::string key = r.k[i] ? std::to_string(*r.k[i]) : "null";
        auto it = at.find(key);
        if (it == at.end()) {
            it = at.emplace(key, groups.size()).first;
            groups.push_back(G{key});
        }
        groups[it->second].total += r.v[i];
        ++groups[it->second].rows;
    }
    std::stable_sort(groups.begin(), groups.end(), [](const G &a, const G &b) { return a.total > b.total; });
    Table want(3);
    for (auto &g : groups) {
        want[0].push_back(g.key);
        want[1].push_back(std::to_string(g.total));
        want[2].push_back(std::to_string(g.rows));
    }
    CHECK(got.height() == 10 && cells(got.columns, 0, got.height()) == want);
}

GPU_TEST(filter_then_sort_then_limit_3) {
    const Rows r = make_rows(5000);
    const DeviceFrame df = frame_of(r);
    const std::vector<SortKey> keys = {{"v", true, false}, {"k", false, false}};
    std::vector<size_t> rows = sorted_rows(r, keys, [&](size_t i) { return r.v[i] < 900; });
    rows.resize(3);
    auto filtered = StreamingPhysicalPlan::gpu_filter_project(StreamingPhysicalPlan::memory_source(batches_of(df, 1024)), lower_predicate(Expr::col("v").lt(Expr::lit(900))), kNames);
    auto got = StreamingPhysicalPlan::limit(StreamingPhysicalPlan::sort(filtered, keys), 3)->collect_batches();
    size_t total = 0;
    for (auto &b : got) total += b.num_rows();
    CHECK(total == 3 && !got.empty());
    RecordBatch whole = got.size() == 1 ? got[0] : RecordBatch::concat(got);
    CHECK(cells(whole.columns(), 0, 3) == table_of(r, rows));
    // the eager twin: filter, sort, and the first three rows
    DeviceFrame eager = PhysicalPlan::sort(PhysicalPlan::filter(PhysicalPlan::source(df), CompareTerm{"v", RV_LT, Literal(int64_t{900})}), keys)->execute();
    CHECK(cells(eager.columns, 0, 3) == table_of(r, rows));
}

GPU_TEST(a_stream_over_many_batches_equals_the_eager_sort_and_emits_one_batch) {
    const Rows r = make_rows(2500);
    const DeviceFrame df = frame_of(r);
    const std::vector<SortKey> keys = {{"k", false, true}, {"f", true, false}};
    DeviceFrame eager = PhysicalPlan::sort(PhysicalPlan::source(df), keys)->execute();
    const Table want = table_of(r, sorted_rows(r, keys));
    CHECK(cells(eager.columns, 0, eager.height()) == want);
    for (size_t batch : {size_t{512}, size_t{2500}}) {
        auto stream = StreamingPhysicalPlan::sort(StreamingPhysicalPlan::memory_source(batches_of(df, batch)), keys)->execute();
        CHECK(stream->schema()->num_fields() == kNames.size() && stream->schema()->field(3).name() == "s");
        auto got = stream->collect();
        CHECK(got.size() == 1 && *got[0].schema() == *stream->schema());
        CHECK(got[0].num_rows() == r.size() && cells(got[0].columns(), 0, got[0].num_rows()) == want);
        CHECK(!stream->next_batch());
    }
    // a resident frame is taken whole after the null fill of dataframe_to_batches: Int64 and Float64 nulls are 0 there, String nulls stay
    Rows filled = r;
    for (auto &k : filled.k) k = k.value_or(0);
    for (auto &f : filled.f) f = f.value_or(0.0);
    auto got = StreamingPhysicalPlan::sort(StreamingPhysicalPlan::dataframe_source(df, 1024), keys)->collect_batches();
    CHECK(got.size() == 1 && got[0].num_rows() == r.size());
    const Table resident = cells(got[0].columns(), 0, got[0].num_rows()), expect = table_of(filled, sorted_rows(filled, keys));
    for (size_t c : {size_t{0}, size_t{1}, size_t{2}, size_t{3}}) CHECK(resident[c] == expect[c]);
}

GPU_TEST(an_empty_input_gives_one_zero_row_batch_with_the_schema) {
    const Rows none = make_rows(0);
    const std::vector<SortKey> keys = {{"k", false, false}};
    auto got = StreamingPhysicalPlan::sort(StreamingPhysicalPlan::dataframe_source(frame_of(none), 1024), keys)->collect_batches();
    CHECK(got.size() == 1 && got[0].num_rows() == 0 && got[0].num_columns() == kNames.size());
    CHECK(got[0].column(2)->data_type() == DataType::Float64 && got[0].column(3)->data_type() == DataType::String && got[0].column(4)->len() == 0);
    DeviceFrame eager = PhysicalPlan::sort(PhysicalPlan::source(frame_of(none)), keys)->execute();
    CHECK(eager.height() == 0 && eager.names == kNames && eager.columns[4]->data_type() == DataType::Boolean);
    // a filter that keeps nothing: whatever batches it yields, the sort yields one without rows
    const Rows r = make_rows(2000);
    auto filtered = StreamingPhysicalPlan::gpu_filter_project(StreamingPhysicalPlan::memory_source(batches_of(frame_of(r), 512)), lower_predicate(Expr::col("v").gt(Expr::lit(5000))), kNames);
    auto none_left = StreamingPhysicalPlan::sort(filtered, keys)->collect_batches();
    CHECK(none_left.size() == 1 && none_left[0].num_rows() == 0 && none_left[0].num_columns() == kNames.size() && none_left[0].column(0)->data_type() == DataType::Int64);
}
