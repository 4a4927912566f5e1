// window(partition_by, order_by, exprs) in the host layer (rivulus_amd/host/rivulus_host.hpp): window_schema, PhysicalPlan::window
// (eager, one rv_window) and StreamingPhysicalPlan::window (a pipeline breaker that emits exactly one batch), String partition keys through
// the dictionary.  The frame is the one of sort_host_tests.cpp; the expected columns come from a sequential loop over every partition's
// rows in window order.  Run by tests/test_window_host.py; the scaffold is host_test_main.hpp.
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

// the rows of the test frame on the host (sort_host_tests.cpp's): k Int64 over few values with nulls, v Int64 without nulls, f Float64 in
// quarters with nulls, s String with nulls, b Boolean with nulls
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
int compare_rows(const Rows &r, size_t x, size_t y, const std::vector<SortKey> &keys) {
    for (auto &key : keys) {
        int c = 0;
        if (key.column == "k") c = compare_cells(r.k[x], r.k[y], key);
        else if (key.column == "v") c = compare_cells(std::optional<int64_t>(r.v[x]), std::optional<int64_t>(r.v[y]), key);
        else c = compare_cells(r.f[x], r.f[y], key);
        if (c) return c;
    }
    return 0;
}
// a row's partition as text: the cells of the partition columns, nulls spelled apart from every value
std::string partition_of(const Rows &r, size_t i, const std::vector<std::string> &by) {
    std::string key;
    for (auto &c : by) {
        if (c == "k") key += r.k[i] ? "k" + std::to_string(*r.k[i]) : "k-null";
        else if (c == "s") key += r.s[i] ? "s'" + *r.s[i] + "'" : "s-null";
        else if (c == "b") key += r.b[i] ? (*r.b[i] ? "bT" : "bF") : "b-null";
        else key += "v" + std::to_string(r.v[i]);
        key += "|";
    }
    return key;
}

// The expressions every device case runs, and the model of their columns: per partition a sequential loop over its rows in window order.
const std::vector<WindowExpr> kExprs = {{WindowOp::RowNumber, "", 0, "rn"},    {WindowOp::Rank, "", 0, "rk"},       {WindowOp::DenseRank, "", 0, "dr"},
                                        {WindowOp::CumCount, "s", 0, "cs"},    {WindowOp::CumSum, "v", 0, "total"}, {WindowOp::CumSum, "f", 0, "ftotal"},
                                        {WindowOp::CumMin, "f", 0, "fmin"},    {WindowOp::CumMax, "k", 0, "kmax"},  {WindowOp::Lag, "v", 1, "prev"},
                                        {WindowOp::Lead, "s", 2, "next_s"},    {WindowOp::Lag, "b", 0, "same_b"}};
Table model(const Rows &r, const std::vector<std::string> &by, const std::vector<SortKey> &order) {
    const size_t n = r.size();
    Table t(kExprs.size(), std::vector<std::string>(n));
    std::map<std::string, std::vector<size_t>> parts;
    for (size_t i = 0; i < n; ++i) parts[partition_of(r, i, by)].push_back(i);
    for (auto &entry : parts) {
        std::vector<size_t> &rows = entry.second;
        std::stable_sort(rows.begin(), rows.end(), [&](size_t x, size_t y) { return compare_rows(r, x, y, order) < 0; });
        int64_t rank = 0, dense = 0, count_s = 0, total = 0;
        double ftotal = 0.0;  // quarters: every partial sum is exact
        std::optional<double> fmin;
        std::optional<int64_t> kmax;
        for (size_t p = 0; p < rows.size(); ++p) {
            const size_t i = rows[p];
            if (p == 0 || compare_rows(r, rows[p - 1], i, order) != 0) {
                rank = static_cast<int64_t>(p) + 1;
                ++dense;
            }
            count_s += r.s[i].has_value();
            total += r.v[i];
            if (r.f[i]) ftotal += *r.f[i];
            if (r.f[i] && (!fmin || *r.f[i] < *fmin)) fmin = r.f[i];
            if (r.k[i] && (!kmax || *r.k[i] > *kmax)) kmax = r.k[i];
            t[0][i] = std::to_string(p + 1);
            t[1][i] = std::to_string(rank);
            t[2][i] = std::to_string(dense);
            t[3][i] = std::to_string(count_s);
            t[4][i] = std::to_string(total);
            t[5][i] = f17(ftotal + 0.0);
            t[6][i] = fmin ? f17(*fmin) : "null";
            t[7][i] = kmax ? std::to_string(*kmax) : "null";
            t[8][i] = p >= 1 ? std::to_string(r.v[rows[p - 1]]) : "null";
            t[9][i] = p + 2 < rows.size() && r.s[rows[p + 2]] ? "'" + *r.s[rows[p + 2]] + "'" : "null";
            t[10][i] = r.b[i] ? (*r.b[i] ? "true" : "false") : "null";
        }
    }
    return t;
}
Table input_table(const Rows &r) {
    Table t(kNames.size());
    for (size_t i = 0; i < r.size(); ++i) {
        t[0].push_back(r.k[i] ? std::to_string(*r.k[i]) : "null");
        t[1].push_back(std::to_string(r.v[i]));
        t[2].push_back(r.f[i] ? f17(*r.f[i]) : "null");
        t[3].push_back(r.s[i] ? "'" + *r.s[i] + "'" : "null");
        t[4].push_back(r.b[i] ? (*r.b[i] ? "true" : "false") : "null");
    }
    return t;
}
Table whole(const Rows &r, const std::vector<std::string> &by, const std::vector<SortKey> &order) {
    Table t = input_table(r);
    for (auto &c : model(r, by, order)) t.push_back(c);
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
std::vector<std::string> names_with_aliases() {
    std::vector<std::string> names = kNames;
    for (auto &e : kExprs) names.push_back(e.alias);
    return names;
}

}  // namespace

// ---- planning (no device) -----------------------------------------------------------------------------------------------------------
CPU_TEST(the_schema_is_the_inputs_plus_one_field_per_expression) {
    const Schema in = kvfsb_schema();
    SchemaRef s = window_schema(in, {"k", "s"}, {{"v", true, false}}, kExprs);
    CHECK(s->num_fields() == kNames.size() + kExprs.size());
    for (size_t c = 0; c < kNames.size(); ++c) CHECK(s->field(c).name() == kNames[c] && s->field(c).data_type() == in.field(c).data_type());
    const std::vector<DataType> want = {DataType::Int64,   DataType::Int64,   DataType::Int64, DataType::Int64, DataType::Int64,  DataType::Float64,
                                        DataType::Float64, DataType::Int64, DataType::Int64, DataType::String, DataType::Boolean};
    for (size_t j = 0; j < kExprs.size(); ++j) CHECK(s->field(kNames.size() + j).name() == kExprs[j].alias && s->field(kNames.size() + j).data_type() == want[j]);
    CHECK(window_schema(in, {}, {}, {{WindowOp::RowNumber, "", 0, "n"}})->field(5).name() == "n");
}

CPU_TEST(planning_errors_say_which_column) {
    const Schema s = kvfsb_schema();
    const std::vector<WindowExpr> one = {{WindowOp::RowNumber, "", 0, "rn"}};
    auto why = [&](std::vector<std::string> by, std::vector<SortKey> order, std::vector<WindowExpr> exprs) {
        return thrown<WindowPlanError>([&] { window_schema(s, by, order, exprs); });
    };
    CHECK(why({"k"}, {}, {}) == "window: no window expressions");
    CHECK(why({"zz"}, {}, one) == "window: unknown partition column 'zz'");
    CHECK(why({"k"}, {{"nope", false, false}}, one) == "window: unknown order column 'nope'");
    CHECK(why({}, {{"s", false, false}}, one) == "window: order column 's' is String; only Int64 and Float64 keys are sorted");
    CHECK(why({}, {{"v", false, false}, {"b", true, false}}, one) == "window: order column 'b' is Boolean; only Int64 and Float64 keys are sorted");
    CHECK(why({}, {}, {{WindowOp::CumSum, "zz", 0, "t"}}) == "window: expression 't' reads the unknown column 'zz'");
    CHECK(why({}, {}, {{WindowOp::Lag, "zz", 1, "t"}}) == "window: expression 't' reads the unknown column 'zz'");
    CHECK(why({}, {}, {{WindowOp::CumSum, "s", 0, "t"}}) == "window: CUM_SUM over column 's' of dtype String");
    CHECK(why({}, {}, {{WindowOp::CumMin, "b", 0, "t"}}) == "window: CUM_MIN over column 'b' of dtype Boolean");
    CHECK(why({}, {}, {{WindowOp::CumMax, "s", 0, "t"}}) == "window: CUM_MAX over column 's' of dtype String");
    CHECK(why({}, {}, {{WindowOp::CumSum, "v", 0, ""}}) == "window: the CUM_SUM expression over column 'v' has no alias");
    CHECK(why({}, {}, {{WindowOp::CumSum, "v", 0, "t"}, {WindowOp::Rank, "", 0, "t"}}) == "window: duplicate output name 't'");
    CHECK(why({}, {}, {{WindowOp::CumSum, "v", 0, "k"}}) == "window: duplicate output name 'k'");
    CHECK(why(std::vector<std::string>(9, "k"), {}, one) == "window: 9 partition columns; at most 8 are taken");
    CHECK(why({"s", "b", "f"}, {{"k", true, true}, {"f", false, false}}, kExprs).empty());
}

// ---- on the device ------------------------------------------------------------------------------------------------------------------
GPU_TEST(eager_window_against_the_sequential_loop) {
    const Rows r = make_rows(3000);
    const DeviceFrame df = frame_of(r);
    struct Shape {
        std::vector<std::string> by;
        std::vector<SortKey> order;
    };
    const std::vector<Shape> shapes = {{{"k"}, {{"v", false, false}}}, {{"k"}, {{"f", true, true}}}, {{"b", "k"}, {{"f", false, false}, {"v", true, false}}},
                                       {{}, {{"k", false, true}}},     {{"k"}, {}},                  {{}, {}}};
    for (auto &shape : shapes) {
        DeviceFrame got = PhysicalPlan::window(PhysicalPlan::source(df), shape.by, shape.order, kExprs)->execute();
        CHECK(got.names == names_with_aliases() && got.height() == r.size() && got.columns.size() == kNames.size() + kExprs.size());
        CHECK(cells(got.columns, 0, got.height()) == whole(r, shape.by, shape.order));
    }
}

GPU_TEST(a_string_partition_key_goes_through_the_dictionary) {
    const Rows r = make_rows(2000);
    const DeviceFrame df = frame_of(r);
    for (const std::vector<std::string> &by : {std::vector<std::string>{"s"}, std::vector<std::string>{"k", "s"}, std::vector<std::string>{"s", "b"}}) {
        const std::vector<SortKey> order = {{"v", true, false}};
        DeviceFrame got = PhysicalPlan::window(PhysicalPlan::source(df), by, order, kExprs)->execute();
        CHECK(got.columns.size() == kNames.size() + kExprs.size());  // the ids of the String key are no column of the result
        CHECK(cells(got.columns, 0, got.height()) == whole(r, by, order));
    }
}

GPU_TEST(planning_errors_reach_execute_and_the_context_stays_usable) {
    const Rows r = make_rows(100);
    const DeviceFrame df = frame_of(r);
    const std::vector<WindowExpr> one = {{WindowOp::RowNumber, "", 0, "rn"}};
    CHECK(thrown<WindowPlanError>([&] { PhysicalPlan::window(PhysicalPlan::source(df), {"zz"}, {}, one)->execute(); }) == "window: unknown partition column 'zz'");
    CHECK(thrown<WindowPlanError>([&] { PhysicalPlan::window(PhysicalPlan::source(df), {}, {}, {})->execute(); }) == "window: no window expressions");
    auto plan = StreamingPhysicalPlan::window(StreamingPhysicalPlan::memory_source(batches_of(df, 16)), {}, {{"s", false, false}}, one);
    CHECK(thrown<WindowPlanError>([&] { plan->execute(); }) == "window: order column 's' is String; only Int64 and Float64 keys are sorted");
    DeviceFrame got = PhysicalPlan::window(PhysicalPlan::source(df), {"k"}, {{"v", false, false}}, kExprs)->execute();
    CHECK(cells(got.columns, 0, got.height()) == whole(r, {"k"}, {{"v", false, false}}));
}

GPU_TEST(a_stream_over_many_batches_equals_the_eager_window_and_emits_one_batch) {
    const Rows r = make_rows(2500);
    const DeviceFrame df = frame_of(r);
    const std::vector<std::string> by = {"k"};
    const std::vector<SortKey> order = {{"f", true, false}, {"v", false, false}};
    const Table want = whole(r, by, order);
    DeviceFrame eager = PhysicalPlan::window(PhysicalPlan::source(df), by, order, kExprs)->execute();
    CHECK(cells(eager.columns, 0, eager.height()) == want);
    for (size_t batch : {size_t{512}, size_t{2500}}) {
        auto stream = StreamingPhysicalPlan::window(StreamingPhysicalPlan::memory_source(batches_of(df, batch)), by, order, kExprs)->execute();
        CHECK(stream->schema()->num_fields() == kNames.size() + kExprs.size() && stream->schema()->field(5).name() == "rn");
        auto got = stream->collect();
        CHECK(got.size() == 1 && *got[0].schema() == *stream->schema());
        CHECK(got[0].num_rows() == r.size() && cells(got[0].columns(), 0, got[0].num_rows()) == want);
        CHECK(!stream->next_batch());
    }
    // a resident frame is taken whole after the null fill of dataframe_to_batches: Int64 and Float64 nulls are 0 there, String nulls stay
    Rows filled = r;
    for (auto &k : filled.k) k = k.value_or(0);
    for (auto &f : filled.f) f = f.value_or(0.0);
    auto got = StreamingPhysicalPlan::window(StreamingPhysicalPlan::dataframe_source(df, 1024), by, order, kExprs)->collect_batches();
    CHECK(got.size() == 1 && got[0].num_rows() == r.size());
    const Table resident = cells(got[0].columns(), 0, got[0].num_rows()), expect = whole(filled, by, order);
    for (size_t c = 0; c < expect.size(); ++c)
        if (c != 4 && c != kNames.size() + 10) CHECK(resident[c] == expect[c]);  // (the Boolean column and its copy: the fill's business)
}

GPU_TEST(an_empty_input_gives_one_zero_row_batch_with_the_schema) {
    const Rows none = make_rows(0);
    auto got = StreamingPhysicalPlan::window(StreamingPhysicalPlan::dataframe_source(frame_of(none), 1024), {"k"}, {{"v", false, false}}, kExprs)->collect_batches();
    CHECK(got.size() == 1 && got[0].num_rows() == 0 && got[0].num_columns() == kNames.size() + kExprs.size());
    CHECK(got[0].column(5)->data_type() == DataType::Int64 && got[0].column(10)->data_type() == DataType::Float64 && got[0].column(14)->data_type() == DataType::String);
    DeviceFrame eager = PhysicalPlan::window(PhysicalPlan::source(frame_of(none)), {"s"}, {{"v", false, false}}, kExprs)->execute();
    CHECK(eager.height() == 0 && eager.names == names_with_aliases() && eager.columns[15]->data_type() == DataType::Boolean);
    // a filter that keeps nothing: whatever batches it yields, the window yields one without rows
    const Rows r = make_rows(2000);
    auto filtered = StreamingPhysicalPlan::gpu_filter_project(StreamingPhysicalPlan::memory_source(batches_of(frame_of(r), 512)), lower_predicate(Expr::col("v").gt(Expr::lit(5000))), kNames);
    auto none_left = StreamingPhysicalPlan::window(filtered, {"k"}, {}, kExprs)->collect_batches();
    CHECK(none_left.size() == 1 && none_left[0].num_rows() == 0 && none_left[0].num_columns() == kNames.size() + kExprs.size());
}
