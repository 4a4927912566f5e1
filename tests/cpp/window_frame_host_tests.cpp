// Window frames in the host layer (rivulus_amd/host/rivulus_host.hpp): the new WindowOps through window_schema, PhysicalPlan::window (eager,
// one rv_window_frames) and StreamingPhysicalPlan::window -- a moving average, a share of the partition's total, FIRST / LAST_VALUE over a
// String column and NTILE -- String partition keys through the dictionary, empty input.  The expected columns come from a sequential loop
// over every frame's rows.  Run by tests/test_window_frame_host.py; the scaffold is host_test_main.hpp.
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

const std::vector<std::string> kNames = {"k", "v", "f", "s"};
constexpr int64_t kEdge = RV_FRAME_UNBOUNDED;

// k Int64 over few values with nulls, v Int64 without nulls, f Float64 in quarters with nulls (every partial sum exact), s String with nulls
struct Rows {
    std::vector<std::optional<int64_t>> k;
    std::vector<int64_t> v;
    std::vector<std::optional<double>> f;
    std::vector<std::optional<std::string>> s;
    size_t size() const { return v.size(); }
};
Rows make_rows(size_t n) {
    Rows r;
    for (size_t i = 0; i < n; ++i) {
        r.k.push_back(i % 11 == 4 ? std::nullopt : std::optional<int64_t>(static_cast<int64_t>((i * 7919 + i / 3) % 9) - 4));
        r.v.push_back(static_cast<int64_t>((i * 104729) % 2001) - 1000);
        r.f.push_back(i % 7 == 2 ? std::nullopt : std::optional<double>(static_cast<double>((i * 31) % 13) * 0.25 - 1.0));
        r.s.push_back(i % 4 == 1 ? std::nullopt : std::optional<std::string>(i % 8 ? "s" + std::to_string(i % 13) : ""));
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
    df.columns = {nullable<int64_t>(r.k), Int64Array::from_values(ctx(), r.v), nullable<double>(r.f), StringArray::create(ctx(), r.s)};
    return df;
}
std::string partition_of(const Rows &r, size_t i, const std::vector<std::string> &by) {
    std::string key;
    for (auto &c : by) {
        if (c == "k") key += r.k[i] ? "k" + std::to_string(*r.k[i]) : "k-null";
        else key += r.s[i] ? "s'" + *r.s[i] + "'" : "s-null";
        key += "|";
    }
    return key;
}

// a moving average, a share of the total (its two halves), "the three rows before", FIRST / LAST over the String column, NTILE, and a
// numbering of rv_window's in the same call
const std::vector<WindowExpr> kExprs = {{WindowOp::Avg, "f", 0, "favg", 2, 0},          {WindowOp::Sum, "v", 0, "vtotal", kEdge, kEdge},
                                        {WindowOp::Avg, "v", 0, "vavg", 3, 3},          {WindowOp::Sum, "f", 0, "fsum", 1, 1},
                                        {WindowOp::Min, "f", 0, "fmin", 3, -1},         {WindowOp::Max, "v", 0, "vmax", 0, kEdge},
                                        {WindowOp::Count, "s", 0, "ns", 1, 1},          {WindowOp::FirstValue, "s", 0, "s_first", 1, 0},
                                        {WindowOp::LastValue, "s", 0, "s_last", 0, 2},  {WindowOp::Ntile, "", 4, "quartile"},
                                        {WindowOp::RowNumber, "", 0, "rn"},             {WindowOp::Sum, "v", 0, "running"}};
Table model(const Rows &r, const std::vector<std::string> &by, bool by_v_descending) {
    const size_t n = r.size();
    Table t(kExprs.size(), std::vector<std::string>(n));
    std::map<std::string, std::vector<size_t>> parts;
    for (size_t i = 0; i < n; ++i) parts[partition_of(r, i, by)].push_back(i);
    for (auto &entry : parts) {
        std::vector<size_t> &rows = entry.second;
        if (by_v_descending) std::stable_sort(rows.begin(), rows.end(), [&](size_t x, size_t y) { return r.v[x] > r.v[y]; });
        const int64_t len = static_cast<int64_t>(rows.size());
        for (int64_t p = 0; p < len; ++p) {
            const size_t i = rows[p];
            for (size_t j = 0; j < kExprs.size(); ++j) {
                const WindowExpr &e = kExprs[j];
                if (e.op == WindowOp::RowNumber) {
                    t[j][i] = std::to_string(p + 1);
                    continue;
                }
                if (e.op == WindowOp::Ntile) {  // deal the rows out: the first len % 4 buckets take one more
                    int64_t bucket = 0, left = p + 1;
                    while (left > 0) left -= len / 4 + (++bucket <= len % 4 ? 1 : 0);
                    t[j][i] = std::to_string(bucket);
                    continue;
                }
                const int64_t lo = e.preceding == kEdge ? 0 : std::max<int64_t>(0, p - e.preceding), hi = e.following == kEdge ? len - 1 : std::min(len - 1, p + e.following);
                int64_t count = 0, vsum = 0;
                double fsum = 0.0;
                std::optional<double> fmin;
                std::optional<int64_t> vmax;
                for (int64_t q = lo; q <= hi; ++q) {
                    const size_t x = rows[q];
                    if (e.column == "v") ++count, vsum += r.v[x], vmax = vmax ? std::max(*vmax, r.v[x]) : r.v[x];
                    else if (e.column == "f" && r.f[x]) ++count, fsum += *r.f[x], fmin = fmin ? std::min(*fmin, *r.f[x]) : *r.f[x];
                    else if (e.column == "s" && r.s[x]) ++count;
                }
                std::string cell = "null";
                switch (e.op) {
                    case WindowOp::Count: cell = std::to_string(count); break;
                    case WindowOp::Sum: cell = e.column == "v" ? std::to_string(vsum) : f17(fsum + 0.0); break;
                    case WindowOp::Avg:
                        if (count) cell = f17((e.column == "v" ? static_cast<double>(vsum) : fsum) / static_cast<double>(count));
                        break;
                    case WindowOp::Min:
                        if (fmin) cell = f17(*fmin);
                        break;
                    case WindowOp::Max:
                        if (vmax) cell = std::to_string(*vmax);
                        break;
                    case WindowOp::FirstValue:
                        if (lo <= hi && r.s[rows[lo]]) cell = "'" + *r.s[rows[lo]] + "'";
                        break;
                    case WindowOp::LastValue:
                        if (lo <= hi && r.s[rows[hi]]) cell = "'" + *r.s[rows[hi]] + "'";
                        break;
                    default: break;
                }
                t[j][i] = cell;
            }
        }
    }
    return t;
}
Table whole(const Rows &r, const std::vector<std::string> &by, bool by_v_descending) {
    Table t(kNames.size());
    for (size_t i = 0; i < r.size(); ++i) {
        t[0].push_back(r.k[i] ? std::to_string(*r.k[i]) : "null");
        t[1].push_back(std::to_string(r.v[i]));
        t[2].push_back(r.f[i] ? f17(*r.f[i]) : "null");
        t[3].push_back(r.s[i] ? "'" + *r.s[i] + "'" : "null");
    }
    for (auto &c : model(r, by, by_v_descending)) t.push_back(c);
    return t;
}
std::vector<SortKey> order_of(bool by_v_descending) { return by_v_descending ? std::vector<SortKey>{{"v", true, false}} : std::vector<SortKey>{}; }
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
Schema kvfs_schema() {
    return Schema({Field{"k", DataType::Int64, true}, Field{"v", DataType::Int64, true}, Field{"f", DataType::Float64, true}, Field{"s", DataType::String, true}});
}

}  // namespace

// ---- planning (no device) -----------------------------------------------------------------------------------------------------------
CPU_TEST(the_ops_follow_the_c_enums) {
    CHECK(static_cast<int>(WindowOp::Lead) == RV_WIN_LEAD && static_cast<int>(WindowOp::Count) == RV_WINF_COUNT && static_cast<int>(WindowOp::Sum) == RV_WINF_SUM);
    CHECK(static_cast<int>(WindowOp::Min) == RV_WINF_MIN && static_cast<int>(WindowOp::Max) == RV_WINF_MAX && static_cast<int>(WindowOp::Avg) == RV_WINF_AVG);
    CHECK(static_cast<int>(WindowOp::FirstValue) == RV_WINF_FIRST_VALUE && static_cast<int>(WindowOp::LastValue) == RV_WINF_LAST_VALUE);
    CHECK(static_cast<int>(WindowOp::Ntile) == RV_WINF_NTILE);
    const WindowExpr plain{WindowOp::Sum, "v", 0, "t"};  // the frame defaults to the running one
    CHECK(plain.preceding == RV_FRAME_UNBOUNDED && plain.following == 0);
}

CPU_TEST(the_schema_knows_the_new_ops) {
    const Schema in = kvfs_schema();
    SchemaRef s = window_schema(in, {"k", "s"}, {{"v", true, false}}, kExprs);
    CHECK(s->num_fields() == kNames.size() + kExprs.size());
    const std::vector<DataType> want = {DataType::Float64, DataType::Int64, DataType::Float64, DataType::Float64, DataType::Float64, DataType::Int64,
                                        DataType::Int64,   DataType::String, DataType::String, DataType::Int64,   DataType::Int64,   DataType::Int64};
    const std::vector<bool> nullable_out = {true, false, true, false, true, true, false, true, true, false, false, false};
    for (size_t j = 0; j < kExprs.size(); ++j) {
        const Field &f = s->field(kNames.size() + j);
        CHECK(f.name() == kExprs[j].alias && f.data_type() == want[j] && f.is_nullable() == nullable_out[j]);
    }
}

CPU_TEST(planning_errors_name_the_column_and_the_alias) {
    const Schema s = kvfs_schema();
    auto why = [&](std::vector<WindowExpr> exprs) { return thrown<WindowPlanError>([&] { window_schema(s, {}, {}, exprs); }); };
    CHECK(why({{WindowOp::Sum, "s", 0, "t", 1, 1}}) == "window: SUM over column 's' of dtype String (expression 't')");
    CHECK(why({{WindowOp::Min, "s", 0, "lo", 1, 1}}) == "window: MIN over column 's' of dtype String (expression 'lo')");
    CHECK(why({{WindowOp::Max, "s", 0, "hi", 1, 1}}) == "window: MAX over column 's' of dtype String (expression 'hi')");
    CHECK(why({{WindowOp::Avg, "s", 0, "m", 1, 1}}) == "window: AVG over column 's' of dtype String (expression 'm')");
    CHECK(why({{WindowOp::Ntile, "", 0, "q"}}) == "window: NTILE expression 'q' has 0 buckets");
    CHECK(why({{WindowOp::Sum, "v", 0, "t", 1, -2}}) == "window: the frame of the SUM expression 't' over column 'v' has preceding + following < 0");
    CHECK(why({{WindowOp::FirstValue, "s", 0, "a", -1, 0}}) == "window: the frame of the FIRST_VALUE expression 'a' over column 's' has preceding + following < 0");
    CHECK(why({{WindowOp::Count, "s", 0, "c", (int64_t{1} << 62) + 1, 0}}) == "window: the frame of the COUNT expression 'c' over column 's' has a finite offset beyond 2^62");
    CHECK(why({{WindowOp::Avg, "zz", 0, "t", 1, 1}}) == "window: expression 't' reads the unknown column 'zz'");
    CHECK(why({{WindowOp::Sum, "v", 0, "", 1, 1}}) == "window: the SUM expression over column 'v' has no alias");
    CHECK(why({{WindowOp::Count, "s", 0, "c", 1, 1}, {WindowOp::Ntile, "", 2, "c"}}) == "window: duplicate output name 'c'");
    CHECK(why({{WindowOp::CumSum, "v", 0, "t", 1, -2}, {WindowOp::Lag, "s", 1, "u", -5, 0}, {WindowOp::Ntile, "nowhere", 3, "q", 0, -9}}).empty());  // the frame is not theirs
    CHECK(why({{WindowOp::Sum, "v", 0, "t", int64_t{1} << 62, -(int64_t{1} << 62)}, {WindowOp::Max, "f", 0, "u", -3, kEdge}, {WindowOp::LastValue, "s", 0, "w", kEdge, -7}}).empty());
}

// ---- on the device ------------------------------------------------------------------------------------------------------------------
GPU_TEST(eager_frames_against_the_sequential_loop) {
    const Rows r = make_rows(3000);
    const DeviceFrame df = frame_of(r);
    for (bool ordered : {true, false})
        for (const std::vector<std::string> &by : {std::vector<std::string>{"k"}, std::vector<std::string>{}}) {
            DeviceFrame got = PhysicalPlan::window(PhysicalPlan::source(df), by, order_of(ordered), kExprs)->execute();
            CHECK(got.height() == r.size() && got.columns.size() == kNames.size() + kExprs.size() && got.names.back() == "running");
            CHECK(cells(got.columns, 0, got.height()) == whole(r, by, ordered));
        }
}

GPU_TEST(a_string_partition_key_goes_through_the_dictionary) {
    const Rows r = make_rows(2000);
    const DeviceFrame df = frame_of(r);
    for (const std::vector<std::string> &by : {std::vector<std::string>{"s"}, std::vector<std::string>{"k", "s"}}) {
        DeviceFrame got = PhysicalPlan::window(PhysicalPlan::source(df), by, order_of(true), kExprs)->execute();
        CHECK(got.columns.size() == kNames.size() + kExprs.size());  // the ids of the String key are no column of the result
        CHECK(cells(got.columns, 0, got.height()) == whole(r, by, true));
    }
}

GPU_TEST(planning_errors_reach_execute_and_the_context_stays_usable) {
    const Rows r = make_rows(100);
    const DeviceFrame df = frame_of(r);
    CHECK(thrown<WindowPlanError>([&] { PhysicalPlan::window(PhysicalPlan::source(df), {}, {}, {{WindowOp::Ntile, "", 0, "q"}})->execute(); }) ==
          "window: NTILE expression 'q' has 0 buckets");
    auto plan = StreamingPhysicalPlan::window(StreamingPhysicalPlan::memory_source(batches_of(df, 16)), {}, {}, {{WindowOp::Avg, "s", 0, "m", 1, 1}});
    CHECK(thrown<WindowPlanError>([&] { plan->execute(); }) == "window: AVG over column 's' of dtype String (expression 'm')");
    DeviceFrame got = PhysicalPlan::window(PhysicalPlan::source(df), {"k"}, order_of(true), kExprs)->execute();
    CHECK(cells(got.columns, 0, got.height()) == whole(r, {"k"}, true));
}

GPU_TEST(a_stream_over_many_batches_equals_the_eager_window_and_emits_one_batch) {
    const Rows r = make_rows(2500);
    const DeviceFrame df = frame_of(r);
    const std::vector<std::string> by = {"k"};
    const Table want = whole(r, by, true);
    for (size_t batch : {size_t{512}, size_t{2500}}) {
        auto stream = StreamingPhysicalPlan::window(StreamingPhysicalPlan::memory_source(batches_of(df, batch)), by, order_of(true), kExprs)->execute();
        CHECK(stream->schema()->num_fields() == kNames.size() + kExprs.size() && stream->schema()->field(4).name() == "favg");
        auto got = stream->collect();
        CHECK(got.size() == 1 && *got[0].schema() == *stream->schema());
        CHECK(got[0].num_rows() == r.size() && cells(got[0].columns(), 0, got[0].num_rows()) == want);
        CHECK(!stream->next_batch());
    }
}

GPU_TEST(an_empty_input_gives_one_zero_row_batch_with_the_schema) {
    const Rows none = make_rows(0);
    auto got = StreamingPhysicalPlan::window(StreamingPhysicalPlan::dataframe_source(frame_of(none), 1024), {"k"}, order_of(true), kExprs)->collect_batches();
    CHECK(got.size() == 1 && got[0].num_rows() == 0 && got[0].num_columns() == kNames.size() + kExprs.size());
    CHECK(got[0].column(4)->data_type() == DataType::Float64 && got[0].column(5)->data_type() == DataType::Int64 && got[0].column(11)->data_type() == DataType::String);
    DeviceFrame eager = PhysicalPlan::window(PhysicalPlan::source(frame_of(none)), {"s"}, {}, kExprs)->execute();
    CHECK(eager.height() == 0 && eager.columns.size() == kNames.size() + kExprs.size() && eager.columns[13]->data_type() == DataType::Int64);
}
