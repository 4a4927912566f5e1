// top_k(keys, k) in the host layer (rivulus_amd/host/rivulus_host.hpp): top_k_schema, PhysicalPlan::top_k (eager, one rv_top_k) and
// StreamingPhysicalPlan::top_k (GpuTopKStream: a pipeline breaker that folds its input and emits exactly one batch), with String and
// Boolean columns riding along.  Run by tests/test_topk_host.py; the scaffold is host_test_main.hpp.
#include <algorithm>
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
// the first k rows of `r` in the order sort(keys) gives them: a stable sort of the row numbers, cut
std::vector<size_t> first_rows(const Rows &r, const std::vector<SortKey> &keys, size_t k) {
    std::vector<size_t> rows(r.size());
    for (size_t i = 0; i < r.size(); ++i) rows[i] = i;
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
    rows.resize(std::min(k, rows.size()));
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
const std::vector<std::vector<SortKey>> kKeyLists = {{{"v", false, false}}, {{"k", true, false}}, {{"f", false, true}}, {{"k", false, true}, {"f", true, false}},
                                                     {{"f", true, true}, {"k", false, false}, {"v", true, false}}};

}  // namespace

// ---- planning (no device) -----------------------------------------------------------------------------------------------------------
CPU_TEST(the_schema_is_the_inputs) {
    const Schema in = kvfsb_schema();
    for (size_t k : {size_t{0}, size_t{1}, size_t{1000}}) CHECK(*top_k_schema(in, {{"k", false, false}, {"f", true, true}}, k) == in);
}

CPU_TEST(planning_errors_are_the_sorts_with_the_same_texts) {
    const Schema s = kvfsb_schema();
    const std::vector<std::vector<SortKey>> bad = {{}, {{"zz", false, false}}, {{"k", false, false}, {"nope", true, false}}, {{"s", false, false}},
                                                   {{"v", false, false}, {"b", false, true}}};
    for (auto &keys : bad) {
        const std::string sort_says = thrown<SortPlanError>([&] { sort_schema(s, keys); });
        CHECK(!sort_says.empty() && thrown<SortPlanError>([&] { top_k_schema(s, keys, 5); }) == sort_says);
    }
    CHECK(thrown<SortPlanError>([&] { top_k_schema(s, {}, 5); }) == "sort: no sort keys");
    CHECK(thrown<SortPlanError>([&] { top_k_schema(s, {{"s", false, false}}, 0); }) == "sort: key column 's' is String; only Int64 and Float64 keys are sorted");
    CHECK(thrown<SortPlanError>([&] { top_k_schema(s, {{"k", true, true}, {"f", false, false}, {"v", true, false}}, 3); }).empty());
}

// ---- on the device ------------------------------------------------------------------------------------------------------------------
GPU_TEST(eager_top_k_equals_the_eager_sort_cut_at_k) {
    const Rows r = make_rows(3000);
    const DeviceFrame df = frame_of(r);
    for (int64_t select_from : {int64_t{0}, int64_t{1}}) {  // the built-in crossover (these rows are sorted whole), and the select forced
        check(rv_ctx_set_option(ctx()->raw(), "top_k_select_from_rows", select_from));
        for (auto &keys : kKeyLists) {
            DeviceFrame sorted = PhysicalPlan::sort(PhysicalPlan::source(df), keys)->execute();
            for (size_t k : {size_t{0}, size_t{1}, size_t{37}, size_t{1499}, size_t{1500}, size_t{3000}, size_t{5000}}) {
                DeviceFrame got = PhysicalPlan::top_k(PhysicalPlan::source(df), keys, k)->execute();
                const size_t rows = std::min(k, r.size());
                CHECK(got.names == kNames && got.height() == rows);
                for (size_t c = 0; c < kNames.size(); ++c) CHECK(got.columns[c]->data_type() == df.columns[c]->data_type());
                CHECK(cells(got.columns, 0, rows) == cells(sorted.columns, 0, rows));
                CHECK(cells(got.columns, 0, rows) == table_of(r, first_rows(r, keys, k)));
            }
        }
    }
    check(rv_ctx_set_option(ctx()->raw(), "top_k_select_from_rows", 0));
}

GPU_TEST(the_select_path_runs_under_the_eager_plan) {
    // the select forced at this size, and a key with many distinct values: the candidates are few
    check(rv_ctx_set_option(ctx()->raw(), "top_k_select_from_rows", 1));
    const size_t n = 200000;
    std::vector<int64_t> v(n), w(n);
    for (size_t i = 0; i < n; ++i) {
        v[i] = static_cast<int64_t>((i * 2654435761ull) % 1000003) - 500000;
        w[i] = static_cast<int64_t>(i);
    }
    DeviceFrame df;
    df.names = {"v", "w"};
    df.columns = {Int64Array::from_values(ctx(), v), Int64Array::from_values(ctx(), w)};
    DeviceFrame got = PhysicalPlan::top_k(PhysicalPlan::source(df), {{"v", true, false}}, 25)->execute();
    int64_t passes = 0;
    check(rv_ctx_get_option(ctx()->raw(), "top_k_last_passes", &passes));
    CHECK(passes >= 1);
    check(rv_ctx_set_option(ctx()->raw(), "top_k_select_from_rows", 0));
    DeviceFrame sorted = PhysicalPlan::sort(PhysicalPlan::source(df), {{"v", true, false}})->execute();
    CHECK(got.height() == 25 && cells(got.columns, 0, 25) == cells(sorted.columns, 0, 25));
}

GPU_TEST(planning_errors_reach_execute_and_the_context_stays_usable) {
    const Rows r = make_rows(100);
    const DeviceFrame df = frame_of(r);
    CHECK(thrown<SortPlanError>([&] { PhysicalPlan::top_k(PhysicalPlan::source(df), {{"zz", false, false}}, 3)->execute(); }) == "sort: unknown key column 'zz'");
    CHECK(thrown<SortPlanError>([&] { PhysicalPlan::top_k(PhysicalPlan::source(df), {}, 3)->execute(); }) == "sort: no sort keys");
    auto plan = StreamingPhysicalPlan::top_k(StreamingPhysicalPlan::memory_source(batches_of(df, 16)), {{"s", false, false}}, 3);
    CHECK(thrown<SortPlanError>([&] { plan->execute(); }) == "sort: key column 's' is String; only Int64 and Float64 keys are sorted");
    const std::vector<SortKey> keys = {{"k", false, false}};
    DeviceFrame got = PhysicalPlan::top_k(PhysicalPlan::source(df), keys, 7)->execute();
    CHECK(cells(got.columns, 0, got.height()) == table_of(r, first_rows(r, keys, 7)));
}

GPU_TEST(a_stream_over_a_resident_frame_is_one_top_k) {
    const Rows r = make_rows(2500);
    const DeviceFrame df = frame_of(r);
    const std::vector<SortKey> keys = {{"k", false, true}, {"f", true, false}};
    // a resident frame is taken whole after the null fill of dataframe_to_batches: Int64 and Float64 nulls are 0 there, String nulls stay
    Rows filled = r;
    for (auto &k : filled.k) k = k.value_or(0);
    for (auto &f : filled.f) f = f.value_or(0.0);
    auto stream = StreamingPhysicalPlan::top_k(StreamingPhysicalPlan::dataframe_source(df, 1024), keys, 40)->execute();
    auto got = stream->collect();
    CHECK(got.size() == 1 && got[0].num_rows() == 40 && !stream->next_batch());
    CHECK(dynamic_cast<GpuTopKStream *>(stream.get()) && dynamic_cast<GpuTopKStream *>(stream.get())->folds() == 1);
    const Table resident = cells(got[0].columns(), 0, 40), expect = table_of(filled, first_rows(filled, keys, 40));
    for (size_t c : {size_t{0}, size_t{1}, size_t{2}, size_t{3}}) CHECK(resident[c] == expect[c]);
}

GPU_TEST(a_stream_of_batches_folds_several_times_and_keeps_equal_keys_in_input_order) {
    // k takes nine values and nulls over 300 rows that arrive two at a time: every key of the answer ties with rows of many other batches
    const Rows r = make_rows(300);
    const DeviceFrame df = frame_of(r);
    for (auto &keys : kKeyLists) {
        // the folds of the two-key lists run the select (forced at this size), the others the whole sort
        check(rv_ctx_set_option(ctx()->raw(), "top_k_select_from_rows", keys.size() == 2 ? 1 : 0));
        for (size_t k : {size_t{1}, size_t{50}, size_t{299}, size_t{400}}) {
            auto stream = StreamingPhysicalPlan::top_k(StreamingPhysicalPlan::memory_source(batches_of(df, 2)), keys, k, 3)->execute();
            CHECK(stream->schema()->num_fields() == kNames.size() && stream->schema()->field(3).name() == "s");
            auto got = stream->collect();
            CHECK(got.size() == 1 && *got[0].schema() == *stream->schema() && !stream->next_batch());
            CHECK(dynamic_cast<GpuTopKStream *>(stream.get())->folds() == 75);  // two batches of two rows reach three rows: 150 batches, 75 folds
            const size_t rows = std::min(k, r.size());
            CHECK(got[0].num_rows() == rows && cells(got[0].columns(), 0, rows) == table_of(r, first_rows(r, keys, k)));
        }
    }
    check(rv_ctx_set_option(ctx()->raw(), "top_k_select_from_rows", 0));
    // batches of uneven sizes, the last fold a partial one; the default fold size takes everything in one
    const std::vector<SortKey> keys = {{"k", false, false}};
    auto uneven = StreamingPhysicalPlan::top_k(StreamingPhysicalPlan::memory_source(batches_of(df, 7)), keys, 20, 3)->collect_batches();
    CHECK(uneven.size() == 1 && cells(uneven[0].columns(), 0, 20) == table_of(r, first_rows(r, keys, 20)));
    auto stream = StreamingPhysicalPlan::top_k(StreamingPhysicalPlan::memory_source(batches_of(df, 7)), keys, 20)->execute();
    auto whole = stream->collect();
    CHECK(whole.size() == 1 && dynamic_cast<GpuTopKStream *>(stream.get())->folds() == 1);
    CHECK(cells(whole[0].columns(), 0, 20) == table_of(r, first_rows(r, keys, 20)));
}

GPU_TEST(k_zero_and_inputs_without_rows_give_one_zero_row_batch_with_the_schema) {
    const Rows r = make_rows(200), none = make_rows(0);
    const std::vector<SortKey> keys = {{"k", false, false}};
    auto check_empty = [&](const std::vector<RecordBatch> &got) {
        CHECK(got.size() == 1 && got[0].num_rows() == 0 && got[0].num_columns() == kNames.size());
        CHECK(got[0].column(0)->data_type() == DataType::Int64 && got[0].column(2)->data_type() == DataType::Float64 &&
              got[0].column(3)->data_type() == DataType::String && got[0].column(4)->data_type() == DataType::Boolean && got[0].column(4)->len() == 0);
    };
    check_empty(StreamingPhysicalPlan::top_k(StreamingPhysicalPlan::memory_source(batches_of(frame_of(r), 16)), keys, 0, 3)->collect_batches());
    check_empty(StreamingPhysicalPlan::top_k(StreamingPhysicalPlan::dataframe_source(frame_of(r), 64), keys, 0)->collect_batches());
    check_empty(StreamingPhysicalPlan::top_k(StreamingPhysicalPlan::dataframe_source(frame_of(none), 1024), keys, 5)->collect_batches());
    DeviceFrame eager = PhysicalPlan::top_k(PhysicalPlan::source(frame_of(none)), keys, 5)->execute();
    CHECK(eager.height() == 0 && eager.names == kNames && eager.columns[4]->data_type() == DataType::Boolean);
    DeviceFrame zero = PhysicalPlan::top_k(PhysicalPlan::source(frame_of(r)), keys, 0)->execute();
    CHECK(zero.height() == 0 && zero.names == kNames && zero.columns[3]->data_type() == DataType::String);
    // a filter that keeps nothing: whatever batches it yields, top_k yields one without rows
    auto filtered = StreamingPhysicalPlan::gpu_filter_project(StreamingPhysicalPlan::memory_source(batches_of(frame_of(r), 64)), lower_predicate(Expr::col("v").gt(Expr::lit(5000))), kNames);
    check_empty(StreamingPhysicalPlan::top_k(filtered, keys, 5, 3)->collect_batches());
}

GPU_TEST(a_limit_on_top_of_it_and_a_filter_below_it) {
    const Rows r = make_rows(5000);
    const DeviceFrame df = frame_of(r);
    const std::vector<SortKey> keys = {{"v", true, false}, {"k", false, false}};
    Rows kept;
    for (size_t i = 0; i < r.size(); ++i)
        if (r.v[i] < 900) {
            kept.k.push_back(r.k[i]);
            kept.v.push_back(r.v[i]);
            kept.f.push_back(r.f[i]);
            kept.s.push_back(r.s[i]);
            kept.b.push_back(r.b[i]);
        }
    auto filtered = StreamingPhysicalPlan::gpu_filter_project(StreamingPhysicalPlan::memory_source(batches_of(df, 1024)), lower_predicate(Expr::col("v").lt(Expr::lit(900))), kNames);
    auto got = StreamingPhysicalPlan::limit(StreamingPhysicalPlan::top_k(filtered, keys, 10, 2000), 3)->collect_batches();
    size_t total = 0;
    for (auto &b : got) total += b.num_rows();
    CHECK(total == 3 && got.size() == 1);
    CHECK(cells(got[0].columns(), 0, 3) == table_of(kept, first_rows(kept, keys, 3)));
    // the planner's arm: Limit(Sort(x)) and top_k(x) say the same
    auto sorted = StreamingPhysicalPlan::limit(StreamingPhysicalPlan::sort(StreamingPhysicalPlan::memory_source(batches_of(df, 1024)), keys), 10)->collect_batches();
    auto best = StreamingPhysicalPlan::top_k(StreamingPhysicalPlan::memory_source(batches_of(df, 1024)), keys, 10)->collect_batches();
    CHECK(sorted.size() == 1 && best.size() == 1 && cells(sorted[0].columns(), 0, 10) == cells(best[0].columns(), 0, 10));
}
