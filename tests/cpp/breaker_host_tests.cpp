// What the pipeline breakers of the host layer (rivulus_amd/host/rivulus_host.hpp) share: GpuGroupByStream (both key forms), GpuSortStream,
// GpuTopKStream and GpuWindowStream drain their input the same way, whatever batches it arrives in, and say the same as the eager
// PhysicalPlan.  Run by tests/test_breaker_host.py; the scaffold is host_test_main.hpp.
#include <optional>

#include "host_test_main.hpp"
#include "join_test_cells.hpp"

using namespace rivulus;
using namespace rivulus::execution;
using namespace rivulus::expressions;
using namespace rivulus::physical_plan;

namespace {

using Keys = std::vector<std::string>;
const Keys kNames = {"k", "v", "s"};
const std::vector<AggSpec> kAggs = {{AggOp::Sum, "v", "total"}, {AggOp::CountRows, "", "rows"}, {AggOp::Count, "s", "n_s"}};
const std::vector<SortKey> kSortKeys = {{"k", true, false}};  // k == 3 three times: the ties stay in input order
const std::vector<SortKey> kWindowOrder = {{"v", false, false}};  // no ties inside a partition
const std::vector<WindowExpr> kWindowExprs = {{WindowOp::Sum, "v", 0, "run"}, {WindowOp::RowNumber, "", 0, "rn"}};  // the default frame is the running one

Schema kvs_schema() { return Schema({Field{"k", DataType::Int64, true}, Field{"v", DataType::Float64, true}, Field{"s", DataType::String, true}}); }

// a stream with a schema that yields no batch at all
struct NoBatches : DataStream {
    SchemaRef schema() const override { return std::make_shared<const Schema>(kvs_schema()); }
    std::optional<RecordBatch> next_batch() override { return std::nullopt; }
};
JoinSide no_batches() {
    JoinSide s;
    s.stream = std::make_unique<NoBatches>();
    return s;
}
// a column without a device handle: only its dtype and length are known
struct OffDevice : Array {
    OffDevice(DataType t, size_t n) : type(t), rows(n) {}
    DataType data_type() const override { return type; }
    size_t len() const override { return rows; }
    DataType type;
    size_t rows;
};

// the five operators, streamed over `in` and eager over `in`
const char *const kOps[] = {"group_by", "group_by_keys", "sort", "top_k", "window"};
StreamingPlanPtr streamed(size_t op, StreamingPlanPtr in) {
    switch (op) {
        case 0: return StreamingPhysicalPlan::group_by(std::move(in), "k", kAggs);
        case 1: return StreamingPhysicalPlan::group_by(std::move(in), Keys{"s", "k"}, kAggs);
        case 2: return StreamingPhysicalPlan::sort(std::move(in), kSortKeys);
        case 3: return StreamingPhysicalPlan::top_k(std::move(in), kSortKeys, 3, 2);
        default: return StreamingPhysicalPlan::window(std::move(in), {"s"}, kWindowOrder, kWindowExprs);
    }
}
PhysicalPlanPtr eager(size_t op, PhysicalPlanPtr in) {
    switch (op) {
        case 0: return PhysicalPlan::group_by(std::move(in), "k", kAggs);
        case 1: return PhysicalPlan::group_by(std::move(in), Keys{"s", "k"}, kAggs);
        case 2: return PhysicalPlan::sort(std::move(in), kSortKeys);
        case 3: return PhysicalPlan::top_k(std::move(in), kSortKeys, 3);
        default: return PhysicalPlan::window(std::move(in), {"s"}, kWindowOrder, kWindowExprs);
    }
}

// 7 rows: k repeats, v in quarters (every sum is exact) with one null, s with one null and one ""
DeviceFrame seven_rows() {
    DeviceFrame df;
    df.names = kNames;
    df.columns = {Int64Array::from_values(ctx(), {3, 1, 3, 2, 1, 3, 2}),
                  Float64Array::create(ctx(), {0.5, 1.25, -2.0, 4.0, 8.0, -0.25, 1.0}, std::vector<bool>{true, true, true, false, true, true, true}),
                  StringArray::create(ctx(), {"a", std::nullopt, "b", "a", "", "b", "a"})};
    return df;
}
DeviceFrame filled(const DeviceFrame &df) {  // the null fill of dataframe_to_batches
    DeviceFrame out;
    out.names = df.names;
    for (auto &c : df.columns) {
        rv_dcolumn *f = nullptr;
        check(rv_fill_nulls(c->context()->raw(), c->handle(), &f));
        out.columns.push_back(Array::adopt(c->context(), f));
    }
    return out;
}
// the rows of `df` as batches of the given sizes; 0 is a zero-row batch
std::vector<RecordBatch> batches_of(const DeviceFrame &df, const std::vector<size_t> &sizes) {
    auto schema = std::make_shared<Schema>(frame_schema(df));
    std::vector<RecordBatch> out;
    size_t lo = 0;
    for (size_t n : sizes) {
        if (n == 0) {
            out.push_back(RecordBatch::empty(ctx(), schema));
            continue;
        }
        std::vector<ArrayRef> cols;
        for (auto &c : df.columns) cols.push_back(c->slice(lo, n));
        out.push_back(RecordBatch::try_new(schema, std::move(cols)));
        lo += n;
    }
    return out;
}
// the one batch a breaker emits: names and cells
struct Result {
    Keys names;
    Table table;
    bool operator==(const Result &o) const { return names == o.names && table == o.table; }
};
Result the_one_batch(const StreamingPlanPtr &plan) {
    auto stream = plan->execute();
    auto got = stream->collect();
    CHECK(got.size() == 1 && *got[0].schema() == *stream->schema() && !stream->next_batch());
    Result r;
    for (auto &f : got[0].schema()->fields()) r.names.push_back(f.name());
    r.table = cells(got[0].columns(), 0, got[0].num_rows());
    return r;
}

}  // namespace

// ---- no device ----------------------------------------------------------------------------------------------------------------------
CPU_TEST(no_batch_and_no_context_is_an_execution_error_and_then_the_stream_is_done) {
    auto check_stream_says = [](DataStream &s, const std::string &op) {
        bool threw = false;
        try {
            s.next_batch();
        } catch (const StreamError &e) {
            threw = true;
            CHECK(e.kind == StreamError::Execution);
            CHECK(e.message == op + ": the input yielded no batch and the plan holds no device context");
        }
        CHECK(threw);
        CHECK(!s.next_batch());
    };
    GpuGroupByStream one(no_batches(), std::string("k"), kAggs, nullptr);
    check_stream_says(one, "group_by");
    GpuGroupByStream list(no_batches(), Keys{"s", "k"}, kAggs, nullptr);
    check_stream_says(list, "group_by");
    GpuSortStream sort(no_batches(), kSortKeys, nullptr);
    check_stream_says(sort, "sort");
    GpuWindowStream window(no_batches(), {"s"}, kWindowOrder, kWindowExprs, nullptr);
    check_stream_says(window, "window");
    GpuTopKStream top_k(no_batches(), kSortKeys, 3, nullptr, 2);
    check_stream_says(top_k, "top_k");
    CHECK(top_k.folds() == 0);
}

CPU_TEST(a_bad_key_is_refused_by_the_constructor_with_the_schema_functions_text) {
    CHECK(thrown<GroupByPlanError>([] { GpuGroupByStream(no_batches(), std::string("zz"), kAggs, nullptr); }) == "group_by: unknown key column 'zz'");
    CHECK(thrown<GroupByPlanError>([] { GpuGroupByStream(no_batches(), std::string("v"), kAggs, nullptr); }) ==
          "group_by: key column 'v' is Float64; only Int64 and String keys are grouped");
    CHECK(thrown<GroupByPlanError>([] { GpuGroupByStream(no_batches(), Keys{"k", "k"}, kAggs, nullptr); }) == "group_by: key column 'k' is named twice");
    CHECK(thrown<GroupByPlanError>([] { GpuGroupByStream(no_batches(), Keys{"v"}, kAggs, nullptr); }).empty());  // the list takes a Float64 key
    CHECK(thrown<SortPlanError>([] { GpuSortStream(no_batches(), {{"s", false, false}}, nullptr); }) ==
          "sort: key column 's' is String; only Int64 and Float64 keys are sorted");
    CHECK(thrown<SortPlanError>([] { GpuTopKStream(no_batches(), {{"zz", false, false}}, 3, nullptr); }) == "sort: unknown key column 'zz'");
    CHECK(thrown<WindowPlanError>([] { GpuWindowStream(no_batches(), {"zz"}, {}, kWindowExprs, nullptr); }) == "window: unknown partition column 'zz'");
    CHECK(thrown<WindowPlanError>([] { GpuWindowStream(no_batches(), {}, {{"s", false, false}}, kWindowExprs, nullptr); }) ==
          "window: order column 's' is String; only Int64 and Float64 keys are sorted");
}

CPU_TEST(a_resident_side_and_a_frame_have_the_same_schema_every_field_nullable) {
    const std::vector<ArrayRef> columns = {std::make_shared<const OffDevice>(DataType::Int64, 4), std::make_shared<const OffDevice>(DataType::Float64, 4),
                                           std::make_shared<const OffDevice>(DataType::String, 4), std::make_shared<const OffDevice>(DataType::Boolean, 4)};
    const Keys names = {"k", "v", "s", "b"};
    const JoinSide side{nullptr, names, columns, 2};
    const Schema of_frame = frame_schema(DeviceFrame{names, columns});
    const SchemaRef of_side = side.schema();
    CHECK(*of_side == of_frame && of_frame.num_fields() == 4);
    for (size_t c = 0; c < 4; ++c) {
        const Field &f = of_side->field(c);
        CHECK(f.name() == names[c] && f.data_type() == columns[c]->data_type() && f.is_nullable());
    }
    CHECK(*JoinSide{}.schema() == frame_schema(DeviceFrame{}) && JoinSide{}.schema()->is_empty());
}

// ---- on the device ------------------------------------------------------------------------------------------------------------------
// (a) a DataFrameSource cut into batches of 3, (b) a MemorySource of one batch, (c) a MemorySource of 3 + 0 + 3 + 1 rows, (d) the eager plan
// over the frame after the streams' null fill: one batch each, the same cells, validity included
GPU_TEST(every_breaker_says_the_same_over_a_frame_one_batch_several_batches_and_eagerly) {
    const DeviceFrame df = seven_rows(), fdf = filled(df);
    for (size_t op = 0; op < 5; ++op) {
        const Result a = the_one_batch(streamed(op, StreamingPhysicalPlan::dataframe_source(df, 3)));
        const Result b = the_one_batch(streamed(op, StreamingPhysicalPlan::memory_source(batches_of(fdf, {7}))));
        const Result c = the_one_batch(streamed(op, StreamingPhysicalPlan::memory_source(batches_of(fdf, {3, 0, 3, 1}))));
        const DeviceFrame e = eager(op, PhysicalPlan::source(fdf))->execute();
        const Result d{e.names, cells(e.columns, 0, e.height())};
        if (!(a == d && b == d && c == d)) throw Fail(std::string("the four results of ") + kOps[op] + " differ");
        CHECK(!d.table.empty() && !d.table[0].empty());
    }
    // what they say, once: the groups in first-row order (the null of v was filled with 0.0), the ties of k == 3 in input order
    const DeviceFrame g = eager(0, PhysicalPlan::source(fdf))->execute();
    CHECK((cells(g.columns, 0, g.height()) == Table{{"3", "1", "2"}, {f17(-1.75), f17(9.25), f17(1.0)}, {"3", "2", "2"}, {"3", "1", "2"}}));
    const DeviceFrame t = eager(3, PhysicalPlan::source(fdf))->execute();
    CHECK((cells(t.columns, 0, t.height()) == Table{{"3", "3", "3"}, {f17(0.5), f17(-2.0), f17(-0.25)}, {"'a'", "'b'", "'b'"}}));
    const DeviceFrame w = eager(4, PhysicalPlan::source(fdf))->execute();
    CHECK((w.names == Keys{"k", "v", "s", "run", "rn"}));
    CHECK((cells({w.columns[3], w.columns[4]}, 0, 7) == Table{{f17(0.5), f17(1.25), f17(-2.0), f17(0.0), f17(8.0), f17(-2.25), f17(1.5)}, {"2", "1", "1", "1", "1", "2", "3"}}));
}

// group_by reaches rv_hash_aggregate with zero rows; sort, top_k and window return before their device call
GPU_TEST(zero_row_batches_only_give_one_zero_row_batch_with_the_output_schema) {
    const DeviceFrame df = seven_rows();
    for (size_t op = 0; op < 5; ++op) {
        auto stream = streamed(op, StreamingPhysicalPlan::memory_source(batches_of(df, {0, 0})))->execute();
        auto got = stream->collect();
        CHECK(got.size() == 1 && got[0].num_rows() == 0 && *got[0].schema() == *stream->schema() && !stream->next_batch());
        CHECK(got[0].num_columns() == stream->schema()->num_fields());
        for (size_t c = 0; c < got[0].num_columns(); ++c) CHECK(got[0].column(c)->len() == 0 && got[0].column(c)->data_type() == stream->schema()->field(c).data_type());
    }
    CHECK(streamed(1, StreamingPhysicalPlan::memory_source(batches_of(df, {0})))->execute()->schema()->num_fields() == 5);
    CHECK(streamed(4, StreamingPhysicalPlan::memory_source(batches_of(df, {0})))->execute()->schema()->num_fields() == 5);
}

GPU_TEST(a_column_off_the_device_is_refused_with_the_filters_text_and_the_other_arms_text) {
    DeviceFrame df;
    df.names = {"k", "s"};
    df.columns = {Int64Array::from_values(ctx(), {1, 2, 3}), std::make_shared<const OffDevice>(DataType::String, 3)};
    DeviceFrame ok;
    ok.names = {"k"};
    ok.columns = {df.columns[0]};
    auto why = [](const PhysicalPlanPtr &plan) { return thrown<Error>([&] { plan->execute(); }); };
    auto src = PhysicalPlan::source(df);
    CHECK(why(PhysicalPlan::filter(src, CompareTerm{"k", RV_GT, Literal(int64_t{1})})) == "String columns are outside the device path");
    const std::string others = "columns off the device are outside the device path";
    CHECK(why(PhysicalPlan::computed_filter(src, Expr::col("k").add(Expr::lit(1)).gt(Expr::lit(2)))) == others);
    CHECK(why(PhysicalPlan::hash_join(src, PhysicalPlan::source(ok), "k", "k")) == others);
    CHECK(why(PhysicalPlan::hash_join(PhysicalPlan::source(ok), src, "k", "k")) == others);
    CHECK(why(PhysicalPlan::group_by(src, "k", {{AggOp::Count, "s", "n"}})) == others);
    CHECK(why(PhysicalPlan::group_by(src, Keys{"k"}, {{AggOp::Count, "s", "n"}})) == others);
    CHECK(why(PhysicalPlan::sort(src, kSortKeys)) == others);
    CHECK(why(PhysicalPlan::top_k(src, kSortKeys, 2)) == others);
    CHECK(why(PhysicalPlan::window(src, {}, kSortKeys, {{WindowOp::RowNumber, "", 0, "rn"}})) == others);
    // the context stays usable
    DeviceFrame kept = PhysicalPlan::filter(PhysicalPlan::source(ok), CompareTerm{"k", RV_GT, Literal(int64_t{1})})->execute();
    CHECK((cells(kept.columns, 0, kept.height()) == Table{{"2", "3"}}));
}
