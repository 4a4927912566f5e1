// Tests of the streaming inner join of the C++ host layer (StreamingPhysicalPlan::HashJoin -> GpuHashJoinStream,
// rivulus_amd/host/rivulus_host.hpp) against the eager PhysicalPlan::HashJoin, batch by batch.
//   stream_join_host_tests --cpu [fixture_dir]   cases without a device
//   stream_join_host_tests [fixture_dir]         every case (needs an MI355X)
// fixture_dir holds users.csv / orders.csv / expected.csv, written by tests/test_stream_join_host.py from
// tests/golden/join_users_orders.json.  Output: "ok <name>" / "FAIL <name>: why"; exit status 0 iff all pass.
#include "host_test_main.hpp"
#include "join_test_cells.hpp"

using namespace rivulus;
using namespace rivulus::execution;
using namespace rivulus::physical_plan;

namespace {
DeviceFrame frame_of(const std::vector<RecordBatch> &batches, SchemaRef schema) {
    DeviceFrame f;
    for (auto &fld : schema->fields()) f.names.push_back(fld.name());
    f.columns = (batches.size() == 1 ? batches[0] : RecordBatch::concat(batches)).columns();
    return f;
}
SchemaRef schema_of(std::vector<Field> f) { return std::make_shared<const Schema>(std::move(f)); }
SchemaRef users_schema() {
    return schema_of({Field{"user_id", DataType::Int64, true}, Field{"name", DataType::String, true}, Field{"city", DataType::String, true}});
}
SchemaRef orders_schema() {
    return schema_of({Field{"order_id", DataType::Int64, true}, Field{"user_id", DataType::Int64, true}, Field{"amount", DataType::Float64, true}});
}
StreamingPlanPtr csv(const std::string &file, SchemaRef s, size_t batch) {
    return StreamingPhysicalPlan::csv_file_source(ctx(), g_arg + "/" + file, std::move(s), batch);
}
DeviceFrame csv_frame(const std::string &file, SchemaRef s) { return frame_of(csv(file, s, 1024)->collect_batches(), s); }

// a frame as a DataFrameSource hands it on: dataframe_to_batches' null fill
DeviceFrame filled(const DeviceFrame &f) {
    DeviceFrame o;
    o.names = f.names;
    for (auto &c : f.columns) {
        rv_dcolumn *h = nullptr;
        check(rv_fill_nulls(ctx()->raw(), c->handle(), &h));
        o.columns.push_back(Array::adopt(ctx(), h));
    }
    return o;
}

// Every output batch b of `plan` equals the eager join of the build frame against probe batch b alone (the probe frame's rows
// [starts[b], starts[b + 1])), dtypes, names and null counts included; returns the concatenated output.
std::vector<RecordBatch> check_per_batch(const StreamingPlanPtr &plan, const DeviceFrame &build, const DeviceFrame &probe, size_t batch,
                                         const std::string &bk, const std::string &pk) {
    auto stream = plan->execute();
    auto got = stream->collect();
    const size_t n = probe.height(), nb = (n + batch - 1) / batch;
    CHECK(got.size() == nb);
    for (size_t b = 0; b < nb; ++b) {
        DeviceFrame slice;
        slice.names = probe.names;
        const size_t lo = b * batch, len = std::min(batch, n - lo);
        for (auto &c : probe.columns) slice.columns.push_back(c->slice(lo, len));
        DeviceFrame want = PhysicalPlan::hash_join(PhysicalPlan::source(build), PhysicalPlan::source(slice), bk, pk)->execute();
        CHECK(got[b].num_columns() == want.width());
        CHECK(got[b].num_rows() == want.height());
        for (size_t j = 0; j < want.width(); ++j) {
            CHECK(got[b].schema()->field(j).name() == want.names[j]);
            CHECK(got[b].column(j)->data_type() == want.columns[j]->data_type());
            CHECK(got[b].column(j)->null_count() == want.columns[j]->null_count());
            if (want.columns[j]->data_type() != DataType::Null) CHECK(got[b].column(j)->has_null_bitmap() == (got[b].column(j)->null_count() > 0));
        }
        CHECK(cells(got[b].columns(), 0, got[b].num_rows()) == cells(want.columns, 0, want.height()));
    }
    return got;
}
}  // namespace

// ---- without a device ---------------------------------------------------------------------------------------------------------
CPU_TEST(missing_key_column_is_a_stream_execution_error) {  // FilterStream's wording (stream.rs:146-148)
    auto s = schema_of({Field{"a", DataType::Int64, true}});
    auto t = schema_of({Field{"k", DataType::Int64, true}});
    JoinSide b, p;
    b.stream = MemoryStream::empty(s);
    p.stream = MemoryStream::empty(t);
    std::string m = thrown<StreamError>([&] { GpuHashJoinStream(std::move(b), std::move(p), "k", "k"); });
    CHECK(m == "Stream execution error: Column 'k' not found in schema");
    JoinSide b2, p2;
    b2.stream = MemoryStream::empty(t);
    p2.stream = MemoryStream::empty(s);
    m = thrown<StreamError>([&] { GpuHashJoinStream(std::move(b2), std::move(p2), "k", "z"); });
    CHECK(m == "Stream execution error: Column 'z' not found in schema");
    // through the plan: an empty DataFrameSource streams with an empty schema (streaming.rs:85-94), so the key is not there
    DeviceFrame empty;
    auto plan = StreamingPhysicalPlan::hash_join(StreamingPhysicalPlan::dataframe_source(empty, 1024), StreamingPhysicalPlan::dataframe_source(empty, 1024), "k", "k");
    m = thrown<StreamingExecutionError>([&] { plan->execute(); });
    CHECK(m == "Stream error: Stream execution error: Column 'k' not found in schema");
}

CPU_TEST(output_schema_names_and_right_suffix) {
    auto bs = schema_of({Field{"k", DataType::Int64, true}, Field{"v", DataType::Float64, false}, Field{"w", DataType::String, true}});
    auto ps = schema_of({Field{"v", DataType::String, true}, Field{"k", DataType::Int64, true}});
    JoinSide b, p;
    b.stream = MemoryStream::empty(bs);
    p.stream = MemoryStream::empty(ps);
    GpuHashJoinStream s(std::move(b), std::move(p), "k", "k");
    auto o = s.schema();
    CHECK(o->num_fields() == 4);
    CHECK(o->field(0).name() == "v" && o->field(1).name() == "k" && o->field(2).name() == "v_right" && o->field(3).name() == "w");
    CHECK(o->field(2).data_type() == DataType::Float64 && !o->field(2).is_nullable());
    CHECK(!s.next_batch());  // an empty probe stream: no batch, no device work
}

// ---- on the device -------------------------------------------------------------------------------------------------------------
GPU_TEST(users_orders_through_every_probe_source) {  // tests/golden/join_users_orders.json
    const DeviceFrame users = csv_frame("users.csv", users_schema()), orders = csv_frame("orders.csv", orders_schema());
    auto out_schema = schema_of({Field{"order_id", DataType::Int64, true}, Field{"user_id", DataType::Int64, true}, Field{"amount", DataType::Float64, true},
                                 Field{"name", DataType::String, true}, Field{"city", DataType::String, true}});
    const DeviceFrame expected = csv_frame("expected.csv", out_schema);
    for (size_t batch : {size_t(1), size_t(2), size_t(1024)}) {
        std::vector<RecordBatch> ob;
        for (size_t lo = 0; lo < orders.height(); lo += batch) {
            std::vector<ArrayRef> c;
            for (auto &col : orders.columns) c.push_back(col->slice(lo, std::min(batch, orders.height() - lo)));
            ob.push_back(RecordBatch::try_new(orders_schema(), c));
        }
        const StreamingPlanPtr probes[] = {StreamingPhysicalPlan::dataframe_source(orders, batch), StreamingPhysicalPlan::memory_source(ob),
                                           csv("orders.csv", orders_schema(), batch)};
        for (auto &probe : probes) {
            auto plan = StreamingPhysicalPlan::hash_join(StreamingPhysicalPlan::dataframe_source(users, 1024), probe, "user_id", "user_id");
            auto got = check_per_batch(plan, users, orders, batch, "user_id", "user_id");
            RecordBatch all = RecordBatch::concat(got);
            CHECK(all.schema()->num_fields() == 5 && all.schema()->field(3).name() == "name");
            CHECK(cells(all.columns(), 0, all.num_rows()) == cells(expected.columns, 0, expected.height()));
        }
    }
}

GPU_TEST(names_with_right_and_nulls_per_batch) {
    DeviceFrame b, p;
    b.names = {"k", "v", "flag", "s"};
    b.columns = {Int64Array::from_values(ctx(), {1, 2, 3, 2}), Int64Array::create(ctx(), {10, 20, 30, 40}, std::vector<bool>{true, false, true, true}),
                 BooleanArray::create(ctx(), {true, std::nullopt, false, true}), StringArray::create(ctx(), {"a", std::nullopt, "c", "d"})};
    p.names = {"v", "k"};
    p.columns = {StringArray::create(ctx(), {"x", std::nullopt, "z", "w", "u", "t", "r"}), Int64Array::from_values(ctx(), {2, 9, 1, 3, 2, 2, 7})};
    for (size_t batch : {size_t(1), size_t(3), size_t(4)}) {
        auto plan = StreamingPhysicalPlan::hash_join(StreamingPhysicalPlan::dataframe_source(b, batch), StreamingPhysicalPlan::dataframe_source(p, batch), "k", "k");
        auto got = check_per_batch(plan, filled(b), filled(p), batch, "k", "k");  // both sides are DataFrameSources
        CHECK((got[0].schema()->field(2).name() == "v_right"));
    }
}

GPU_TEST(null_key_of_a_dataframe_source_is_filled_to_zero) {  // dataframe_to_batches' rv_fill_nulls: null Int64 -> 0, and 0 matches 0
    DeviceFrame b, p;
    b.names = {"k", "v"};
    b.columns = {Int64Array::from_values(ctx(), {0, 1}), Int64Array::from_values(ctx(), {100, 101})};
    p.names = {"k"};
    p.columns = {Int64Array::create(ctx(), {5, 1}, std::vector<bool>{false, true})};
    auto got = StreamingPhysicalPlan::hash_join(StreamingPhysicalPlan::dataframe_source(b, 1024), StreamingPhysicalPlan::dataframe_source(p, 1024), "k", "k")
                   ->execute()
                   ->collect();
    CHECK(got.size() == 1 && got[0].num_rows() == 2);
    CHECK((cells(got[0].columns(), 0, 2) == std::vector<std::vector<std::string>>{{"0", "1"}, {"100", "101"}}));
    // the eager join over the same frames keeps the null, which meets nothing here
    DeviceFrame eager = PhysicalPlan::hash_join(PhysicalPlan::source(b), PhysicalPlan::source(p), "k", "k")->execute();
    CHECK(eager.height() == 1);
}

GPU_TEST(empty_build_and_probe_streams) {
    DeviceFrame b, p;
    b.names = {"k", "s"};
    b.columns = {Int64Array::from_values(ctx(), {1, 2}), StringArray::from_strings(ctx(), {"a", "b"})};
    p.names = {"k", "f"};
    p.columns = {Int64Array::from_values(ctx(), {1, 2, 3, 1, 2}), Float64Array::from_values(ctx(), {0.5, 1.5, 2.5, 3.5, 4.5})};
    // a build stream that yields no batch: one zero-row batch per probe batch, with the join's schema
    JoinSide build, probe;
    build.stream = MemoryStream::empty(schema_of({Field{"k", DataType::Int64, true}, Field{"s", DataType::String, true}}));
    probe.names = p.names;
    probe.columns = p.columns;
    probe.batch_size = 2;
    GpuHashJoinStream s(std::move(build), std::move(probe), "k", "k");
    auto got = s.collect();
    CHECK(got.size() == 3);
    for (auto &g : got) {
        CHECK(g.num_rows() == 0 && g.num_columns() == 3);
        CHECK(g.column(2)->data_type() == DataType::String && g.schema()->field(2).name() == "s");
    }
    // an empty build frame (zero rows, its columns still typed): the same
    DeviceFrame eb;
    eb.names = b.names;
    eb.columns = {Int64Array::from_values(ctx(), {}), StringArray::from_strings(ctx(), {})};
    got = StreamingPhysicalPlan::hash_join(StreamingPhysicalPlan::dataframe_source(eb, 1024), StreamingPhysicalPlan::dataframe_source(p, 2), "k", "k")->execute()->collect();
    CHECK(got.size() == 3 && got[0].num_rows() == 0 && got[2].num_columns() == 3);
    // an empty probe stream: no batch at all
    JoinSide b2, p2;
    b2.names = b.names;
    b2.columns = b.columns;
    p2.stream = MemoryStream::empty(schema_of({Field{"k", DataType::Int64, true}}));
    GpuHashJoinStream s2(std::move(b2), std::move(p2), "k", "k");
    CHECK(s2.collect().empty());
}

GPU_TEST(limit_probes_a_small_window) {
    const size_t n = 1 << 20;
    std::vector<int64_t> keys(n), vals(n);
    for (size_t i = 0; i < n; ++i) keys[i] = static_cast<int64_t>(i % 1000), vals[i] = static_cast<int64_t>(i);
    DeviceFrame b, p;
    b.names = {"k", "bv"};
    std::vector<int64_t> bk(1000), bv(1000);
    for (size_t i = 0; i < 1000; ++i) bk[i] = static_cast<int64_t>(i), bv[i] = 7 * static_cast<int64_t>(i);
    b.columns = {Int64Array::from_values(ctx(), bk), Int64Array::from_values(ctx(), bv)};
    p.names = {"k", "pv"};
    p.columns = {Int64Array::from_values(ctx(), keys), Int64Array::from_values(ctx(), vals)};
    JoinSide build, probe;
    build.names = b.names;
    build.columns = b.columns;
    probe.names = p.names;
    probe.columns = p.columns;
    probe.batch_size = 1024;
    auto js = std::make_unique<GpuHashJoinStream>(std::move(build), std::move(probe), "k", "k");
    GpuHashJoinStream *raw = js.get();
    LimitStream lim(std::move(js), 10);
    auto got = lim.collect();
    size_t rows = 0;
    for (auto &g : got) rows += g.num_rows();
    CHECK(rows == 10);
    CHECK(raw->rows_scanned() > 0 && raw->rows_scanned() < n / 16);
    RecordBatch all = RecordBatch::concat(got);
    for (size_t i = 0; i < 10; ++i) {
        CHECK(cell(all.column(1), i) == std::to_string(i));          // pv: probe rows in order
        CHECK(cell(all.column(2), i) == std::to_string(7 * (i % 1000)));  // bv
    }
}

GPU_TEST(concatenation_equals_the_eager_join) {
    const size_t nb = 3000, np = 20000;
    std::vector<std::optional<int64_t>> bk(nb), pk(np);
    std::vector<int64_t> bval(nb), pval(np);
    std::vector<bool> pvalid(np), bvalid(nb);
    uint64_t x = 12345;
    auto rnd = [&] { return x = x * 6364136223846793005ull + 1442695040888963407ull, x >> 33; };
    for (size_t i = 0; i < nb; ++i) bk[i] = static_cast<int64_t>(rnd() % 900), bval[i] = static_cast<int64_t>(rnd()), bvalid[i] = rnd() % 5 != 0;
    for (size_t i = 0; i < np; ++i) pk[i] = static_cast<int64_t>(rnd() % 1200), pval[i] = static_cast<int64_t>(rnd()), pvalid[i] = rnd() % 7 != 0;
    DeviceFrame b, p;
    std::vector<int64_t> bkv(nb), pkv(np);
    for (size_t i = 0; i < nb; ++i) bkv[i] = *bk[i];
    for (size_t i = 0; i < np; ++i) pkv[i] = *pk[i];
    b.names = {"k", "x"};
    b.columns = {Int64Array::from_values(ctx(), bkv), Int64Array::create(ctx(), bval, bvalid)};
    p.names = {"x", "k"};
    p.columns = {Int64Array::create(ctx(), pval, pvalid), Int64Array::from_values(ctx(), pkv)};
    DeviceFrame eager = PhysicalPlan::hash_join(PhysicalPlan::source(b), PhysicalPlan::source(p), "k", "k")->execute();
    // default windows; small windows; a pair budget that cuts every window short
    for (auto [window, budget] : {std::pair<size_t, uint64_t>{size_t(1) << 28, uint64_t(1) << 28}, {5000, uint64_t(1) << 28}, {size_t(1) << 28, 777}}) {
        JoinSide build, probe;
        build.names = b.names;
        build.columns = b.columns;
        probe.names = p.names;
        probe.columns = p.columns;
        probe.batch_size = 1024;
        GpuHashJoinStream s(std::move(build), std::move(probe), "k", "k", window, budget);
        auto got = s.collect();
        CHECK(got.size() == (np + 1023) / 1024);
        RecordBatch all = RecordBatch::concat(got);
        CHECK(all.num_rows() == eager.height());
        CHECK(all.schema()->field(2).name() == "x_right");
        CHECK(cells(all.columns(), 0, all.num_rows()) == cells(eager.columns, 0, eager.height()));
        CHECK(s.rows_scanned() == np);
    }
}
