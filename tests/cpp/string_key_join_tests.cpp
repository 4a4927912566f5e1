// Tests of String join keys in the C++ host layer (rivulus_amd/host/rivulus_host.hpp): PhysicalPlan::hash_join and
// StreamingPhysicalPlan::hash_join / GpuHashJoinStream over the device string dictionary, against a model of the reference's
// join (plan.rs:174-284) written out here: a map from key to build rows, probe rows in order.
//   string_key_join_tests --cpu   cases without a device
//   string_key_join_tests         every case (needs an MI355X)
// Output: "ok <name>" / "FAIL <name>: why"; exit status 0 iff all pass.
#include <map>

#include "host_test_main.hpp"
#include "join_test_cells.hpp"

using namespace rivulus;
using namespace rivulus::execution;
using namespace rivulus::physical_plan;

namespace {
using Strs = std::vector<std::optional<std::string>>;
using Pairs = std::vector<std::pair<size_t, size_t>>;  // (probe row, build row)
SchemaRef schema_of(std::vector<Field> f) { return std::make_shared<const Schema>(std::move(f)); }

// The reference's result_pairs (plan.rs:183-204) for two key columns read back from the device: AnyValue keys -- a cell's dtype and
// value, null == null, values of different dtypes never equal -- probe rows in order, build rows ascending within a probe row.
Pairs model_pairs(const ArrayRef &build, const ArrayRef &probe) {
    auto key = [](const ArrayRef &a, size_t i) {
        const std::string c = cell(a, i);
        return c == "null" ? c : std::to_string(static_cast<int>(a->data_type())) + ":" + c;
    };
    std::map<std::string, std::vector<size_t>> table;
    for (size_t r = 0; r < build->len(); ++r) table[key(build, r)].push_back(r);
    Pairs pairs;
    for (size_t p = 0; p < probe->len(); ++p) {
        auto it = table.find(key(probe, p));
        if (it == table.end()) continue;
        for (size_t r : it->second) pairs.emplace_back(p, r);
    }
    return pairs;
}

// materialize_join_result (plan.rs:212-255) over `pairs`: names and cells of every probe column, then every build column but the key
struct Expected {
    std::vector<std::string> names;
    std::vector<DataType> types;
    Table table;
    std::vector<size_t> nulls;
};
Expected materialize(const DeviceFrame &b, const DeviceFrame &p, const std::string &bk, const Pairs &pairs) {
    Expected e;
    auto add = [&](const std::string &name, const ArrayRef &col, bool probe_side) {
        e.names.push_back(name);
        e.types.push_back(col->data_type());
        e.table.emplace_back();
        e.nulls.push_back(0);
        std::vector<std::string> all;
        for (size_t i = 0; i < col->len(); ++i) all.push_back(cell(col, i));
        for (auto &pr : pairs) {
            e.table.back().push_back(all[probe_side ? pr.first : pr.second]);
            e.nulls.back() += e.table.back().back() == "null";
        }
    };
    for (size_t i = 0; i < p.width(); ++i) add(p.names[i], p.columns[i], true);
    for (size_t i = 0; i < b.width(); ++i)
        if (b.names[i] != bk) add(p.column(b.names[i]) ? b.names[i] + "_right" : b.names[i], b.columns[i], false);
    return e;
}
void check_columns(const std::vector<std::string> &names, const std::vector<ArrayRef> &cols, size_t rows, const Expected &e) {
    CHECK(names == e.names);
    CHECK(cols.size() == e.names.size());
    for (size_t j = 0; j < cols.size(); ++j) {
        CHECK(cols[j]->len() == rows);
        CHECK(cols[j]->data_type() == e.types[j]);
        CHECK(cols[j]->null_count() == e.nulls[j]);
    }
    CHECK(rows == (e.table.empty() ? 0 : e.table[0].size()));
    CHECK(cells(cols, 0, rows) == e.table);
}
// the eager join of b and p against the model; returns the frame
DeviceFrame check_eager(const DeviceFrame &b, const DeviceFrame &p, const std::string &bk, const std::string &pk, size_t *npairs = nullptr) {
    DeviceFrame got = PhysicalPlan::hash_join(PhysicalPlan::source(b), PhysicalPlan::source(p), bk, pk)->execute();
    const Pairs pairs = model_pairs(*b.column(bk), *p.column(pk));
    check_columns(got.names, got.columns, got.height(), materialize(b, p, bk, pairs));
    if (npairs) *npairs = pairs.size();
    return got;
}
std::vector<std::string> names_of(const SchemaRef &s) {
    std::vector<std::string> n;
    for (auto &f : s->fields()) n.push_back(f.name());
    return n;
}

// deterministic test data: n keys out of `distinct` names, one in `null_every` null
uint64_t g_seed = 2024;
uint64_t rnd() { return g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull, g_seed >> 33; }
Strs random_keys(size_t n, size_t distinct, size_t null_every) {
    Strs v(n);
    for (auto &x : v) {
        const uint64_t k = rnd() % distinct;
        if (rnd() % null_every != 0) x = "name-" + std::to_string(k) + std::string(k % 19, '#');
    }
    return v;
}
std::vector<int64_t> iota64(size_t n, int64_t from) {
    std::vector<int64_t> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = from + static_cast<int64_t>(i);
    return v;
}
DeviceFrame slice_frame(const DeviceFrame &f, size_t lo, size_t len) {
    DeviceFrame s;
    s.names = f.names;
    for (auto &c : f.columns) s.columns.push_back(c->slice(lo, len));
    return s;
}
JoinSide resident(const DeviceFrame &f, size_t batch = 0) {
    JoinSide s;
    s.names = f.names;
    s.columns = f.columns;
    s.batch_size = batch;
    return s;
}
// build (3000 rows, duplicate and null keys, a String payload and a name the probe side has too) and probe (`np` rows)
void big_frames(size_t np, DeviceFrame &b, DeviceFrame &p) {
    const size_t nb = 3000;
    std::vector<bool> valid(nb);
    for (size_t i = 0; i < nb; ++i) valid[i] = rnd() % 5 != 0;
    b.names = {"v", "name", "note"};
    b.columns = {Int64Array::create(ctx(), iota64(nb, 100000), valid), StringArray::create(ctx(), random_keys(nb, 2500, 40)),
                 StringArray::create(ctx(), random_keys(nb, 50, 6))};
    p.names = {"name", "v"};
    p.columns = {StringArray::create(ctx(), random_keys(np, 3500, 50)), Int64Array::from_values(ctx(), iota64(np, 0))};
}
}  // namespace

// ---- without a device ---------------------------------------------------------------------------------------------------------
CPU_TEST(which_keys_go_through_the_dictionary) {
    CHECK(!StringKeyEncoder(DataType::Int64, DataType::Int64).active());
    CHECK(!StringKeyEncoder(DataType::Float64, DataType::Boolean).active());
    CHECK(!StringKeyEncoder(DataType::Null, DataType::Int64).active());
    StringKeyEncoder both(DataType::String, DataType::String), build_only(DataType::String, DataType::Int64), probe_only(DataType::Float64, DataType::String);
    CHECK(both.active() && both.probe_helper());
    CHECK(build_only.active() && !build_only.probe_helper());
    CHECK(probe_only.active() && probe_only.probe_helper());
}

CPU_TEST(output_schema_keeps_the_string_probe_key) {
    auto bs = schema_of({Field{"id", DataType::Int64, true}, Field{"name", DataType::String, true}, Field{"city", DataType::String, false}});
    auto ps = schema_of({Field{"id", DataType::Int64, true}, Field{"name", DataType::String, true}, Field{"amount", DataType::Float64, true}});
    JoinSide b, p;
    b.stream = MemoryStream::empty(bs);
    p.stream = MemoryStream::empty(ps);
    GpuHashJoinStream s(std::move(b), std::move(p), "name", "name");
    auto o = s.schema();
    CHECK((names_of(o) == std::vector<std::string>{"id", "name", "amount", "id_right", "city"}));
    CHECK(o->field(1).data_type() == DataType::String);  // the probe key as it is: no helper column in the schema
    CHECK(o->field(3).data_type() == DataType::Int64 && o->field(4).data_type() == DataType::String && !o->field(4).is_nullable());
    CHECK(!s.next_batch());  // an empty probe stream: no batch, no device work
}

CPU_TEST(missing_string_key_column_error_text) {
    auto bs = schema_of({Field{"name", DataType::String, true}});
    auto ps = schema_of({Field{"label", DataType::String, true}});
    JoinSide b, p;
    b.stream = MemoryStream::empty(bs);
    p.stream = MemoryStream::empty(ps);
    std::string m = thrown<StreamError>([&] { GpuHashJoinStream(std::move(b), std::move(p), "name", "name"); });
    CHECK(m == "Stream execution error: Column 'name' not found in schema");
}

CPU_TEST(helper_column_leaves_the_null_counts) {  // [batches][ncols] row-major -> [batches][ncols - 1]
    std::vector<int64_t> none;
    drop_count_column(none, 0, 4, 2);
    CHECK(none.empty());
    std::vector<int64_t> padded = {7, 8, 9};  // room for one batch, none taken
    drop_count_column(padded, 0, 3, 1);
    CHECK(padded.empty());
    std::vector<int64_t> one = {5, 6, 7};
    drop_count_column(one, 1, 3, 0);
    CHECK((one == std::vector<int64_t>{6, 7}));
    std::vector<int64_t> three = {10, 11, 12, 13, 20, 21, 22, 23, 30, 31, 32, 33};
    drop_count_column(three, 3, 4, 2);
    CHECK((three == std::vector<int64_t>{10, 11, 13, 20, 21, 23, 30, 31, 33}));
    std::vector<int64_t> last = {10, 11, 12, 20, 21, 22};
    drop_count_column(last, 2, 3, 2);
    CHECK((last == std::vector<int64_t>{10, 11, 20, 21}));
    std::vector<int64_t> only = {4, 5};  // the helper as the only column
    drop_count_column(only, 2, 1, 0);
    CHECK(only.empty());
}

CPU_TEST(helper_column_is_appended_as_the_key) {
    const rv_dcolumn *a = reinterpret_cast<const rv_dcolumn *>(0x10), *b = reinterpret_cast<const rv_dcolumn *>(0x20);  // never dereferenced
    ProbeColumns plain = with_key_helper({a, b}, 1, nullptr);
    CHECK(plain.cols.size() == 2 && plain.key == 1 && !plain.helper_at);
    std::vector<ArrayRef> out(3);
    std::vector<int64_t> nulls = {1, 2, 3};
    without_key_helper(plain, out, &nulls, 1);  // no helper: nothing leaves
    CHECK(out.size() == 3 && nulls.size() == 3);
}

CPU_TEST(join_output_fields_follow_materialize_join_result) {
    const Schema probe({Field{"id", DataType::Int64, false}, Field{"name", DataType::String, true}});
    const Schema build({Field{"name", DataType::String, true}, Field{"id", DataType::Float64, false}, Field{"city", DataType::String, false},
                        Field{"note", DataType::Boolean, true}});
    const std::vector<Field> f = join_output_fields(probe, build, 1);  // keyed on the build side's `id`
    CHECK((f == std::vector<Field>{Field{"id", DataType::Int64, false}, Field{"name", DataType::String, true}, Field{"name_right", DataType::String, true},
                                   Field{"city", DataType::String, false}, Field{"note", DataType::Boolean, true}}));
    // the key is left out by its index, not its name: keyed on `name`, the build side's `id` clashes and stays
    const std::vector<Field> g = join_output_fields(probe, build, 0);
    CHECK(g.size() == 5 && g[2] == (Field{"id_right", DataType::Float64, false}) && g[3].name() == "city" && !g[3].is_nullable());
    CHECK(join_output_fields(Schema::empty(), build, 3).size() == 3);
}

// ---- on the device: the eager join -----------------------------------------------------------------------------------------------
GPU_TEST(users_orders_joined_on_name) {  // tests/golden/join_users_orders.json, re-keyed on `name` instead of `user_id`
    DeviceFrame users, orders;
    users.names = {"user_id", "name", "city"};
    users.columns = {Int64Array::from_values(ctx(), {1, 2, 3, 4}), StringArray::from_strings(ctx(), {"Alice", "Bob", "Charlie", "Diana"}),
                     StringArray::from_strings(ctx(), {"NYC", "LA", "Chicago", "Boston"})};
    orders.names = {"order_id", "name", "amount"};
    orders.columns = {Int64Array::from_values(ctx(), {101, 102, 103, 104, 105}), StringArray::from_strings(ctx(), {"Alice", "Bob", "Alice", "Charlie", "Nobody"}),
                      Float64Array::from_values(ctx(), {25.99, 15.5, 99.99, 45.0, 12.99})};
    DeviceFrame got = check_eager(users, orders, "name", "name");
    CHECK((got.names == std::vector<std::string>{"order_id", "name", "amount", "user_id", "city"}));
    CHECK(got.columns[1]->data_type() == DataType::String);  // the probe key comes back as the String column it was
    CHECK((cells(got.columns, 0, got.height()) == Table{{"101", "102", "103", "104"},
                                                        {"'Alice'", "'Bob'", "'Alice'", "'Charlie'"},
                                                        {f17(25.99), f17(15.5), f17(99.99), f17(45.0)},
                                                        {"1", "2", "1", "3"},
                                                        {"'NYC'", "'LA'", "'NYC'", "'Chicago'"}}));
    // the same frames with the key names differing and a name clash: `_right` on the build column
    users.names = {"amount", "who", "city"};
    got = check_eager(users, orders, "who", "name");
    CHECK((got.names == std::vector<std::string>{"order_id", "name", "amount", "amount_right", "city"}));
}

GPU_TEST(eager_shapes) {
    DeviceFrame b, p;
    // duplicate build keys, a null key on both sides, "" as a value, a String payload on both sides, a clashing name
    b.names = {"k", "pay", "s"};
    b.columns = {StringArray::create(ctx(), {"x", std::nullopt, "y", "x", "", std::nullopt, std::string("x\0z", 3)}),
                 Int64Array::create(ctx(), {1, 2, 3, 4, 5, 6, 7}, std::vector<bool>{true, true, false, true, true, true, true}),
                 StringArray::create(ctx(), {"s0", "s1", std::nullopt, "s3", "s4", "s5", "s6"})};
    p.names = {"s", "k"};
    p.columns = {StringArray::create(ctx(), {"p0", std::nullopt, "p2", "p3", "p4", "p5"}), StringArray::create(ctx(), {"x", std::nullopt, "", "absent", "y", "x"})};
    size_t npairs = 0;
    DeviceFrame got = check_eager(b, p, "k", "k", &npairs);
    CHECK(npairs == 2 + 2 + 1 + 0 + 1 + 2);  // "x\0z" is not "x"
    CHECK((got.names == std::vector<std::string>{"s", "k", "pay", "s_right"}));
    // zero pairs: zero-row columns of the same dtypes
    DeviceFrame q;
    q.names = {"k", "f"};
    q.columns = {StringArray::from_strings(ctx(), {"none", "of", "these"}), Float64Array::from_values(ctx(), {1.5, 2.5, 3.5})};
    got = check_eager(b, q, "k", "k", &npairs);
    CHECK(npairs == 0 && got.height() == 0 && got.width() == 4);
    CHECK(got.columns[0]->data_type() == DataType::String && got.columns[1]->data_type() == DataType::Float64 && got.columns[3]->data_type() == DataType::String);
    // an empty build side, an empty probe side
    DeviceFrame eb = slice_frame(b, 0, 0), ep = slice_frame(p, 0, 0);
    got = check_eager(eb, p, "k", "k");
    CHECK(got.height() == 0 && got.width() == 4);
    got = check_eager(b, ep, "k", "k");
    CHECK(got.height() == 0 && got.width() == 4);
    got = check_eager(eb, ep, "k", "k");
    CHECK(got.height() == 0 && got.width() == 4);
    // sliced frames: keys at offsets that are no multiple of 8
    check_eager(slice_frame(b, 1, 5), slice_frame(p, 1, 4), "k", "k");
}

GPU_TEST(eager_mixed_keys_meet_null_to_null_only) {
    DeviceFrame s, i, f;
    s.names = {"k", "sv"};
    s.columns = {StringArray::create(ctx(), {"0", std::nullopt, "-1", "1", std::nullopt, "2"}), Int64Array::from_values(ctx(), {10, 11, 12, 13, 14, 15})};
    i.names = {"k", "iv"};
    i.columns = {Int64Array::create(ctx(), {0, -1, 7, 1, 2, 3}, std::vector<bool>{true, true, false, true, false, true}), Int64Array::from_values(ctx(), {20, 21, 22, 23, 24, 25})};
    f.names = {"k", "fv"};
    f.columns = {Float64Array::create(ctx(), {0.0, -1.0, 0.5, 1.0}, std::vector<bool>{true, false, true, true}), Int64Array::from_values(ctx(), {30, 31, 32, 33})};
    size_t npairs = 0;
    DeviceFrame got = check_eager(s, i, "k", "k", &npairs);  // String on the build side, Int64 probe
    CHECK(npairs == 2 * 2);
    CHECK(got.columns[0]->data_type() == DataType::Int64);
    got = check_eager(i, s, "k", "k", &npairs);  // Int64 build, String on the probe side
    CHECK(npairs == 2 * 2);
    CHECK(got.columns[0]->data_type() == DataType::String && got.width() == 3);
    check_eager(s, f, "k", "k", &npairs);  // String against Float64, either way round
    CHECK(npairs == 2 * 1);
    check_eager(f, s, "k", "k", &npairs);
    CHECK(npairs == 2 * 1);
    // no nulls on the String side: nothing meets
    DeviceFrame t;
    t.names = {"k"};
    t.columns = {StringArray::from_strings(ctx(), {"0", "1"})};
    check_eager(t, i, "k", "k", &npairs);
    CHECK(npairs == 0);
    check_eager(i, t, "k", "k", &npairs);
    CHECK(npairs == 0);
}

GPU_TEST(eager_join_of_thousands_of_rows) {
    DeviceFrame b, p;
    big_frames(5000, b, p);
    size_t npairs = 0;
    check_eager(b, p, "name", "name", &npairs);
    CHECK(npairs > 3000);
}

// ---- on the device: the streaming join ---------------------------------------------------------------------------------------------
GPU_TEST(stream_resident_probe_in_windows) {  // 4 x 1024 rows + a ragged batch of 904; small windows, a small pair budget
    DeviceFrame b, p;
    big_frames(5000, b, p);
    const DeviceFrame eager = check_eager(b, p, "name", "name");
    for (auto [window, budget] : {std::pair<size_t, uint64_t>{size_t(1) << 28, uint64_t(1) << 28}, {2048, uint64_t(1) << 28}, {size_t(1) << 28, 777}}) {
        GpuHashJoinStream s(resident(b), resident(p, 1024), "name", "name", window, budget);
        auto got = s.collect();
        CHECK(got.size() == 5);
        for (size_t k = 0; k < got.size(); ++k) {  // batch k == the eager join of the whole build side against probe batch k
            const DeviceFrame pk = slice_frame(p, k * 1024, std::min<size_t>(1024, 5000 - k * 1024));
            const Pairs pairs = model_pairs(*b.column("name"), *pk.column("name"));
            check_columns(names_of(got[k].schema()), got[k].columns(), got[k].num_rows(), materialize(b, pk, "name", pairs));
            for (size_t j = 0; j < got[k].num_columns(); ++j)
                if (got[k].column(j)->data_type() != DataType::Null) CHECK(got[k].column(j)->has_null_bitmap() == (got[k].column(j)->null_count() > 0));
        }
        RecordBatch all = RecordBatch::concat(got);
        CHECK(all.num_rows() == eager.height());
        CHECK(cells(all.columns(), 0, all.num_rows()) == cells(eager.columns, 0, eager.height()));
        CHECK(s.rows_scanned() == 5000);
    }
}

GPU_TEST(stream_pulled_batches_one_output_each) {  // a MemoryStream of separate batches, empty ones included
    DeviceFrame b, p;
    big_frames(2500, b, p);
    auto ps = schema_of({Field{"name", DataType::String, true}, Field{"v", DataType::Int64, true}});
    std::vector<std::pair<size_t, size_t>> cuts = {{0, 700}, {700, 0}, {700, 1}, {701, 1024}, {1725, 775}, {2500, 0}};
    std::vector<RecordBatch> batches;
    for (auto [lo, len] : cuts) batches.push_back(RecordBatch::try_new(ps, slice_frame(p, lo, len).columns));
    JoinSide probe;
    probe.stream = std::make_unique<MemoryStream>(ps, batches);
    GpuHashJoinStream s(resident(b), std::move(probe), "name", "name");
    auto got = s.collect();
    CHECK(got.size() == cuts.size());
    size_t total = 0;
    for (size_t k = 0; k < cuts.size(); ++k) {
        const DeviceFrame pk = slice_frame(p, cuts[k].first, cuts[k].second);
        const Pairs pairs = model_pairs(*b.column("name"), *pk.column("name"));
        check_columns(names_of(got[k].schema()), got[k].columns(), got[k].num_rows(), materialize(b, pk, "name", pairs));  // null counts included
        total += pairs.size();
    }
    CHECK(got[1].num_rows() == 0 && got[5].num_rows() == 0 && got[1].num_columns() == 4);
    CHECK(total > 1000);
    // through the plans, a String key on the build STREAM as well
    std::vector<RecordBatch> bb;
    auto bs = schema_of({Field{"v", DataType::Int64, true}, Field{"name", DataType::String, true}, Field{"note", DataType::String, true}});
    for (size_t lo = 0; lo < 3000; lo += 1300) bb.push_back(RecordBatch::try_new(bs, slice_frame(b, lo, std::min<size_t>(1300, 3000 - lo)).columns));
    auto plan = StreamingPhysicalPlan::hash_join(StreamingPhysicalPlan::memory_source(bb), StreamingPhysicalPlan::memory_source(batches), "name", "name");
    auto again = plan->execute()->collect();
    CHECK(again.size() == got.size());
    for (size_t k = 0; k < got.size(); ++k) CHECK(cells(again[k].columns(), 0, again[k].num_rows()) == cells(got[k].columns(), 0, got[k].num_rows()));
}

GPU_TEST(stream_mixed_keys_meet_null_to_null_only) {
    DeviceFrame s, i;
    s.names = {"k", "sv"};
    s.columns = {StringArray::create(ctx(), {"0", std::nullopt, "-1", "1", std::nullopt, "2", "3"}), Int64Array::from_values(ctx(), {10, 11, 12, 13, 14, 15, 16})};
    i.names = {"k", "iv"};
    i.columns = {Int64Array::create(ctx(), {0, -1, 7, 1, 2}, std::vector<bool>{true, true, false, true, false}), Int64Array::from_values(ctx(), {20, 21, 22, 23, 24})};
    for (int string_builds = 0; string_builds < 2; ++string_builds) {
        const DeviceFrame &b = string_builds ? s : i, &p = string_builds ? i : s;
        GpuHashJoinStream js(resident(b), resident(p, 3), "k", "k");
        auto got = js.collect();
        CHECK(got.size() == (p.height() + 2) / 3);
        for (size_t k = 0; k < got.size(); ++k) {
            const DeviceFrame pk = slice_frame(p, k * 3, std::min<size_t>(3, p.height() - k * 3));
            check_columns(names_of(got[k].schema()), got[k].columns(), got[k].num_rows(), materialize(b, pk, "k", model_pairs(*b.column("k"), *pk.column("k"))));
        }
        CHECK(RecordBatch::concat(got).num_rows() == 4);
    }
}

GPU_TEST(stream_under_a_limit_is_the_first_pairs) {
    DeviceFrame b, p;
    big_frames(5000, b, p);
    const DeviceFrame eager = check_eager(b, p, "name", "name");
    CHECK(eager.height() > 10);
    auto js = std::make_unique<GpuHashJoinStream>(resident(b), resident(p, 1024), "name", "name");
    LimitStream lim(std::move(js), 10);
    auto got = lim.collect();
    RecordBatch all = RecordBatch::concat(got);
    CHECK(all.num_rows() == 10);
    CHECK(cells(all.columns(), 0, 10) == cells(eager.columns, 0, 10));
}
