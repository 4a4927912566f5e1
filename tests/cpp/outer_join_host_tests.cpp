// Tests of the join types of the C++ host layer (rivulus_amd/host/rivulus_host.hpp): JoinType { Inner, Left, Right, Outer, Semi, Anti }
// through the eager PhysicalPlan::hash_join and, all but Outer, through StreamingPhysicalPlan::hash_join -> GpuHashJoinStream.
//   outer_join_host_tests --cpu   cases without a device
//   outer_join_host_tests         every case (needs an MI355X)
// Output: "ok <name>" / "FAIL <name>: why"; exit status 0 iff all pass.
#include "host_test_main.hpp"
#include "join_test_cells.hpp"

using namespace rivulus;
using namespace rivulus::execution;
using namespace rivulus::physical_plan;

namespace {
using Names = std::vector<std::string>;
using Col = std::vector<std::string>;
SchemaRef schema_of(std::vector<Field> f) { return std::make_shared<const Schema>(std::move(f)); }
const JoinType kAllTypes[] = {JoinType::Inner, JoinType::Left, JoinType::Right, JoinType::Outer, JoinType::Semi, JoinType::Anti};
const JoinType kStreamedTypes[] = {JoinType::Inner, JoinType::Left, JoinType::Right, JoinType::Semi, JoinType::Anti};

// left: ids 1, 2, 2, null; right: ids 2, null, 1, 9.  Both frames have a column "amount".
DeviceFrame left_frame() {
    DeviceFrame f;
    f.names = {"id", "amount", "tag"};
    f.columns = {Int64Array::create(ctx(), {1, 2, 2, 0}, std::vector<bool>{true, true, true, false}),
                 Float64Array::create(ctx(), {0.5, -0.0, 2.5, 0.0}, std::vector<bool>{true, true, true, false}),
                 StringArray::create(ctx(), {"a", std::nullopt, "c", "d"})};
    return f;
}
DeviceFrame right_frame() {
    DeviceFrame f;
    f.names = {"amount", "id"};
    f.columns = {Float64Array::from_values(ctx(), {1.0, 2.0, 3.0, 4.0}), Int64Array::create(ctx(), {2, 0, 1, 9}, std::vector<bool>{true, false, true, true})};
    return f;
}
DeviceFrame eager(const DeviceFrame &l, const DeviceFrame &r, const std::string &lk, const std::string &rk, JoinType t) {
    return PhysicalPlan::hash_join(PhysicalPlan::source(l), PhysicalPlan::source(r), lk, rk, t)->execute();
}
Table table_of(const DeviceFrame &f) { return cells(f.columns, 0, f.height()); }
std::vector<RecordBatch> batches_of(const DeviceFrame &f, size_t batch) {
    std::vector<Field> fields;
    for (size_t c = 0; c < f.names.size(); ++c) fields.push_back(Field{f.names[c], f.columns[c]->data_type(), true});
    auto schema = schema_of(fields);
    std::vector<RecordBatch> out;
    for (size_t lo = 0; lo < f.height(); lo += batch) {
        std::vector<ArrayRef> c;
        for (auto &col : f.columns) c.push_back(col->slice(lo, std::min(batch, f.height() - lo)));
        out.push_back(RecordBatch::try_new(schema, c));
    }
    return out;
}
DeviceFrame rows_of(const DeviceFrame &f, size_t lo, size_t len) {
    DeviceFrame o;
    o.names = f.names;
    for (auto &c : f.columns) o.columns.push_back(c->slice(lo, len));
    return o;
}
}  // namespace

// ---- without a device ---------------------------------------------------------------------------------------------------------------
CPU_TEST(join_shape_of_every_type) {
    CHECK(join_shape(JoinType::Inner).kind == RV_JOIN_INNER && !join_shape(JoinType::Inner).swapped);
    CHECK(join_shape(JoinType::Right).kind == RV_JOIN_PROBE_OUTER && !join_shape(JoinType::Right).swapped);
    CHECK(join_shape(JoinType::Outer).kind == RV_JOIN_FULL_OUTER && !join_shape(JoinType::Outer).swapped);
    CHECK(join_shape(JoinType::Left).kind == RV_JOIN_PROBE_OUTER && join_shape(JoinType::Left).swapped);
    CHECK(join_shape(JoinType::Semi).kind == RV_JOIN_PROBE_SEMI && join_shape(JoinType::Semi).swapped);
    CHECK(join_shape(JoinType::Anti).kind == RV_JOIN_PROBE_ANTI && join_shape(JoinType::Anti).swapped);
}

CPU_TEST(default_argument_is_inner_and_the_left_plan_is_the_build_side) {
    DeviceFrame empty;
    auto l = PhysicalPlan::source(empty), r = PhysicalPlan::source(empty);
    auto plan = PhysicalPlan::hash_join(l, r, "a", "b");
    CHECK(plan->join_kind == RV_JOIN_INNER && plan->build_side == l && plan->input == r && plan->build_key == "a" && plan->probe_key == "b");
    auto right = PhysicalPlan::hash_join(l, r, "a", "b", JoinType::Right);
    CHECK(right->join_kind == RV_JOIN_PROBE_OUTER && right->build_side == l && right->probe_key == "b");
    auto outer = PhysicalPlan::hash_join(l, r, "a", "b", JoinType::Outer);
    CHECK(outer->join_kind == RV_JOIN_FULL_OUTER && outer->build_side == l);
    for (JoinType t : {JoinType::Left, JoinType::Semi, JoinType::Anti}) {  // the left frame probes a table built on the right frame
        auto swapped = PhysicalPlan::hash_join(l, r, "a", "b", t);
        CHECK(swapped->build_side == r && swapped->input == l && swapped->build_key == "b" && swapped->probe_key == "a");
    }
    auto sl = StreamingPhysicalPlan::dataframe_source(empty, 4), sr = StreamingPhysicalPlan::dataframe_source(empty, 4);
    auto splan = StreamingPhysicalPlan::hash_join(sl, sr, "a", "b");
    CHECK(splan->join_kind == RV_JOIN_INNER && splan->build_side == sl && splan->input == sr);
    auto sleft = StreamingPhysicalPlan::hash_join(sl, sr, "a", "b", JoinType::Left);
    CHECK(sleft->join_kind == RV_JOIN_PROBE_OUTER && sleft->build_side == sr && sleft->input == sl && sleft->probe_key == "a");
}

CPU_TEST(outer_in_a_streaming_plan_is_unsupported_and_names_the_eager_plan) {
    DeviceFrame empty;
    auto l = StreamingPhysicalPlan::dataframe_source(empty, 4), r = StreamingPhysicalPlan::dataframe_source(empty, 4);
    const std::string what = thrown<Error>([&] { StreamingPhysicalPlan::hash_join(l, r, "a", "b", JoinType::Outer); });
    CHECK(what.find("JoinType::Outer is not streamed") != std::string::npos);
    CHECK(what.find("PhysicalPlan::hash_join") != std::string::npos && what.find("eager plan") != std::string::npos);
    try {
        StreamingPhysicalPlan::hash_join(l, r, "a", "b", JoinType::Outer);
        CHECK(false);
    } catch (const Error &e) {
        CHECK(e.status == RV_ERR_UNSUPPORTED);
    }
    // the stream itself refuses the kind as well
    auto s = schema_of({Field{"k", DataType::Int64, true}});
    JoinSide b, p;
    b.stream = MemoryStream::empty(s);
    p.stream = MemoryStream::empty(s);
    const std::string direct = thrown<Error>([&] { GpuHashJoinStream(std::move(b), std::move(p), "k", "k", 1024, 1024, RV_JOIN_FULL_OUTER); });
    CHECK(direct.find("eager plan") != std::string::npos);
}

CPU_TEST(output_fields_of_every_kind) {
    auto build = schema_of({Field{"k", DataType::Int64, false}, Field{"v", DataType::Float64, false}, Field{"w", DataType::String, true}});
    auto probe = schema_of({Field{"v", DataType::String, false}, Field{"k", DataType::Int64, false}});
    auto names = [](const std::vector<Field> &f) {
        Names n;
        for (auto &x : f) n.push_back(x.name());
        return n;
    };
    CHECK((names(join_output_fields(*probe, *build, 0)) == Names{"v", "k", "v_right", "w"}));
    CHECK((names(join_output_fields(*probe, *build, 0, RV_JOIN_INNER)) == Names{"v", "k", "v_right", "w"}));
    auto outer = join_output_fields(*probe, *build, 0, RV_JOIN_PROBE_OUTER);
    CHECK((names(outer) == Names{"v", "k", "v_right", "w"}));
    CHECK(!outer[0].is_nullable() && outer[2].is_nullable() && outer[2].data_type() == DataType::Float64);  // the build side can lack a partner
    auto full = join_output_fields(*probe, *build, 0, RV_JOIN_FULL_OUTER);
    CHECK((names(full) == Names{"v", "k", "k_right", "v_right", "w"}));  // the build key stays, at its place
    CHECK(full[0].is_nullable() && full[2].is_nullable() && full[2].data_type() == DataType::Int64);
    CHECK((names(join_output_fields(*probe, *build, 0, RV_JOIN_PROBE_SEMI)) == Names{"v", "k"}));
    CHECK((names(join_output_fields(*probe, *build, 0, RV_JOIN_PROBE_ANTI)) == Names{"v", "k"}));
    auto other = schema_of({Field{"id", DataType::Int64, false}});
    CHECK((names(join_output_fields(*other, *build, 0, RV_JOIN_FULL_OUTER)) == Names{"id", "k", "v", "w"}));  // no clash, no suffix
    // a stream of a probe-preserving kind has that kind's schema
    JoinSide b, p;
    b.stream = MemoryStream::empty(build);
    p.stream = MemoryStream::empty(probe);
    GpuHashJoinStream semi(std::move(b), std::move(p), "k", "k", 1024, 1024, RV_JOIN_PROBE_SEMI);
    CHECK(semi.schema()->num_fields() == 2 && semi.schema()->field(1).name() == "k");
    CHECK(!semi.next_batch());
}

// ---- the eager plan -------------------------------------------------------------------------------------------------------------------
GPU_TEST(inner_with_and_without_the_argument) {
    const DeviceFrame l = left_frame(), r = right_frame();
    DeviceFrame a = PhysicalPlan::hash_join(PhysicalPlan::source(l), PhysicalPlan::source(r), "id", "id")->execute();
    DeviceFrame b = eager(l, r, "id", "id", JoinType::Inner);
    CHECK((a.names == Names{"amount", "id", "amount_right", "tag"}) && a.names == b.names);
    CHECK(table_of(a) == table_of(b));
    CHECK((table_of(a) == Table{Col{"1", "1", "2", "3"}, Col{"2", "2", "null", "1"}, Col{"-0", "2.5", "null", "0.5"}, Col{"null", "'c'", "'d'", "'a'"}}));
}

GPU_TEST(right_keeps_every_row_of_the_right_frame) {  // the left frame is the build side: PROBE_OUTER
    DeviceFrame out = eager(left_frame(), right_frame(), "id", "id", JoinType::Right);
    CHECK((out.names == Names{"amount", "id", "amount_right", "tag"}));
    CHECK((table_of(out) == Table{Col{"1", "1", "2", "3", "4"}, Col{"2", "2", "null", "1", "9"}, Col{"-0", "2.5", "null", "0.5", "null"},
                                  Col{"null", "'c'", "'d'", "'a'", "null"}}));
}

GPU_TEST(outer_keeps_both_sides_and_the_build_key) {
    DeviceFrame l = left_frame();
    l.columns[0] = Int64Array::create(ctx(), {1, 2, 2, 7}, std::vector<bool>{true, true, true, true});  // 7 meets nothing
    DeviceFrame out = eager(l, right_frame(), "id", "id", JoinType::Outer);
    CHECK((out.names == Names{"amount", "id", "id_right", "amount_right", "tag"}));
    // right rows in order (id 2 -> left 1, 2; null -> nothing; 1 -> left 0; 9 -> nothing), then the unmatched left row 3
    CHECK((table_of(out) == Table{Col{"1", "1", "2", "3", "4", "null"}, Col{"2", "2", "null", "1", "9", "null"}, Col{"2", "2", "null", "1", "null", "7"},
                                  Col{"-0", "2.5", "null", "0.5", "null", "null"}, Col{"null", "'c'", "null", "'a'", "null", "'d'"}}));
}

GPU_TEST(left_puts_the_left_frame_first) {  // swapped: the left frame probes, PROBE_OUTER
    DeviceFrame out = eager(left_frame(), right_frame(), "id", "id", JoinType::Left);
    CHECK((out.names == Names{"id", "amount", "tag", "amount_right"}));
    // left rows in order: 1 -> right 2; 2 -> right 0; 2 -> right 0; null -> right 1
    CHECK((table_of(out) == Table{Col{"1", "2", "2", "null"}, Col{"0.5", "-0", "2.5", "null"}, Col{"'a'", "null", "'c'", "'d'"}, Col{"3", "1", "1", "2"}}));
    DeviceFrame r = right_frame();
    r.columns[1] = Int64Array::from_values(ctx(), {5, 5, 1, 5});
    out = eager(left_frame(), r, "id", "id", JoinType::Left);
    CHECK((table_of(out) == Table{Col{"1", "2", "2", "null"}, Col{"0.5", "-0", "2.5", "null"}, Col{"'a'", "null", "'c'", "'d'"}, Col{"3", "null", "null", "null"}}));
}

GPU_TEST(semi_and_anti_keep_the_left_frame_s_columns_only) {
    DeviceFrame r = right_frame();
    r.columns[1] = Int64Array::from_values(ctx(), {2, 2, 5, 9});  // id 2 twice: a semi join still yields a left row once
    DeviceFrame semi = eager(left_frame(), r, "id", "id", JoinType::Semi), anti = eager(left_frame(), r, "id", "id", JoinType::Anti);
    CHECK((semi.names == Names{"id", "amount", "tag"}) && semi.names == anti.names);
    CHECK((table_of(semi) == Table{Col{"2", "2"}, Col{"-0", "2.5"}, Col{"null", "'c'"}}));
    CHECK((table_of(anti) == Table{Col{"1", "null"}, Col{"0.5", "null"}, Col{"'a'", "'d'"}}));  // a null key without a null partner is kept
    // with a null on the right the null left row has a partner: not SQL's NOT IN
    anti = eager(left_frame(), right_frame(), "id", "id", JoinType::Anti);
    CHECK(anti.height() == 0 && anti.width() == 3 && anti.columns[2]->data_type() == DataType::String);
}

GPU_TEST(empty_sides_give_the_right_names_and_dtypes) {
    const DeviceFrame l = left_frame(), r = right_frame(), l0 = rows_of(l, 0, 0), r0 = rows_of(r, 0, 0);
    for (JoinType t : kAllTypes) {
        const DeviceFrame both = eager(l0, r0, "id", "id", t);
        CHECK(both.height() == 0);
        const DeviceFrame full = eager(l, r, "id", "id", t);
        CHECK(both.names == full.names);
        for (size_t c = 0; c < both.width(); ++c) CHECK(both.columns[c]->data_type() == full.columns[c]->data_type());
    }
    CHECK(eager(l, r0, "id", "id", JoinType::Left).height() == 4 && eager(l, r0, "id", "id", JoinType::Right).height() == 0);
    CHECK(eager(l, r0, "id", "id", JoinType::Outer).height() == 4 && eager(l0, r, "id", "id", JoinType::Outer).height() == 4);
    CHECK(eager(l, r0, "id", "id", JoinType::Anti).height() == 4 && eager(l, r0, "id", "id", JoinType::Semi).height() == 0);
}

// ---- String keys ----------------------------------------------------------------------------------------------------------------------
GPU_TEST(string_keys_outer_returns_the_strings_not_their_ids) {
    DeviceFrame l, r;
    l.names = {"name", "n"};
    l.columns = {StringArray::create(ctx(), {"ann", "bob", std::nullopt, "cy"}), Int64Array::from_values(ctx(), {1, 2, 3, 4})};
    r.names = {"m", "name"};
    r.columns = {Int64Array::from_values(ctx(), {10, 20, 30}), StringArray::create(ctx(), {"bob", "dan", "ann"})};
    DeviceFrame out = eager(l, r, "name", "name", JoinType::Outer);
    CHECK((out.names == Names{"m", "name", "name_right", "n"}));
    CHECK(out.columns[2]->data_type() == DataType::String);
    CHECK((table_of(out) == Table{Col{"10", "20", "30", "null", "null"}, Col{"'bob'", "'dan'", "'ann'", "null", "null"},
                                  Col{"'bob'", "null", "'ann'", "null", "'cy'"}, Col{"2", "null", "1", "3", "4"}}));
    // a String key against an Int64 key: only nulls meet; the build key still comes back as strings
    DeviceFrame ri;
    ri.names = {"name"};
    ri.columns = {Int64Array::create(ctx(), {7, 0}, std::vector<bool>{true, false})};
    out = eager(l, ri, "name", "name", JoinType::Outer);
    CHECK((out.names == Names{"name", "name_right", "n"}));
    CHECK((table_of(out) == Table{Col{"7", "null", "null", "null", "null"}, Col{"null", "null", "'ann'", "'bob'", "'cy'"}, Col{"null", "3", "1", "2", "4"}}));
    // the other types over String keys
    CHECK((table_of(eager(l, r, "name", "name", JoinType::Left)) ==
           Table{Col{"'ann'", "'bob'", "null", "'cy'"}, Col{"1", "2", "3", "4"}, Col{"30", "10", "null", "null"}}));
    CHECK((table_of(eager(l, r, "name", "name", JoinType::Right)) == Table{Col{"10", "20", "30"}, Col{"'bob'", "'dan'", "'ann'"}, Col{"2", "null", "1"}}));
    CHECK((table_of(eager(l, r, "name", "name", JoinType::Semi)) == Table{Col{"'ann'", "'bob'"}, Col{"1", "2"}}));
    CHECK((table_of(eager(l, r, "name", "name", JoinType::Anti)) == Table{Col{"null", "'cy'"}, Col{"3", "4"}}));
}

// ---- the streaming plan -----------------------------------------------------------------------------------------------------------------
// one output batch per batch of the streamed side, empty ones included, each the eager join of that batch alone
GPU_TEST(streamed_types_batch_by_batch) {
    const size_t nl = 2500, nr = 3100, batch = 1024;
    std::vector<int64_t> lk(nl), lv(nl), rk(nr), rv(nr);
    std::vector<bool> lvalid(nl), rvalid(nr);
    uint64_t x = 777;
    auto rnd = [&] { return x = x * 6364136223846793005ull + 1442695040888963407ull, x >> 33; };
    for (size_t i = 0; i < nl; ++i) lk[i] = static_cast<int64_t>(rnd() % 700), lv[i] = static_cast<int64_t>(rnd() % 1000), lvalid[i] = rnd() % 9 != 0;
    for (size_t i = 0; i < nr; ++i) rk[i] = static_cast<int64_t>(rnd() % 900), rv[i] = static_cast<int64_t>(rnd() % 1000), rvalid[i] = rnd() % 9 != 0;
    DeviceFrame l, r;
    l.names = {"k", "x"};
    l.columns = {Int64Array::create(ctx(), lk, lvalid), Int64Array::from_values(ctx(), lv)};
    r.names = {"x", "k", "s"};
    std::vector<std::optional<std::string>> rs(nr);
    for (size_t i = 0; i < nr; ++i) rs[i] = i % 11 ? std::optional<std::string>("r" + std::to_string(i)) : std::nullopt;
    r.columns = {Int64Array::from_values(ctx(), rv), Int64Array::create(ctx(), rk, rvalid), StringArray::create(ctx(), rs)};
    for (JoinType t : kStreamedTypes) {
        const bool swapped = join_shape(t).swapped;
        const DeviceFrame &streamed = swapped ? l : r;
        auto plan = StreamingPhysicalPlan::hash_join(StreamingPhysicalPlan::memory_source(batches_of(l, batch)),
                                                     StreamingPhysicalPlan::memory_source(batches_of(r, batch)), "k", "k", t);
        auto got = plan->execute()->collect();
        const size_t nb = (streamed.height() + batch - 1) / batch;
        CHECK(got.size() == nb);
        for (size_t b = 0; b < nb; ++b) {
            const size_t lo = b * batch, len = std::min(batch, streamed.height() - lo);
            const DeviceFrame want = swapped ? eager(rows_of(l, lo, len), r, "k", "k", t) : eager(l, rows_of(r, lo, len), "k", "k", t);
            CHECK(got[b].num_columns() == want.width() && got[b].num_rows() == want.height());
            for (size_t c = 0; c < want.width(); ++c) CHECK(got[b].schema()->field(c).name() == want.names[c]);
            CHECK(cells(got[b].columns(), 0, got[b].num_rows()) == table_of(want));
        }
    }
}

GPU_TEST(streamed_types_over_a_resident_frame_and_string_keys) {
    DeviceFrame l, r;  // no nulls: a DataFrameSource fills them
    l.names = {"name", "n"};
    l.columns = {StringArray::from_strings(ctx(), {"ann", "bob", "cy", "bob", "eve"}), Int64Array::from_values(ctx(), {1, 2, 3, 4, 5})};
    r.names = {"m", "name"};
    r.columns = {Int64Array::from_values(ctx(), {10, 20, 30}), StringArray::from_strings(ctx(), {"bob", "dan", "ann"})};
    for (JoinType t : kStreamedTypes) {
        auto plan = StreamingPhysicalPlan::hash_join(StreamingPhysicalPlan::dataframe_source(l, 2), StreamingPhysicalPlan::dataframe_source(r, 2), "name", "name", t);
        auto got = plan->execute()->collect();
        CHECK(got.size() == (join_shape(t).swapped ? 3u : 2u));  // one batch per batch of the streamed side, empty ones included
        const DeviceFrame want = eager(l, r, "name", "name", t);
        RecordBatch all = RecordBatch::concat(got);
        CHECK(all.num_rows() == want.height() && all.num_columns() == want.width());
        for (size_t c = 0; c < want.width(); ++c) CHECK(all.schema()->field(c).name() == want.names[c]);
        CHECK(cells(all.columns(), 0, all.num_rows()) == table_of(want));
    }
}
