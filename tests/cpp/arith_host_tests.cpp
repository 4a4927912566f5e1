// Arithmetic select and filter expressions in the host layer (rivulus_amd/host/rivulus_host.hpp): lower_select_exprs,
// lower_computed_predicate, PhysicalPlan::project / computed_filter, StreamingPhysicalPlan::project / computed_filter_project.
// Run by tests/test_arith_host.py; the scaffold is host_test_main.hpp.
#include <cmath>
#include <optional>

#include "host_test_main.hpp"
#include "join_test_cells.hpp"

using namespace rivulus;
using namespace rivulus::execution;
using namespace rivulus::expressions;
using namespace rivulus::physical_plan;

namespace {

Expr col(const char *n) { return Expr::col(n); }
Expr flit(double v) { return Expr::lit(Literal(v)); }

Schema abc_schema() {
    return Schema({Field{"a", DataType::Int64, true}, Field{"b", DataType::Float64, true}, Field{"c", DataType::Boolean, true}});
}
ArithStep step_col(const char *n) { return ArithStep{RV_ARITH_COL, n, {}}; }
ArithStep step_lit(Literal v) { return ArithStep{RV_ARITH_LIT, "", std::move(v)}; }
ArithStep step_op(rv_arith_op op) { return ArithStep{op, "", {}}; }

// a: Int64 with nulls where `nulls`, b: Float64 without, over n rows
DeviceFrame ab_frame(size_t n, bool nulls) {
    std::vector<int64_t> a(n);
    std::vector<double> b(n);
    std::vector<bool> valid(n);
    for (size_t i = 0; i < n; ++i) {
        a[i] = static_cast<int64_t>((i * 7919) % 41) - 20;
        b[i] = static_cast<double>((i * 104729) % 1000) * 0.25 - 100.0;
        valid[i] = !nulls || i % 5 != 3;
    }
    DeviceFrame df;
    df.names = {"a", "b"};
    df.columns = {Int64Array::create(ctx(), a, nulls ? std::optional<std::vector<bool>>(valid) : std::nullopt), Float64Array::from_values(ctx(), b)};
    return df;
}
std::vector<RecordBatch> batches_of(const DeviceFrame &df, size_t batch) {  // zero-copy slices: the nulls stay
    std::vector<Field> f;
    for (size_t c = 0; c < df.columns.size(); ++c) f.push_back(Field{df.names[c], df.columns[c]->data_type(), true});
    auto schema = std::make_shared<Schema>(f);
    std::vector<RecordBatch> out;
    for (size_t lo = 0; lo < df.height(); lo += batch) {
        std::vector<ArrayRef> cols;
        for (auto &c : df.columns) cols.push_back(c->slice(lo, std::min(batch, df.height() - lo)));
        out.push_back(RecordBatch::try_new(schema, std::move(cols)));
    }
    return out;
}
std::optional<int64_t> ival(const ArrayRef &a, size_t i) { return std::dynamic_pointer_cast<const Int64Array>(a)->value(i); }
std::optional<double> fval(const ArrayRef &a, size_t i) { return std::dynamic_pointer_cast<const Float64Array>(a)->value(i); }
uint64_t splitmix64(uint64_t z) {  // the generator of rv_generate (include/rivulus_gpu.h, rv_synth_spec)
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

// ---- lowering (no device) -------------------------------------------------------------------------------------------------------
CPU_TEST(select_expressions_lower_to_names_dtypes_and_programs) {
    const Schema s = abc_schema();
    auto l = lower_select_exprs({col("a").add(col("b")), col("a").mul(Expr::lit(2)).alias("d"), col("a").div(col("b").sub(flit(1.5))), col("b"),
                                 col("a").alias("z"), col("a").div(col("a")), col("nope").add(col("a"))},
                                s);
    CHECK(l.size() == 7);
    CHECK(l[0].name == "a" && l[0].data_type == DataType::Float64 && l[0].computed());
    CHECK((l[0].program == std::vector<ArithStep>{step_col("a"), step_col("b"), step_op(RV_ARITH_ADD)}));
    CHECK(l[1].name == "d" && l[1].data_type == DataType::Int64);
    CHECK((l[1].program == std::vector<ArithStep>{step_col("a"), step_lit(int64_t{2}), step_op(RV_ARITH_MUL)}));
    CHECK(l[2].name == "a" && l[2].data_type == DataType::Float64);
    CHECK((l[2].program == std::vector<ArithStep>{step_col("a"), step_col("b"), step_lit(1.5), step_op(RV_ARITH_SUB), step_op(RV_ARITH_DIV)}));
    CHECK(!l[3].computed() && l[3].source == "b" && l[3].name == "b" && l[3].data_type == DataType::Float64);  // a plain column beside computed ones
    CHECK(!l[4].computed() && l[4].source == "a" && l[4].name == "z" && l[4].data_type == DataType::Int64);
    CHECK(l[5].data_type == DataType::Int64);  // Int64 / Int64 stays Int64
    CHECK(l[6].name == "nope" && l[6].data_type == DataType::Int64);  // a column the schema lacks types as Null (resolve_expr_schema): Null + Int64
    // the left-most leaf names the column, a literal as "literal"; an alias inside names its subtree
    CHECK(lower_select_exprs({Expr::lit(2).mul(col("a"))}, s)[0].name == "literal");
    CHECK(lower_select_exprs({col("a").alias("x").add(col("b"))}, s)[0].name == "x");
    CHECK(lower_select_exprs({Expr::lit(Literal()).add(col("a"))}, s)[0].data_type == DataType::Int64);  // Null o Int64
}

CPU_TEST(what_a_projection_refuses) {
    const Schema s = abc_schema();
    auto kind_of = [&](const Expr &e) -> int {
        try {
            lower_select_exprs({e}, s);
        } catch (const ConversionError &c) {
            return c.kind;
        }
        return -1;
    };
    CHECK(kind_of(Expr::lit(1)) == ConversionError::InvalidSelectExpression);  // a bare literal
    CHECK(thrown<ConversionError>([&] { lower_select_exprs({Expr::lit(1)}, s); }) == "Select expression must be a column or alias");
    CHECK(kind_of(Expr::lit(1).alias("one")) == ConversionError::UnsupportedExpression);
    CHECK(kind_of(Expr::lit(1).add(Expr::lit(2))) == ConversionError::UnsupportedExpression);  // reads no column
    CHECK(kind_of(col("a").gt(Expr::lit(1))) == ConversionError::UnsupportedExpression);       // not arithmetic
    CHECK(kind_of(col("a").add(col("a").gt(Expr::lit(1)))) == ConversionError::UnsupportedExpression);
    auto status_of = [&](const Expr &e) -> int {
        try {
            lower_select_exprs({e}, s);
        } catch (const Error &err) {
            return err.status;
        }
        return RV_OK;
    };
    CHECK(status_of(col("c").add(Expr::lit(1))) == RV_ERR_TYPE_MISMATCH);    // a Boolean column
    CHECK(status_of(col("a").add(Expr::lit("x"))) == RV_ERR_TYPE_MISMATCH);  // a String literal
    CHECK(status_of(col("a").mul(Expr::lit(Literal(true)))) == RV_ERR_TYPE_MISMATCH);
}

CPU_TEST(computed_predicates_lower_to_helpers_and_ordinary_terms) {
    const Schema s = abc_schema();
    ComputedPredicate p = lower_computed_predicate(col("a").add(col("b")).gt(Expr::lit(10)).and_(col("c")), s);
    CHECK(p.helpers.size() == 1 && p.helpers[0].name == "__arith0" && p.helpers[0].data_type == DataType::Float64);
    CHECK((p.helpers[0].program == std::vector<ArithStep>{step_col("a"), step_col("b"), step_op(RV_ARITH_ADD)}));
    CHECK(p.predicate.terms.size() == 2 && p.predicate.expr.empty());  // AND alone: the plain term list
    CHECK(p.predicate.terms[0].column == "__arith0" && p.predicate.terms[0].op == RV_GT && p.predicate.terms[0].literal == Literal(int64_t{10}));
    CHECK(p.predicate.terms[1].column == "c" && p.predicate.terms[1].op == RV_IS_TRUE);
    // under OR, beside an ordinary compare, two helpers
    p = lower_computed_predicate(col("a").mul(col("a")).lte(flit(2.5)).or_(col("b").lt(Expr::lit(0)).and_(col("b").sub(col("a")).neq(Expr::lit(1)))), s);
    CHECK(p.helpers.size() == 2 && p.helpers[1].name == "__arith1" && p.helpers[0].data_type == DataType::Int64);
    CHECK(p.predicate.terms.size() == 3 && p.predicate.terms[1].column == "b" && p.predicate.terms[2].column == "__arith1" && p.predicate.terms[2].op == RV_NE);
    CHECK((p.predicate.expr == std::vector<uint8_t>{0, 1, 2, RV_EXPR_AND, RV_EXPR_OR}));
    // the widened projection: the batch's columns, then the helpers
    auto all = with_arith_helpers(s, p.helpers);
    CHECK(all.size() == 5 && !all[2].computed() && all[2].source == "c" && all[3].name == "__arith0" && all[4].computed());
    // what it still refuses: arithmetic on the right, a column against a column
    CHECK(!thrown<StreamingPlannerError>([&] { lower_computed_predicate(Expr::lit(1).gt(col("a").add(col("b"))), s); }).empty());
    CHECK(!thrown<StreamingPlannerError>([&] { lower_computed_predicate(col("a").add(col("b")).gt(col("a")), s); }).empty());
    CHECK(!thrown<StreamingPlannerError>([&] { lower_computed_predicate(Expr::lit(1).add(Expr::lit(2)).gt(Expr::lit(1)), s); }).empty());
}

CPU_TEST(the_reference_grammar_refuses_what_it_refused) {
    const Expr sum = col("a").add(col("b"));
    auto kind_of = [](auto f) -> int {
        try {
            f();
        } catch (const ConversionError &c) {
            return c.kind;
        }
        return -1;
    };
    CHECK(kind_of([&] { convert_select_expr(sum); }) == ConversionError::UnsupportedExpression);
    CHECK(kind_of([&] { convert_select_expr(sum.alias("s")); }) == ConversionError::UnsupportedExpression);
    CHECK(kind_of([&] { convert_filter_predicate(sum); }) == ConversionError::UnsupportedFilterOperator);
    CHECK(kind_of([&] { convert_filter_predicate(sum.gt(Expr::lit(10))); }) == ConversionError::FilterLeftNotColumn);
    CHECK(thrown<StreamingPlannerError>([&] { extract_column_names_from_expressions({sum}); }) ==
          "Expression conversion error: Complex expressions not yet supported in streaming mode");
    CHECK(thrown<StreamingPlannerError>([&] { extract_column_names_from_expressions({sum.alias("s")}); }) ==
          "Expression conversion error: Complex expressions with aliases not yet supported");
    CHECK(thrown<StreamingPlannerError>([&] { extract_boolean_predicate_column(sum.gt(Expr::lit(1))); }) ==
          "Expression conversion error: Complex binary expressions not supported in streaming mode");
    CHECK(!thrown<StreamingPlannerError>([&] { lower_predicate(col("a").add(Expr::lit(1))); }).empty());
    CHECK(!thrown<StreamingPlannerError>([&] { lower_predicate(sum.gt(Expr::lit(10))); }).empty());
}

// ---- on the device ------------------------------------------------------------------------------------------------------------------
GPU_TEST(eager_project_over_filter) {
    const size_t n = 1000;
    DeviceFrame df = ab_frame(n, true);
    auto plan = PhysicalPlan::project(PhysicalPlan::filter(PhysicalPlan::source(df), CompareTerm{"b", RV_GT, Literal(0.0)}),
                                      {col("a").add(col("b")), col("a").mul(Expr::lit(2)).alias("d"), col("b"), col("a").div(col("a").sub(Expr::lit(3)))});
    DeviceFrame got = plan->execute();
    CHECK((got.names == std::vector<std::string>{"a", "d", "b", "a"}));
    CHECK(got.columns[0]->data_type() == DataType::Float64 && got.columns[1]->data_type() == DataType::Int64 && got.columns[3]->data_type() == DataType::Int64);
    size_t row = 0;
    for (size_t i = 0; i < n; ++i) {
        const auto a = ival(df.columns[0], i);
        const double b = *fval(df.columns[1], i);
        if (!(b > 0.0)) continue;
        CHECK(row < got.height());
        CHECK(fval(got.columns[0], row) == (a ? std::optional<double>(static_cast<double>(*a) + b) : std::nullopt));
        CHECK(ival(got.columns[1], row) == (a ? std::optional<int64_t>(*a * 2) : std::nullopt));
        CHECK(fval(got.columns[2], row) == b);
        CHECK(ival(got.columns[3], row) == (a && *a != 3 ? std::optional<int64_t>(*a / (*a - 3)) : std::nullopt));  // x / 0 is null
        ++row;
    }
    CHECK(row == got.height() && row > 100);
    CHECK(got.columns[2]->handle() != nullptr && !got.columns[2]->has_null_bitmap());
}

GPU_TEST(eager_computed_filter_orders_nulls_lowest) {
    const size_t n = 1000;
    DeviceFrame df = ab_frame(n, true);
    auto rows_of = [&](const Expr &p) { return PhysicalPlan::computed_filter(PhysicalPlan::source(df), p)->execute(); };
    // Gt: a null helper cell is below everything, the row goes; NotEq: null != x holds, the row stays (series.rs:87-117)
    const Expr sum = col("a").add(col("b"));
    for (bool ne : {false, true}) {
        DeviceFrame got = rows_of(ne ? sum.neq(flit(10.0)) : sum.gt(flit(10.0)));
        CHECK((got.names == std::vector<std::string>{"a", "b"}) && got.width() == 2);  // the helper is gone
        size_t row = 0, null_rows = 0;
        for (size_t i = 0; i < n; ++i) {
            const auto a = ival(df.columns[0], i);
            const double b = *fval(df.columns[1], i);
            const bool keep = a ? (ne ? static_cast<double>(*a) + b != 10.0 : static_cast<double>(*a) + b > 10.0) : ne;
            if (!keep) continue;
            CHECK(row < got.height() && ival(got.columns[0], row) == a && fval(got.columns[1], row) == b);
            null_rows += !a;
            ++row;
        }
        CHECK(row == got.height());
        CHECK(ne ? null_rows == n / 5 : null_rows == 0);
    }
    // under AND / OR with an ordinary term
    DeviceFrame got = rows_of(sum.gt(flit(10.0)).and_(col("b").lt(flit(50.0))).or_(col("a").mul(col("a")).eq(Expr::lit(400))));
    size_t want = 0;
    for (size_t i = 0; i < n; ++i) {
        const auto a = ival(df.columns[0], i);
        const double b = *fval(df.columns[1], i);
        want += (a && static_cast<double>(*a) + b > 10.0 && b < 50.0) || (a && *a * *a == 400);
    }
    CHECK(got.height() == want && want > 0);
}

GPU_TEST(a_missing_column_is_column_not_found) {
    DeviceFrame df = ab_frame(10, false);
    auto kind_and_text = [](const PhysicalPlanPtr &p) -> std::string {
        try {
            p->execute();
        } catch (const ExecutionError &e) {
            return std::to_string(e.kind) + " " + e.what();
        }
        return "";
    };
    const std::string want = std::to_string(ExecutionError::ColumnNotFound) + " Column not found: 'zz'";
    CHECK(kind_and_text(PhysicalPlan::project(PhysicalPlan::source(df), {col("a").add(col("zz"))})) == want);
    CHECK(kind_and_text(PhysicalPlan::project(PhysicalPlan::source(df), {col("a"), col("zz")})) == want);
    CHECK(kind_and_text(PhysicalPlan::select(PhysicalPlan::source(df), {"zz"}, {"zz"})) == want);  // Select's text
    CHECK(kind_and_text(PhysicalPlan::computed_filter(PhysicalPlan::source(df), col("zz").mul(col("a")).gt(Expr::lit(1)))) == want);
    // ... and a plain term beside a computed one that names no column of the frame
    CHECK(kind_and_text(PhysicalPlan::computed_filter(PhysicalPlan::source(df), col("a").add(col("b")).gt(Expr::lit(1)).and_(col("zz").gt(Expr::lit(1))))) == want);
    // a frame without columns is refused before anything is evaluated
    CHECK(thrown<Error>([&] { PhysicalPlan::computed_filter(PhysicalPlan::source(DeviceFrame{}), col("a").add(col("b")).gt(Expr::lit(1)))->execute(); }) ==
          "filter over a frame without columns");
    // a stream says it the way SelectStream does
    auto plan = StreamingPhysicalPlan::project(StreamingPhysicalPlan::memory_source(batches_of(df, 4)), {col("a").add(col("zz"))});
    CHECK(thrown<StreamingExecutionError>([&] { plan->execute(); }) == "Stream error: Stream execution error: Column 'zz' not found in schema");
}

GPU_TEST(streaming_project_equals_the_eager_one) {
    const size_t n = 2500;
    DeviceFrame df = ab_frame(n, true);
    const std::vector<Expr> exprs = {col("a").add(col("b")), col("b"), col("a").div(col("a").add(Expr::lit(5))).alias("q")};
    DeviceFrame eager = PhysicalPlan::project(PhysicalPlan::source(df), exprs)->execute();
    auto plan = StreamingPhysicalPlan::project(StreamingPhysicalPlan::memory_source(batches_of(df, 1024)), exprs);
    auto stream = plan->execute();
    CHECK(stream->schema()->num_fields() == 3 && stream->schema()->field(0).name() == "a" && stream->schema()->field(0).data_type() == DataType::Float64);
    CHECK(stream->schema()->field(2).name() == "q" && stream->schema()->field(2).data_type() == DataType::Int64);
    auto got = stream->collect();
    CHECK(got.size() == 3 && got[0].num_rows() == 1024 && got[1].num_rows() == 1024 && got[2].num_rows() == 452);  // the last one short
    size_t at = 0;
    for (auto &b : got) {
        CHECK(*b.schema() == *stream->schema());
        CHECK(cells(b.columns(), 0, b.num_rows()) == cells(eager.columns, at, at + b.num_rows()));
        at += b.num_rows();
    }
    CHECK(at == n);
    RecordBatch all = plan->collect(ctx());
    CHECK(all.num_rows() == n && cells(all.columns(), 0, n) == cells(eager.columns, 0, n));
}

GPU_TEST(streaming_computed_filter_equals_the_eager_one_without_nulls) {
    const size_t n = 2500;
    DeviceFrame df = ab_frame(n, false);
    const Expr p = col("a").add(col("b")).gt(flit(10.0)).and_(col("b").lt(flit(50.0))).or_(col("a").mul(col("a")).eq(Expr::lit(400)));
    DeviceFrame eager = PhysicalPlan::computed_filter(PhysicalPlan::source(df), p)->execute();
    auto plan = StreamingPhysicalPlan::computed_filter_project(StreamingPhysicalPlan::memory_source(batches_of(df, 1024)), p, {"a", "b"});
    auto stream = plan->execute();
    CHECK(stream->schema()->num_fields() == 2);  // the helpers are dropped from the result
    auto got = stream->collect();
    CHECK(got.size() == 3);  // one output batch per input batch
    RecordBatch all = RecordBatch::concat(got);
    CHECK(all.num_rows() == eager.height() && eager.height() > 0 && eager.height() < n);
    CHECK(cells(all.columns(), 0, all.num_rows()) == cells(eager.columns, 0, eager.height()));
    // over a resident frame (DataFrameSource) too
    auto plan2 = StreamingPhysicalPlan::computed_filter_project(StreamingPhysicalPlan::dataframe_source(df, 1024), p, {"b"});
    RecordBatch all2 = plan2->collect(ctx());
    CHECK(all2.num_rows() == eager.height() && cells(all2.columns(), 0, all2.num_rows()) == cells({eager.columns[1]}, 0, eager.height()));
}

GPU_TEST(with_nulls_the_two_null_policies_differ_by_design) {
    // four rows; the helper a + b is {2, null, 21, null}.  `!= 2`: the eager filter orders null lowest, so null != 2 holds and the
    // null rows stay (RV_NULL_IS_LEAST); a stream drops a row whose compare reads a null cell (RV_NULL_DROPS).
    DeviceFrame df;
    df.names = {"a", "b"};
    df.columns = {Int64Array::create(ctx(), {1, 0, 20, 0}, std::vector<bool>{true, false, true, false}), Int64Array::from_values(ctx(), {1, 1, 1, 1})};
    const Expr p = col("a").add(col("b")).neq(Expr::lit(2));
    DeviceFrame eager = PhysicalPlan::computed_filter(PhysicalPlan::source(df), p)->execute();
    CHECK(eager.height() == 3);
    CHECK((cells(eager.columns, 0, 3) == Table{{"null", "20", "null"}, {"1", "1", "1"}}));
    RecordBatch streamed = StreamingPhysicalPlan::computed_filter_project(StreamingPhysicalPlan::memory_source(batches_of(df, 1024)), p, {"a", "b"})->collect(ctx());
    CHECK(streamed.num_rows() == 1);
    CHECK((cells(streamed.columns(), 0, 1) == Table{{"20"}, {"1"}}));
}

GPU_TEST(a_limit_downstream_of_a_project_still_bounds_the_scan) {
    const uint64_t n = uint64_t{1} << 25;  // more rows than the bound below: unhinted, the operator would filter all of them
    rv_synth_spec spec{};
    spec.dtype = RV_INT64;
    spec.seed = 42;
    spec.length = n;
    spec.modulus = 1000;
    rv_dcolumn *h = nullptr;
    check(rv_generate(ctx()->raw(), &spec, &h));
    DeviceFrame df;
    df.names = {"x"};
    df.columns = {Array::adopt(ctx(), h)};
    auto scanned = [&] {
        int64_t v = 0;
        check(rv_ctx_get_option(ctx()->raw(), "fused_rows_scanned", &v));
        return static_cast<uint64_t>(v);
    };
    auto filtered = StreamingPhysicalPlan::gpu_filter_project(StreamingPhysicalPlan::dataframe_source(df, 1024), lower_predicate(col("x").gt(Expr::lit(899))), {"x"});
    auto plan = StreamingPhysicalPlan::limit(StreamingPhysicalPlan::project(filtered, {col("x").mul(Expr::lit(2)).add(Expr::lit(1)).alias("y"), col("x")}), 10);
    const uint64_t before = scanned();
    RecordBatch got = plan->collect(ctx());
    const uint64_t touched = scanned() - before;
    CHECK(got.num_rows() == 10 && got.schema()->field(0).name() == "y");
    CHECK(touched > 0 && touched < 10000000);
    size_t row = 0;
    for (uint64_t i = 0; i < n && row < 10; ++i) {
        const int64_t v = static_cast<int64_t>(splitmix64(42 + i) % 1000);
        if (v <= 899) continue;
        CHECK(ival(got.column(0), row) == 2 * v + 1 && ival(got.column(1), row) == v);
        ++row;
    }
    CHECK(row == 10);
}
