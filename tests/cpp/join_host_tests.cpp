// Tests of the eager PhysicalPlan::HashJoin arm of the C++ host layer (rivulus_amd/host/rivulus_host.hpp) against the
// reference's plan.rs:174-284.
//   join_host_tests --cpu   cases without a device
//   join_host_tests         every case (needs an MI355X)
// Output: "ok <name>" / "FAIL <name>: why"; exit status 0 iff all pass.
#include "host_test_main.hpp"

using namespace rivulus;
using namespace rivulus::execution;
using namespace rivulus::physical_plan;

namespace {
template <class E, class F>
bool throws(F f) {
    try {
        f();
    } catch (const E &) {
        return true;
    }
    return false;
}
}  // namespace

CPU_TEST(missing_key_column_is_the_references_unwrap) {  // plan.rs:184, :195: column(..).unwrap()
    DeviceFrame empty;
    auto plan = PhysicalPlan::hash_join(PhysicalPlan::source(empty), PhysicalPlan::source(empty), "user_id", "user_id");
    CHECK(throws<Panic>([&] { plan->execute(); }));
}

// the reference demo's users / orders (main.rs, queries 6 and 7): users is the left (build) frame
DeviceFrame users() {
    DeviceFrame f;
    f.names = {"user_id", "name", "city"};
    f.columns = {Int64Array::from_values(ctx(), {1, 2, 3, 4}), StringArray::from_strings(ctx(), {"Alice", "Bob", "Charlie", "Diana"}),
                 StringArray::from_strings(ctx(), {"NYC", "LA", "Chicago", "Boston"})};
    return f;
}
DeviceFrame orders() {
    DeviceFrame f;
    f.names = {"order_id", "user_id", "amount"};
    f.columns = {Int64Array::from_values(ctx(), {101, 102, 103, 104, 105}), Int64Array::from_values(ctx(), {1, 2, 1, 3, 99}),
                 Float64Array::from_values(ctx(), {25.99, 15.50, 99.99, 45.00, 12.99})};
    return f;
}
std::optional<std::string> str_at(const ArrayRef &a, size_t i) { return std::dynamic_pointer_cast<const StringArray>(a)->value(i); }
std::optional<int64_t> i64_at(const ArrayRef &a, size_t i) { return std::dynamic_pointer_cast<const Int64Array>(a)->value(i); }

GPU_TEST(users_join_orders_demo) {
    DeviceFrame out = PhysicalPlan::hash_join(PhysicalPlan::source(users()), PhysicalPlan::source(orders()), "user_id", "user_id")->execute();
    CHECK((out.names == std::vector<std::string>{"order_id", "user_id", "amount", "name", "city"}));
    CHECK(out.height() == 4);
    const int64_t oid[] = {101, 102, 103, 104};
    const char *name[] = {"Alice", "Bob", "Alice", "Charlie"}, *city[] = {"NYC", "LA", "NYC", "Chicago"};
    for (size_t i = 0; i < 4; ++i) {
        CHECK(*i64_at(out.columns[0], i) == oid[i]);
        CHECK(*str_at(out.columns[3], i) == name[i] && *str_at(out.columns[4], i) == city[i]);
    }
    CHECK(*std::dynamic_pointer_cast<const Float64Array>(out.columns[2])->value(2) == 99.99);
}

GPU_TEST(name_collisions_get_the_right_suffix_and_nulls_stay_null) {  // materialize_join_result's `{}_right`
    DeviceFrame b, p;
    b.names = {"k", "v", "flag"};
    b.columns = {Int64Array::create(ctx(), {1, 2, 0}, std::vector<bool>{true, true, false}), Int64Array::create(ctx(), {10, 20, 30}, std::vector<bool>{true, false, true}),
                 BooleanArray::create(ctx(), {true, std::nullopt, false})};
    p.names = {"v", "k"};
    p.columns = {StringArray::create(ctx(), {"a", std::nullopt, "c"}), Int64Array::create(ctx(), {2, 0, 1}, std::vector<bool>{true, false, true})};
    DeviceFrame out = PhysicalPlan::hash_join(PhysicalPlan::source(b), PhysicalPlan::source(p), "k", "k")->execute();
    CHECK((out.names == std::vector<std::string>{"v", "k", "v_right", "flag"}));
    CHECK(out.height() == 3);  // probe rows 0 (k=2 -> build 1), 1 (null -> build 2), 2 (k=1 -> build 0)
    CHECK(*str_at(out.columns[0], 0) == "a" && !str_at(out.columns[0], 1) && *str_at(out.columns[0], 2) == "c");
    CHECK(!i64_at(out.columns[2], 0) && *i64_at(out.columns[2], 1) == 30 && *i64_at(out.columns[2], 2) == 10);
    auto flag = std::dynamic_pointer_cast<const BooleanArray>(out.columns[3]);
    CHECK(!flag->value(0) && *flag->value(1) == false && *flag->value(2) == true);
}

GPU_TEST(empty_result_keeps_names_and_dtypes) {  // create_empty_join_result (plan.rs:257-284)
    DeviceFrame o = orders();
    o.columns[1] = Int64Array::from_values(ctx(), {7, 8, 9, 10, 11});
    DeviceFrame out = PhysicalPlan::hash_join(PhysicalPlan::source(users()), PhysicalPlan::source(o), "user_id", "user_id")->execute();
    CHECK(out.height() == 0 && out.width() == 5);
    CHECK(out.columns[2]->data_type() == DataType::Float64 && out.columns[4]->data_type() == DataType::String);
}
