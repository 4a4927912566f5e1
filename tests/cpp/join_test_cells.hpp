// Cells of device arrays as text, for the join test programs to compare frames by: the value, "null", a Float64 by its 17
// digits (so -0.0 and 0.0 differ), a String in quotes.
#pragma once

#include <cstdio>
#include <string>
#include <vector>

#include "../../rivulus_amd/host/rivulus_host.hpp"

namespace {
[[maybe_unused]] std::string f17(double x) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.17g", x);
    return buf;
}
[[maybe_unused]] std::string cell(const rivulus::execution::ArrayRef &a, size_t i) {
    using namespace rivulus::execution;
    switch (a->data_type()) {
        case DataType::Int64: {
            auto v = std::dynamic_pointer_cast<const Int64Array>(a)->value(i);
            return v ? std::to_string(*v) : "null";
        }
        case DataType::Float64: {
            auto v = std::dynamic_pointer_cast<const Float64Array>(a)->value(i);
            return v ? f17(*v) : "null";
        }
        case DataType::Boolean: {
            auto v = std::dynamic_pointer_cast<const BooleanArray>(a)->value(i);
            return v ? (*v ? "true" : "false") : "null";
        }
        case DataType::String: {
            auto v = std::dynamic_pointer_cast<const StringArray>(a)->value(i);
            return v ? "'" + *v + "'" : "null";
        }
        default: return "null";
    }
}
// a frame's rows [lo, hi) as text, column by column
using Table = std::vector<std::vector<std::string>>;
[[maybe_unused]] Table cells(const std::vector<rivulus::execution::ArrayRef> &cols, size_t lo, size_t hi) {
    Table out;
    for (auto &c : cols) {
        out.emplace_back();
        for (size_t i = lo; i < hi; ++i) out.back().push_back(cell(c, i));
    }
    return out;
}
}  // namespace
