// C++ host layer above the C ABI (include/rivulus_gpu.h): the mirror of the reference's
// operator interfaces for the filter / project / scan path, with every array resident in
// HBM.  Same names, argument meaning and error texts as the reference (Rust), so code written
// against the reference reads the same here:
//
//   execution::{DataType, Field, Schema}                    src/execution/schema.rs:1-76
//   execution::{PrimitiveArray<T>, BooleanArray}             src/execution/array/{primitive,boolean}.rs
//   execution::RecordBatch                                   src/execution/record_batch.rs:8-422
//   execution::{DataStream, MemoryStream, FilterStream,
//               SelectStream, LimitStream}                   src/execution/stream.rs:25-213, streaming.rs:246-288
//   execution::GpuFilterProjectStream                        the operator the new backend adds at seam S1
//   execution::GpuHashJoinStream                             StreamingPhysicalPlan::HashJoin (todo!() in the reference, streaming.rs:128-131)
//   expressions::{Expr, BinaryOperator}                      src/expressions/expr.rs:3-139
//   physical_plan::{convert_filter_predicate, convert_select_expr,
//                   extract_boolean_predicate_column,
//                   extract_column_names_from_expressions}   planner.rs:113-189, streaming_planner.rs:102-168
//   physical_plan::lower_predicate                           compare / AND / OR lowering (replaces the rejection at
//                                                            streaming_planner.rs:141-162)
//   physical_plan::{lower_select_exprs,
//                   lower_computed_predicate}               arithmetic select / filter expressions (expr.rs:44-74; refused by the
//                                                            reference at planner.rs:124-126, :151-156) -> rv_eval_arith
//   execution::GpuProjectStream                              select([...]) with computed columns, batch by batch
//   physical_plan::StreamingPhysicalPlan                     streaming.rs:29-133, :235-238, :343-352
//   physical_plan::PhysicalPlan (Source/Filter/Select)       plan.rs:8-150 over typed device columns
//
// String columns live on the device as well (bytes + int32 offsets + validity): they ride through
// filter / take / concat and `name == "Bob"` compare terms run on the device (byte-wise str ordering).
// There is no CPU fallback anywhere in this layer.
#pragma once

#include <cstring>
#include <exception>
#include <cstdlib>
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <fstream>
#include <functional>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "../../include/rivulus_gpu.h"

namespace rivulus {

// Err(String) of the reference; `status` is the C-ABI code it came with.
struct Error : std::runtime_error {
    rv_status status;
    Error(rv_status s, const std::string &m) : std::runtime_error(m), status(s) {}
};
struct Panic : std::runtime_error {  // Rust assert!/panic!
    using std::runtime_error::runtime_error;
};

inline void check(rv_status s) {
    if (s != RV_OK) throw Error(s, rv_last_error());
}

// One device + one stream (rv_ctx).  Shared by the arrays created from it.
class Context {
  public:
    explicit Context(int device = 0) { check(rv_ctx_create(device, &ctx_)); }
    ~Context() { rv_ctx_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    rv_ctx *raw() const { return ctx_; }

  private:
    rv_ctx *ctx_ = nullptr;
};
using ContextRef = std::shared_ptr<Context>;

namespace execution {

// ---------------------------------------------------------------------------------------
// schema.rs:1-76
// ---------------------------------------------------------------------------------------
enum class DataType { Null, Boolean, Int64, Float64, String };
inline const char *to_string(DataType t) {
    static const char *n[] = {"Null", "Boolean", "Int64", "Float64", "String"};
    return n[static_cast<int>(t)];
}
inline rv_dtype to_rv(DataType t) { return static_cast<rv_dtype>(static_cast<int>(t)); }
inline DataType from_rv(rv_dtype t) { return static_cast<DataType>(static_cast<int>(t)); }

class Field {
  public:
    Field(std::string name, DataType data_type, bool nullable) : name_(std::move(name)), data_type_(data_type), nullable_(nullable) {}
    const std::string &name() const { return name_; }
    DataType data_type() const { return data_type_; }
    bool is_nullable() const { return nullable_; }
    bool operator==(const Field &o) const { return name_ == o.name_ && data_type_ == o.data_type_ && nullable_ == o.nullable_; }

  private:
    std::string name_;
    DataType data_type_;
    bool nullable_;
};

class Schema {
  public:
    Schema() = default;
    explicit Schema(std::vector<Field> fields) : fields_(std::move(fields)) {}
    static Schema empty() { return Schema(); }
    const std::vector<Field> &fields() const { return fields_; }
    const Field &field(size_t i) const { return fields_.at(i); }
    const Field *field_by_name(const std::string &n) const {
        for (auto &f : fields_)
            if (f.name() == n) return &f;
        return nullptr;
    }
    std::optional<size_t> index_of(const std::string &n) const {
        for (size_t i = 0; i < fields_.size(); ++i)
            if (fields_[i].name() == n) return i;
        return std::nullopt;
    }
    size_t num_fields() const { return fields_.size(); }
    bool is_empty() const { return fields_.empty(); }
    bool operator==(const Schema &o) const { return fields_ == o.fields_; }
    bool operator!=(const Schema &o) const { return !(*this == o); }

  private:
    std::vector<Field> fields_;
};
using SchemaRef = std::shared_ptr<const Schema>;

// ---------------------------------------------------------------------------------------
// trait Array (array/mod.rs:10-16): a device column handle
// ---------------------------------------------------------------------------------------
class Array;
using ArrayRef = std::shared_ptr<const Array>;

class Array {
  public:
    virtual ~Array() {
        if (handle_) rv_free(ctx_ ? ctx_->raw() : nullptr, handle_);
    }
    virtual size_t len() const { return info().length; }
    virtual DataType data_type() const { return from_rv(info().dtype); }
    virtual size_t null_count() const {  // primitive.rs:90-105
        uint64_t n = 0;
        check(rv_null_count(ctx_->raw(), handle_, &n));
        return n;
    }
    virtual ArrayRef slice(size_t offset, size_t length) const {  // primitive.rs:107-117 (zero copy)
        if (offset + length > len()) throw Panic("Slice out of bounds");
        rv_dcolumn *out = nullptr;
        check(rv_slice(ctx_->raw(), handle_, offset, length, &out));
        return adopt(ctx_, out);
    }
    bool has_null_bitmap() const { return info().has_validity != 0; }  // `null_bitmap.is_some()`
    rv_dcolumn *handle() const { return handle_; }
    const ContextRef &context() const { return ctx_; }
    bool on_device() const { return handle_ != nullptr; }

    // adopts a handle returned by the C ABI; the concrete type follows its dtype
    static ArrayRef adopt(const ContextRef &ctx, rv_dcolumn *h);

  protected:
    Array() = default;
    Array(ContextRef ctx, rv_dcolumn *h) : ctx_(std::move(ctx)), handle_(h) {}
    rv_column_info info() const {
        rv_column_info i{};
        check(rv_column_info_get(ctx_->raw(), handle_, &i));
        return i;
    }
    // host copy of the logical range, fetched once (element access is for tests and display)
    struct HostCopy {
        std::vector<uint64_t> values;   // 8-byte cells, or bit bytes packed in the low part for Boolean
        std::vector<uint8_t> bits;      // Boolean value bits
        std::vector<uint8_t> validity;  // empty: no null bitmap
    };
    const HostCopy &host() const {
        if (!host_) {
            auto h = std::make_shared<HostCopy>();
            const rv_column_info i = info();
            const size_t n = i.length, nb = (n + 7) / 8;
            int hv = 0;
            if (i.has_validity) h->validity.resize(std::max<size_t>(nb, 1));
            if (i.dtype == RV_BOOLEAN) {
                h->bits.resize(std::max<size_t>(nb, 1));
                check(rv_download(ctx_->raw(), handle_, h->bits.data(), i.has_validity ? h->validity.data() : nullptr, &hv));
            } else {
                h->values.resize(std::max<size_t>(n, 1));
                check(rv_download(ctx_->raw(), handle_, h->values.data(), i.has_validity ? h->validity.data() : nullptr, &hv));
            }
            host_ = h;
        }
        return *host_;
    }
    bool host_valid(size_t i) const {
        const HostCopy &h = host();
        return h.validity.empty() || ((h.validity[i / 8] >> (i % 8)) & 1);
    }
    ContextRef ctx_;
    rv_dcolumn *handle_ = nullptr;
    mutable std::shared_ptr<HostCopy> host_;
};

inline std::vector<uint8_t> pack_bits(const std::vector<bool> &v) {  // BitMap::from_bool_slice, bitmap.rs:44-59
    std::vector<uint8_t> out((v.size() + 7) / 8, 0);
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i]) out[i / 8] |= static_cast<uint8_t>(1u << (i % 8));
    return out;
}

// PrimitiveArray<i64|f64> -- primitive.rs:20-122
template <class T>
class PrimitiveArray : public Array {
    static_assert(sizeof(T) == 8, "Int64 / Float64");

  public:
    static constexpr DataType kType = std::is_same<T, double>::value ? DataType::Float64 : DataType::Int64;
    PrimitiveArray(ContextRef ctx, rv_dcolumn *h) : Array(std::move(ctx), h) {}

    // PrimitiveArray::new(values, validity) -- primitive.rs:31-42
    static std::shared_ptr<const PrimitiveArray> create(const ContextRef &ctx, const std::vector<T> &values,
                                                        const std::optional<std::vector<bool>> &validity = std::nullopt) {
        std::vector<uint8_t> vbits;
        if (validity) {
            if (validity->size() != values.size()) throw Error(RV_ERR_LENGTH_MISMATCH, "validity length != values length");
            vbits = pack_bits(*validity);
            if (vbits.empty()) vbits.push_back(0);
        }
        rv_column c{};
        c.dtype = to_rv(kType);
        c.values = values.data();
        c.validity = validity ? vbits.data() : nullptr;
        c.length = values.size();
        rv_dcolumn *h = nullptr;
        check(rv_upload(ctx->raw(), &c, &h));
        return std::make_shared<const PrimitiveArray>(ctx, h);
    }
    static std::shared_ptr<const PrimitiveArray> from_values(const ContextRef &ctx, const std::vector<T> &values) {  // :44-46
        return create(ctx, values);
    }
    // primitive.rs:48-60
    std::optional<T> value(size_t index) const {
        if (index >= len()) throw Panic("Index " + std::to_string(index) + " out of bounds");
        if (!host_valid(index)) return std::nullopt;
        T out;
        std::memcpy(&out, &host().values[index], 8);
        return out;
    }
    // the raw slot, placeholder included (take_array writes 0 / 0.0 under nulls, record_batch.rs:142-146)
    T raw_value(size_t index) const {
        T out;
        std::memcpy(&out, &host().values.at(index), 8);
        return out;
    }
};
using Int64Array = PrimitiveArray<int64_t>;
using Float64Array = PrimitiveArray<double>;

// BooleanArray -- boolean.rs:9-180
class BooleanArray : public Array {
  public:
    BooleanArray(ContextRef ctx, rv_dcolumn *h) : Array(std::move(ctx), h) {}
    // BooleanArray::new(Vec<Option<bool>>) -- boolean.rs:19-50 (false under null, bitmap dropped when no null)
    static std::shared_ptr<const BooleanArray> create(const ContextRef &ctx, const std::vector<std::optional<bool>> &v) {
        std::vector<bool> vals(v.size()), valid(v.size());
        bool any_null = false;
        for (size_t i = 0; i < v.size(); ++i) {
            vals[i] = v[i].value_or(false);
            valid[i] = v[i].has_value();
            any_null |= !valid[i];
        }
        return upload(ctx, vals, any_null ? std::optional<std::vector<bool>>(valid) : std::nullopt);
    }
    static std::shared_ptr<const BooleanArray> from_bools(const ContextRef &ctx, const std::vector<bool> &v) {  // :52-55
        return upload(ctx, v, std::nullopt);
    }
    static std::shared_ptr<const BooleanArray> all_true(const ContextRef &ctx, size_t n) { return from_bools(ctx, std::vector<bool>(n, true)); }
    static std::shared_ptr<const BooleanArray> all_false(const ContextRef &ctx, size_t n) { return from_bools(ctx, std::vector<bool>(n, false)); }

    std::optional<bool> value(size_t index) const {  // boolean.rs:92-104
        if (index >= len()) throw Panic("Index " + std::to_string(index) + " out of bounds");
        if (!host_valid(index)) return std::nullopt;
        return ((host().bits[index / 8] >> (index % 8)) & 1) != 0;
    }
    // boolean.rs:120-165: strict null propagation; errors keep the reference text
    std::shared_ptr<const BooleanArray> logical_and(const BooleanArray &o) const { return binary(&rv_boolean_and, o); }
    std::shared_ptr<const BooleanArray> logical_or(const BooleanArray &o) const { return binary(&rv_boolean_or, o); }
    std::shared_ptr<const BooleanArray> logical_not() const {
        rv_dcolumn *out = nullptr;
        check(rv_boolean_not(ctx_->raw(), handle_, &out));
        return std::make_shared<const BooleanArray>(ctx_, out);
    }
    size_t count_true() const {  // boolean.rs:167-172
        uint64_t t = 0, f = 0;
        check(rv_boolean_count(ctx_->raw(), handle_, &t, &f));
        return t;
    }
    size_t count_false() const {
        uint64_t t = 0, f = 0;
        check(rv_boolean_count(ctx_->raw(), handle_, &t, &f));
        return f;
    }

  private:
    static std::shared_ptr<const BooleanArray> upload(const ContextRef &ctx, const std::vector<bool> &vals,
                                                      const std::optional<std::vector<bool>> &valid) {
        std::vector<uint8_t> vb = pack_bits(vals), mb;
        if (vb.empty()) vb.push_back(0);
        if (valid) {
            mb = pack_bits(*valid);
            if (mb.empty()) mb.push_back(0);
        }
        rv_column c{};
        c.dtype = RV_BOOLEAN;
        c.values = vb.data();
        c.validity = valid ? mb.data() : nullptr;
        c.length = vals.size();
        rv_dcolumn *h = nullptr;
        check(rv_upload(ctx->raw(), &c, &h));
        return std::make_shared<const BooleanArray>(ctx, h);
    }
    using BinFn = rv_status (*)(rv_ctx *, const rv_dcolumn *, const rv_dcolumn *, rv_dcolumn **);
    std::shared_ptr<const BooleanArray> binary(BinFn fn, const BooleanArray &o) const {
        rv_dcolumn *out = nullptr;
        check(fn(ctx_->raw(), handle_, o.handle_, &out));
        return std::make_shared<const BooleanArray>(ctx_, out);
    }
};

// StringArray -- string.rs:8-190: UTF-8 bytes + int32 offsets + optional validity, on the device
class StringArray : public Array {
  public:
    StringArray(ContextRef ctx, rv_dcolumn *h) : Array(std::move(ctx), h) {}
    // StringArray::new(Vec<Option<String>>) -- string.rs:19-57: a null spans no bytes, the bitmap is
    // dropped when there is no null
    static std::shared_ptr<const StringArray> create(const ContextRef &ctx, const std::vector<std::optional<std::string>> &v) {
        std::vector<int32_t> offsets{0};
        std::string data;
        std::vector<bool> valid(v.size());
        bool any_null = false;
        for (size_t i = 0; i < v.size(); ++i) {
            valid[i] = v[i].has_value();
            any_null |= !valid[i];
            if (v[i]) data += *v[i];
            offsets.push_back(static_cast<int32_t>(data.size()));
        }
        std::vector<uint8_t> vb;
        if (any_null) {
            vb = pack_bits(valid);
            if (vb.empty()) vb.push_back(0);
        }
        rv_column c{};
        c.dtype = RV_STRING;
        c.values = data.data();
        c.data_bytes = data.size();
        c.offsets = offsets.data();
        c.validity = any_null ? vb.data() : nullptr;
        c.length = v.size();
        rv_dcolumn *h = nullptr;
        check(rv_upload(ctx->raw(), &c, &h));
        return std::make_shared<const StringArray>(ctx, h);
    }
    static std::shared_ptr<const StringArray> from_strings(const ContextRef &ctx, const std::vector<std::string> &v) {  // string.rs:59-62
        return create(ctx, std::vector<std::optional<std::string>>(v.begin(), v.end()));
    }
    std::optional<std::string> value(size_t i) const {  // string.rs:81-99
        if (i >= len()) throw Panic("Index " + std::to_string(i) + " out of bounds");
        const Strings &h = strings();
        if (!h.validity.empty() && !((h.validity[i / 8] >> (i % 8)) & 1)) return std::nullopt;
        return std::string(h.data.begin() + h.offsets[i], h.data.begin() + h.offsets[i + 1]);
    }
    size_t total_bytes() const { return info().data_bytes; }  // bytes of the logical elements

  private:
    struct Strings {
        std::vector<int32_t> offsets;
        std::vector<uint8_t> data, validity;
    };
    const Strings &strings() const {  // host copy, fetched once (element access is for tests and display)
        if (!strings_) {
            auto h = std::make_shared<Strings>();
            const rv_column_info i = info();
            h->offsets.resize(i.length + 1);
            h->data.resize(std::max<size_t>(i.data_bytes, 1));
            if (i.has_validity) h->validity.resize(std::max<size_t>((i.length + 7) / 8, 1));
            int hv = 0;
            check(rv_download_string(ctx_->raw(), handle_, h->offsets.data(), h->data.data(), i.has_validity ? h->validity.data() : nullptr, &hv));
            strings_ = h;
        }
        return *strings_;
    }
    mutable std::shared_ptr<Strings> strings_;
};

// NullArray -- null.rs:5-66: a length, every element null
class NullArray : public Array {
  public:
    NullArray(ContextRef ctx, rv_dcolumn *h) : Array(std::move(ctx), h) {}
    static std::shared_ptr<const NullArray> create(const ContextRef &ctx, size_t n) {
        rv_column c{};
        c.dtype = RV_NULL;
        c.length = n;
        rv_dcolumn *h = nullptr;
        check(rv_upload(ctx->raw(), &c, &h));
        return std::make_shared<const NullArray>(ctx, h);
    }
};

inline ArrayRef Array::adopt(const ContextRef &ctx, rv_dcolumn *h) {
    rv_column_info i{};
    check(rv_column_info_get(ctx->raw(), h, &i));
    switch (i.dtype) {
        case RV_INT64: return std::make_shared<const Int64Array>(ctx, h);
        case RV_FLOAT64: return std::make_shared<const Float64Array>(ctx, h);
        case RV_BOOLEAN: return std::make_shared<const BooleanArray>(ctx, h);
        case RV_STRING: return std::make_shared<const StringArray>(ctx, h);
        case RV_NULL: return std::make_shared<const NullArray>(ctx, h);
        default: rv_free(ctx->raw(), h); throw Error(RV_ERR_UNSUPPORTED, "unsupported device array type");
    }
}
// the handles a C-ABI call returned, adopted in their order
inline std::vector<ArrayRef> adopt_columns(const ContextRef &ctx, const std::vector<rv_dcolumn *> &out) {
    std::vector<ArrayRef> res;
    for (auto *h : out) res.push_back(Array::adopt(ctx, h));
    return res;
}
// ... and the handles a C-ABI call takes: those of `columns`, in their order.  A column off the device is refused with `off_device`.
inline std::vector<const rv_dcolumn *> column_handles(const std::vector<ArrayRef> &columns,
                                                      const std::string &off_device = "columns off the device are outside the device path") {
    std::vector<const rv_dcolumn *> h;
    for (auto &c : columns) {
        if (!c->on_device()) throw Error(RV_ERR_UNSUPPORTED, off_device);
        h.push_back(c->handle());
    }
    return h;
}

// ---------------------------------------------------------------------------------------
// RecordBatch -- record_batch.rs:8-422
// ---------------------------------------------------------------------------------------
class RecordBatch {
  public:
    RecordBatch() : schema_(std::make_shared<Schema>()), num_rows_(0) {}
    // record_batch.rs:16-58
    static RecordBatch try_new(SchemaRef schema, std::vector<ArrayRef> columns) {
        if (schema->num_fields() != columns.size())
            throw Error(RV_ERR_INVALID_ARG, "Schema has " + std::to_string(schema->num_fields()) + " fields but " +
                                                std::to_string(columns.size()) + " columns provided");
        const size_t rows = columns.empty() ? 0 : columns[0]->len();
        for (size_t i = 0; i < columns.size(); ++i)
            if (columns[i]->len() != rows)
                throw Error(RV_ERR_LENGTH_MISMATCH, "Column " + std::to_string(i) + " has length " + std::to_string(columns[i]->len()) +
                                                        " but expected " + std::to_string(rows));
        for (size_t i = 0; i < columns.size(); ++i)
            if (schema->field(i).data_type() != columns[i]->data_type())
                throw Error(RV_ERR_TYPE_MISMATCH, "Column " + std::to_string(i) + " has type " + to_string(columns[i]->data_type()) +
                                                      " but schema expects " + to_string(schema->field(i).data_type()));
        return RecordBatch(std::move(schema), std::move(columns), rows);
    }
    static RecordBatch new_unchecked(SchemaRef schema, std::vector<ArrayRef> columns, size_t num_rows) {
        return RecordBatch(std::move(schema), std::move(columns), num_rows);
    }
    const SchemaRef &schema() const { return schema_; }
    size_t num_rows() const { return num_rows_; }
    size_t num_columns() const { return columns_.size(); }
    const ArrayRef &column(size_t i) const {
        if (i >= columns_.size()) throw Panic("index out of bounds");
        return columns_[i];
    }
    const ArrayRef *column_by_name(const std::string &n) const {
        auto i = schema_->index_of(n);
        return i ? &columns_[*i] : nullptr;
    }
    const std::vector<ArrayRef> &columns() const { return columns_; }
    bool is_empty() const { return num_rows_ == 0; }

    RecordBatch slice(size_t offset, size_t length) const {  // :92-106
        if (offset + length > num_rows_) throw Panic("Slice out of bounds");
        std::vector<ArrayRef> cols;
        for (auto &c : columns_) cols.push_back(c->slice(offset, length));
        return RecordBatch(schema_, std::move(cols), length);
    }
    RecordBatch select_columns(const std::vector<size_t> &indices) const {  // :180-206
        for (size_t i : indices)
            if (i >= num_columns())
                throw Error(RV_ERR_OUT_OF_BOUNDS, "Column index " + std::to_string(i) + " out of bounds for " + std::to_string(num_columns()) + " columns");
        std::vector<Field> f;
        std::vector<ArrayRef> c;
        for (size_t i : indices) {
            f.push_back(schema_->field(i));
            c.push_back(columns_[i]);
        }
        return RecordBatch(std::make_shared<Schema>(f), std::move(c), num_rows_);
    }
    RecordBatch select_columns_by_name(const std::vector<std::string> &names) const {  // :208-219
        std::vector<size_t> idx;
        for (auto &n : names) {
            auto i = schema_->index_of(n);
            if (!i) throw Error(RV_ERR_INVALID_ARG, "Column '" + n + "' not found");
            idx.push_back(*i);
        }
        return select_columns(idx);
    }
    // record_batch.rs:221-243 -> rv_filter (one fused device pass per group of columns)
    RecordBatch filter(const ArrayRef &predicate) const {
        if (predicate->len() != num_rows_)
            throw Error(RV_ERR_LENGTH_MISMATCH, "Predicate length " + std::to_string(predicate->len()) + " doesn't match batch length " + std::to_string(num_rows_));
        if (predicate->data_type() != DataType::Boolean) throw Error(RV_ERR_TYPE_MISMATCH, "Predicate must be a BooleanArray");
        auto handles = device_handles("filter");
        std::vector<rv_dcolumn *> out(columns_.size(), nullptr);
        uint64_t rows = 0;
        check(rv_filter(predicate->context()->raw(), handles.data(), static_cast<uint32_t>(handles.size()), predicate->handle(), out.data(), &rows));
        return adopt_all(predicate->context(), out, rows);
    }
    // record_batch.rs:108-129 -> rv_take
    RecordBatch take(const std::vector<size_t> &indices) const {
        for (size_t i : indices)
            if (i >= num_rows_) throw Error(RV_ERR_OUT_OF_BOUNDS, "Index " + std::to_string(i) + " out of bounds for " + std::to_string(num_rows_) + " rows");
        if (columns_.empty()) return RecordBatch(schema_, {}, indices.size());
        auto handles = device_handles("take");
        std::vector<uint64_t> idx(indices.begin(), indices.end());
        std::vector<rv_dcolumn *> out(columns_.size(), nullptr);
        check(rv_take(ctx()->raw(), handles.data(), static_cast<uint32_t>(handles.size()), idx.data(), idx.size(), out.data()));
        return adopt_all(ctx(), out, indices.size());
    }
    // record_batch.rs:245-275 -> rv_concat per column position
    static RecordBatch concat(const std::vector<RecordBatch> &batches) {
        if (batches.empty()) throw Error(RV_ERR_INVALID_ARG, "Cannot concatenate empty batch list");
        for (size_t i = 1; i < batches.size(); ++i)
            if (*batches[i].schema_ != *batches[0].schema_) throw Error(RV_ERR_TYPE_MISMATCH, "All batches must have the same schema");
        size_t total = 0;
        for (auto &b : batches) total += b.num_rows_;
        std::vector<ArrayRef> cols;
        for (size_t c = 0; c < batches[0].num_columns(); ++c) {
            std::vector<const rv_dcolumn *> parts;
            for (auto &b : batches) {
                if (!b.columns_[c]->on_device()) throw Error(RV_ERR_UNSUPPORTED, "concat: String columns are outside the device path");
                parts.push_back(b.columns_[c]->handle());
            }
            rv_dcolumn *out = nullptr;
            check(rv_concat(batches[0].ctx()->raw(), parts.data(), static_cast<uint32_t>(parts.size()), &out));
            cols.push_back(Array::adopt(batches[0].ctx(), out));
        }
        return RecordBatch(batches[0].schema_, std::move(cols), total);
    }
    // record_batch.rs:402-421
    static RecordBatch empty(const ContextRef &ctx, SchemaRef schema) {
        std::vector<ArrayRef> cols;
        for (auto &f : schema->fields()) {
            switch (f.data_type()) {
                case DataType::Int64: cols.push_back(Int64Array::from_values(ctx, {})); break;
                case DataType::Float64: cols.push_back(Float64Array::from_values(ctx, {})); break;
                case DataType::Boolean: cols.push_back(BooleanArray::from_bools(ctx, {})); break;
                case DataType::String: cols.push_back(StringArray::create(ctx, {})); break;
                default: cols.push_back(NullArray::create(ctx, 0)); break;
            }
        }
        return RecordBatch(std::move(schema), std::move(cols), 0);
    }
    ContextRef ctx() const {
        for (auto &c : columns_)
            if (c->on_device()) return c->context();
        throw Error(RV_ERR_INVALID_ARG, "batch has no device column");
    }

  private:
    RecordBatch(SchemaRef s, std::vector<ArrayRef> c, size_t n) : schema_(std::move(s)), columns_(std::move(c)), num_rows_(n) {}
    std::vector<const rv_dcolumn *> device_handles(const char *what) const {
        return column_handles(columns_, std::string(what) + ": String columns are outside the device path");
    }
    RecordBatch adopt_all(const ContextRef &ctx, const std::vector<rv_dcolumn *> &out, size_t rows) const {
        return RecordBatch(schema_, adopt_columns(ctx, out), rows);
    }
    SchemaRef schema_;
    std::vector<ArrayRef> columns_;
    size_t num_rows_;
};

// ---------------------------------------------------------------------------------------
// streams -- stream.rs:7-213
// ---------------------------------------------------------------------------------------
struct StreamError : std::runtime_error {
    enum Kind { Execution, SchemaMismatch, Exhausted, Io } kind;
    std::string message;  // StreamError::Execution { message }
    StreamError(Kind k, const std::string &display, std::string msg = "") : std::runtime_error(display), kind(k), message(std::move(msg)) {}
    static StreamError execution(const std::string &m) { return StreamError(Execution, "Stream execution error: " + m, m); }
    static StreamError schema_mismatch() { return StreamError(SchemaMismatch, "Schema mismatch"); }
};

// the library's Error as a stream reports it (StreamError::Execution): the result of f(), or the translated error
template <class F>
auto stream_call(F &&f) -> decltype(f()) {
    try {
        return f();
    } catch (const Error &e) {
        throw StreamError::execution(e.what());
    }
}
inline void check_stream(rv_status st) {
    stream_call([&] { check(st); });
}

class DataStream {  // trait DataStream, stream.rs:25-54
  public:
    virtual ~DataStream() = default;
    virtual SchemaRef schema() const = 0;
    virtual std::optional<RecordBatch> next_batch() = 0;
    // Not in the reference's trait: a consumer that will take at most `rows` rows (LimitStream, streaming.rs:246-288) says
    // so once, before it pulls.  Row-preserving operators pass it on; the device operators size the window they filter
    // ahead by it instead of by their default of 2^28 rows.  A hint, never a contract: pulling past it still works.
    virtual void limit_hint(size_t /*rows*/) {}
    std::vector<RecordBatch> collect() {
        std::vector<RecordBatch> out;
        while (auto b = next_batch()) out.push_back(std::move(*b));
        return out;
    }
};
using DataStreamRef = std::unique_ptr<DataStream>;

class MemoryStream : public DataStream {  // stream.rs:58-114
  public:
    MemoryStream(SchemaRef schema, std::vector<RecordBatch> batches) : schema_(std::move(schema)), batches_(std::move(batches)) {
        for (auto &b : batches_)
            if (*b.schema() != *schema_) throw StreamError::schema_mismatch();
    }
    static std::unique_ptr<MemoryStream> from_single_batch(RecordBatch b) {
        auto s = b.schema();
        std::vector<RecordBatch> v;
        v.push_back(std::move(b));
        return std::make_unique<MemoryStream>(s, std::move(v));
    }
    static std::unique_ptr<MemoryStream> empty(SchemaRef s) { return std::make_unique<MemoryStream>(std::move(s), std::vector<RecordBatch>{}); }
    SchemaRef schema() const override { return schema_; }
    std::optional<RecordBatch> next_batch() override {
        if (index_ < batches_.size()) return batches_[index_++];
        return std::nullopt;
    }

  private:
    SchemaRef schema_;
    std::vector<RecordBatch> batches_;
    size_t index_ = 0;
};

// FilterStream -- stream.rs:116-163: predicate = a Boolean column of the batch
class FilterStream : public DataStream {
  public:
    FilterStream(DataStreamRef input, std::string predicate_column) : input_(std::move(input)), predicate_column_(std::move(predicate_column)) {}
    SchemaRef schema() const override { return input_->schema(); }
    std::optional<RecordBatch> next_batch() override {
        auto batch = input_->next_batch();
        if (!batch) return std::nullopt;
        auto idx = batch->schema()->index_of(predicate_column_);
        if (!idx) throw StreamError::execution("Column '" + predicate_column_ + "' not found in schema");
        const auto &pred = batch->column(*idx);
        if (pred->data_type() != DataType::Boolean) throw StreamError::execution("Predicate column '" + predicate_column_ + "' is not of boolean type");
        try {
            return batch->filter(pred);  // empty batches are still emitted (:156-158)
        } catch (const Error &e) {
            throw StreamError::execution(e.what());
        }
    }

  private:
    DataStreamRef input_;
    std::string predicate_column_;
};

class SelectStream : public DataStream {  // stream.rs:165-213
  public:
    SelectStream(DataStreamRef input, std::vector<std::string> column_names) : input_(std::move(input)), column_names_(std::move(column_names)) {
        auto in = input_->schema();
        std::vector<Field> f;
        for (auto &n : column_names_) {
            auto fld = in->field_by_name(n);
            if (!fld) throw StreamError::execution("Column '" + n + "' not found in schema");
            f.push_back(*fld);
        }
        output_schema_ = std::make_shared<Schema>(f);
    }
    SchemaRef schema() const override { return output_schema_; }
    void limit_hint(size_t rows) override { input_->limit_hint(rows); }  // a projection keeps every row
    std::optional<RecordBatch> next_batch() override {
        auto batch = input_->next_batch();
        if (!batch) return std::nullopt;
        try {
            return batch->select_columns_by_name(column_names_);
        } catch (const Error &e) {
            throw StreamError::execution(e.what());
        }
    }

  private:
    DataStreamRef input_;
    std::vector<std::string> column_names_;
    SchemaRef output_schema_;
};

class LimitStream : public DataStream {  // streaming.rs:246-288
  public:
    LimitStream(DataStreamRef input, size_t limit) : input_(std::move(input)), limit_(limit) { input_->limit_hint(limit_); }
    void limit_hint(size_t rows) override { input_->limit_hint(std::min(rows, limit_)); }
    SchemaRef schema() const override { return input_->schema(); }
    std::optional<RecordBatch> next_batch() override {
        if (rows_returned_ >= limit_) return std::nullopt;  // the device stops launching chunks here
        auto batch = input_->next_batch();
        if (!batch) return std::nullopt;
        const size_t remaining = limit_ - rows_returned_;
        if (batch->num_rows() <= remaining) {
            rows_returned_ += batch->num_rows();
            return batch;
        }
        rows_returned_ += remaining;
        return batch->slice(0, remaining);
    }

  private:
    DataStreamRef input_;
    size_t limit_, rows_returned_ = 0;
};

// One lowered compare term: batch column name <op> literal (planner.rs:134-189 grammar).
using Literal = std::variant<std::monostate, int64_t, double, bool, std::string>;  // AnyValue of a literal
// CsvFileStream -- file_stream.rs:10-336: schema-driven CSV scan into device RecordBatches.
// Split on the delimiter, trim, "" / "null" = null, first line is the header, blank lines skipped,
// batch_size rows per batch (default: calculate_adaptive_batch_size, :345-368).
//
// Null bitmaps of Int64 / Float64 columns: the reference hands its `nulls` flags (true = null) to
// PrimitiveArray::new, whose second argument is a VALIDITY vector (true = valid, primitive.rs:31-33), so
// there a column with a null comes out with every cell's validity inverted (file_stream.rs:213-249).
// CsvNulls::AsReference -- THE DEFAULT: this layer is a drop-in, and a drop-in gives the reference's arrays bit for
// bit, its defect included -- reproduces that; CsvNulls::AsIntended marks the null cells as null and must be asked
// for ("CSV nulls").  String and Boolean columns are right in the reference.
enum class CsvNulls { AsIntended, AsReference };
// Where the cells are parsed.  Host: one host core reads and parses every line, then each batch is uploaded.  Device: the
// file goes to HBM in pinned chunks and gfx950 kernels split and parse it (rv_csv_open / rv_csv_next): the same batches and
// the same errors, call by call.
enum class CsvScan { Host, Device };

inline size_t calculate_adaptive_batch_size(const Schema &schema) {  // file_stream.rs:345-368
    size_t row_bytes = 0;
    for (auto &f : schema.fields()) {
        switch (f.data_type()) {
            case DataType::Int64:
            case DataType::Float64: row_bytes += 8; break;
            case DataType::Boolean: row_bytes += 1; break;
            case DataType::String: row_bytes += 32; break;
            default: break;
        }
    }
    if (row_bytes == 0) return 10000;
    return std::min<size_t>(100000, std::max<size_t>(1000, (8u * 1024 * 1024) / row_bytes));
}

class CsvFileStream : public DataStream {
  public:
    // Err(String) of CsvFileStream::new (file_stream.rs:21-41) -> Error(RV_ERR_INVALID_ARG, same text)
    CsvFileStream(ContextRef ctx, const std::string &path, SchemaRef schema, std::optional<size_t> batch_size = std::nullopt,
                  std::optional<char> delimiter = std::nullopt, CsvNulls nulls = CsvNulls::AsReference, CsvScan scan = CsvScan::Host)
        : ctx_(std::move(ctx)), schema_(std::move(schema)), batch_size_(batch_size ? *batch_size : calculate_adaptive_batch_size(*schema_)),
          delimiter_(delimiter.value_or(',')), nulls_(nulls) {
        if (scan == CsvScan::Device) {  // rv_csv_open gives the same two errors, in the same order
            std::vector<rv_dtype> types;
            for (auto &f : schema_->fields()) types.push_back(to_rv(f.data_type()));
            check(rv_csv_open(ctx_->raw(), path.c_str(), types.data(), static_cast<uint32_t>(types.size()), static_cast<unsigned char>(delimiter_),
                              batch_size_, nulls_ == CsvNulls::AsReference ? RV_CSV_NULLS_AS_REFERENCE : 0u, 0, &reader_));
            return;
        }
        file_.open(path);
        if (!file_) throw Error(RV_ERR_INVALID_ARG, "Failed to open file: " + std::string(std::strerror(errno)));
        for (auto &f : schema_->fields())
            if (f.data_type() == DataType::Null) throw Error(RV_ERR_UNSUPPORTED, "Null columns are outside the device path");
    }
    ~CsvFileStream() override {
        if (reader_) rv_csv_close(reader_);
    }
    CsvFileStream(const CsvFileStream &) = delete;
    CsvFileStream &operator=(const CsvFileStream &) = delete;
    SchemaRef schema() const override { return schema_; }
    size_t batch_size() const { return batch_size_; }

    std::optional<RecordBatch> next_batch() override {  // read_batch, file_stream.rs:124-197
        if (reader_) return next_device_batch();
        if (finished_) return std::nullopt;
        const size_t ncols = schema_->num_fields();
        std::vector<std::vector<int64_t>> ints(ncols);
        std::vector<std::vector<double>> floats(ncols);
        std::vector<std::vector<std::optional<std::string>>> strings(ncols);
        std::vector<std::vector<std::optional<bool>>> bools(ncols);
        std::vector<std::vector<bool>> is_null(ncols);
        std::string line;
        if (current_line_ == 0) {  // header
            if (!std::getline(file_, line)) {
                finished_ = true;
                return std::nullopt;
            }
            ++current_line_;
        }
        size_t rows = 0;
        while (rows < batch_size_) {
            if (!std::getline(file_, line)) {
                finished_ = true;
                break;
            }
            ++current_line_;
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (trim(line).empty()) continue;
            parse_line(line, ints, floats, strings, bools, is_null);
            ++rows;
        }
        if (rows == 0) return std::nullopt;
        std::vector<ArrayRef> cols;  // build_record_batch, file_stream.rs:199-327
        for (size_t c = 0; c < ncols; ++c) {
            const bool any_null = std::find(is_null[c].begin(), is_null[c].end(), true) != is_null[c].end();
            auto validity = [&]() -> std::optional<std::vector<bool>> {
                if (!any_null) return std::nullopt;
                std::vector<bool> v(is_null[c].size());
                for (size_t i = 0; i < v.size(); ++i) v[i] = nulls_ == CsvNulls::AsReference ? is_null[c][i] : !is_null[c][i];
                return v;
            };
            switch (schema_->field(c).data_type()) {
                case DataType::Int64: cols.push_back(Int64Array::create(ctx_, ints[c], validity())); break;
                case DataType::Float64: cols.push_back(Float64Array::create(ctx_, floats[c], validity())); break;
                case DataType::String: cols.push_back(StringArray::create(ctx_, strings[c])); break;
                default: cols.push_back(BooleanArray::create(ctx_, bools[c])); break;
            }
        }
        try {
            return RecordBatch::try_new(schema_, std::move(cols));
        } catch (const Error &e) {
            throw StreamError::execution(std::string("Failed to create RecordBatch: ") + e.what());
        }
    }

  private:
    std::optional<RecordBatch> next_device_batch() {
        // batch size 0: read_batch gathers no row and every call is the end (rv_csv_open would take 0 for "adaptive")
        if (batch_size_ == 0) return std::nullopt;
        const size_t ncols = schema_->num_fields();
        std::vector<rv_dcolumn *> out(std::max<size_t>(ncols, 1), nullptr);
        uint64_t rows = 0;
        const rv_status s = rv_csv_next(reader_, out.data(), &rows);
        if (s == RV_ERR_PARSE) fail(rv_last_error());
        check(s);
        if (rows == 0) return std::nullopt;
        std::vector<ArrayRef> cols;
        for (size_t c = 0; c < ncols; ++c) cols.push_back(Array::adopt(ctx_, out[c]));
        try {
            return RecordBatch::try_new(schema_, std::move(cols));
        } catch (const Error &e) {
            throw StreamError::execution(std::string("Failed to create RecordBatch: ") + e.what());
        }
    }
    static std::string trim(const std::string &s) {
        size_t b = 0, e = s.size();
        while (b < e && std::isspace(static_cast<unsigned char>(s[b]))) ++b;
        while (e > b && std::isspace(static_cast<unsigned char>(s[e - 1]))) --e;
        return s.substr(b, e - b);
    }
    [[noreturn]] void fail(const std::string &what) const { throw StreamError::execution("Parse error: " + what); }
    void parse_line(const std::string &line, std::vector<std::vector<int64_t>> &ints, std::vector<std::vector<double>> &floats,
                    std::vector<std::vector<std::optional<std::string>>> &strings, std::vector<std::vector<std::optional<bool>>> &bools,
                    std::vector<std::vector<bool>> &is_null) const {  // file_stream.rs:43-122
        std::vector<std::string> fields;
        size_t start = 0;
        for (;;) {
            const size_t p = line.find(delimiter_, start);
            fields.push_back(trim(line.substr(start, p == std::string::npos ? std::string::npos : p - start)));
            if (p == std::string::npos) break;
            start = p + 1;
        }
        if (fields.size() != schema_->num_fields())
            fail("Line " + std::to_string(current_line_) + ": Expected " + std::to_string(schema_->num_fields()) + " fields, found " + std::to_string(fields.size()));
        // the row is appended only once every field has parsed (the reference returns before pushing anything)
        struct Cell {
            bool null = false;
            int64_t i = 0;
            double f = 0;
            bool b = false;
        };
        std::vector<Cell> cells(fields.size());
        for (size_t c = 0; c < fields.size(); ++c) {
            const std::string &f = fields[c];
            Cell &cell = cells[c];
            cell.null = f.empty() || f == "null";
            if (cell.null) continue;
            auto bad = [&](const char *type) { fail("Line " + std::to_string(current_line_) + ", field " + std::to_string(c) + ": Cannot parse '" + f + "' as " + type); };
            switch (schema_->field(c).data_type()) {
                case DataType::Int64: {  // str::parse::<i64>: optional sign, decimal digits only
                    size_t k = (f[0] == '+' || f[0] == '-') ? 1 : 0;
                    bool ok = k < f.size();
                    for (size_t q = k; q < f.size(); ++q) ok = ok && std::isdigit(static_cast<unsigned char>(f[q]));
                    errno = 0;
                    char *end = nullptr;
                    const long long v = ok ? std::strtoll(f.c_str(), &end, 10) : 0;
                    if (!ok || errno == ERANGE || *end) bad("Int64");
                    cell.i = v;
                    break;
                }
                case DataType::Float64: {  // str::parse::<f64>: decimal / exponent forms, inf, infinity, nan (any case); no hex
                    bool ok = true;
                    for (char ch : f) ok = ok && (std::isalnum(static_cast<unsigned char>(ch)) || ch == '+' || ch == '-' || ch == '.');
                    if (f.find_first_of("xXpP") != std::string::npos) ok = false;
                    char *end = nullptr;
                    const double v = ok ? std::strtod(f.c_str(), &end) : 0.0;
                    if (!ok || end == f.c_str() || *end) bad("Float64");
                    cell.f = v;
                    break;
                }
                case DataType::Boolean: {
                    std::string l = f;
                    for (auto &ch : l) ch = static_cast<char>(std::tolower(static_cast<unsigned char>(ch)));
                    if (l == "true" || l == "t" || l == "1") cell.b = true;
                    else if (l == "false" || l == "f" || l == "0") cell.b = false;
                    else bad("Boolean");
                    break;
                }
                default: break;
            }
        }
        for (size_t c = 0; c < fields.size(); ++c) {
            const Cell &cell = cells[c];
            is_null[c].push_back(cell.null);
            switch (schema_->field(c).data_type()) {
                case DataType::Int64: ints[c].push_back(cell.null ? 0 : cell.i); break;       // placeholder 0 (:218-221)
                case DataType::Float64: floats[c].push_back(cell.null ? 0.0 : cell.f); break;  // placeholder 0.0 (:246-249)
                case DataType::String: strings[c].push_back(cell.null ? std::nullopt : std::optional<std::string>(fields[c])); break;
                default: bools[c].push_back(cell.null ? std::nullopt : std::optional<bool>(cell.b)); break;
            }
        }
    }

    ContextRef ctx_;
    std::ifstream file_;
    SchemaRef schema_;
    size_t batch_size_;
    char delimiter_;
    CsvNulls nulls_;
    size_t current_line_ = 0;
    bool finished_ = false;
    rv_csv_reader *reader_ = nullptr;  // CsvScan::Device
};

struct CompareTerm {
    std::string column;
    rv_cmp op;
    Literal literal;  // monostate == Literal(AnyValue::Null); unused for RV_IS_TRUE
};

// A lowered predicate: compare terms + (for OR) the postfix program over them (rv_predicate::expr; empty: AND of
// the terms).  Converts from a plain term list, which is what AND-only call sites pass.
struct LoweredPredicate {
    std::vector<CompareTerm> terms;
    std::vector<uint8_t> expr;
    LoweredPredicate() = default;
    LoweredPredicate(std::vector<CompareTerm> t) : terms(std::move(t)) {}          // NOLINT: implicit on purpose
    LoweredPredicate(std::initializer_list<CompareTerm> t) : terms(t) {}            // NOLINT
};

inline rv_term to_rv_term(const CompareTerm &t, uint32_t column_index) {
    rv_term r{};
    r.column = column_index;
    r.op = t.op;
    switch (t.literal.index()) {
        case 0: r.lit_type = RV_NULL; break;
        case 1: r.lit_type = RV_INT64; r.lit.i = std::get<1>(t.literal); break;
        case 2: r.lit_type = RV_FLOAT64; r.lit.f = std::get<2>(t.literal); break;
        case 3: r.lit_type = RV_BOOLEAN; r.lit.i = std::get<3>(t.literal); break;
        default: {  // String literal: borrowed from the term for the duration of the call
            const std::string &str = std::get<4>(t.literal);
            r.lit_type = RV_STRING;
            r.lit.s.ptr = str.data();
            r.lit.s.len = str.size();
            break;
        }
    }
    return r;
}

// ---- arithmetic expressions (rv_eval_arith) ----------------------------------------------------------------------------
// One step of a postfix program over NAMED columns: what Expr::add / sub / mul / div trees are lowered to (expr.rs:44-74).
struct ArithStep {
    rv_arith_op op = RV_ARITH_COL;
    std::string column;  // RV_ARITH_COL
    Literal literal;     // RV_ARITH_LIT; monostate == Literal(AnyValue::Null)
    bool operator==(const ArithStep &o) const { return op == o.op && column == o.column && literal == o.literal; }
};
// One output column of a projection: a plain column of the input (`source`), or an arithmetic program over its columns.  Name and
// dtype are resolve_expr_schema's (logical_plan/plan.rs:204-233).
struct LoweredSelect {
    std::string name;
    DataType data_type = DataType::Null;
    std::string source;              // plain column: the input column it passes through
    std::vector<ArithStep> program;  // computed column
    bool computed() const { return !program.empty(); }
};
// `<arith> <cmp> <literal>` terms of a filter: every computed left side is a helper column appended to the batch, and the
// predicate is an ordinary one over the batch's columns and the helpers (rv_filter_project); the helpers never leave the filter.
struct ComputedPredicate {
    std::vector<LoweredSelect> helpers;
    LoweredPredicate predicate;
};

// The program's value over the columns `column(name)` finds (nullptr: the caller's `missing(name)` throws): one rv_eval_arith.
inline ArrayRef eval_arith(const std::vector<ArithStep> &program, const std::function<const ArrayRef *(const std::string &)> &column,
                           const std::function<void(const std::string &)> &missing) {
    std::vector<const rv_dcolumn *> cols;
    std::vector<std::string> names;
    std::vector<rv_arith_step> steps;
    ContextRef ctx;
    for (auto &s : program) {
        rv_arith_step r{};
        r.op = s.op;
        if (s.op == RV_ARITH_COL) {
            size_t k = 0;
            while (k < names.size() && names[k] != s.column) ++k;
            if (k == names.size()) {
                const ArrayRef *a = column(s.column);
                if (!a) missing(s.column);
                if (!a || !(*a)->on_device()) throw Error(RV_ERR_UNSUPPORTED, "columns off the device are outside the device path");
                if (!ctx) ctx = (*a)->context();
                names.push_back(s.column);
                cols.push_back((*a)->handle());
            }
            r.column = static_cast<uint32_t>(k);
        } else if (s.op == RV_ARITH_LIT) {
            switch (s.literal.index()) {
                case 0: r.lit_type = RV_NULL; break;
                case 1: r.lit_type = RV_INT64; r.lit.i = std::get<1>(s.literal); break;
                case 2: r.lit_type = RV_FLOAT64; r.lit.f = std::get<2>(s.literal); break;
                case 3: r.lit_type = RV_BOOLEAN; r.lit.i = std::get<3>(s.literal); break;  // refused by the library
                default: r.lit_type = RV_STRING; break;                                    // likewise
            }
        }
        steps.push_back(r);
    }
    if (!ctx) throw Error(RV_ERR_INVALID_ARG, "arithmetic expression reads no column");
    rv_dcolumn *out = nullptr;
    check(rv_eval_arith(ctx->raw(), cols.data(), static_cast<uint32_t>(cols.size()), steps.data(), static_cast<uint32_t>(steps.size()), &out));
    return Array::adopt(ctx, out);
}

// GpuProjectStream -- select([...]) with computed columns, batch by batch: a plain column passes through zero-copy (as
// SelectStream does, under the name the lowering gave it), a computed one is one rv_eval_arith over the batch.  A projection
// keeps every row, so a consumer's limit_hint goes on to the input.
class GpuProjectStream : public DataStream {
  public:
    GpuProjectStream(DataStreamRef input, std::vector<LoweredSelect> outputs) : input_(std::move(input)), outputs_(std::move(outputs)) {
        auto in = input_->schema();
        auto need = [&](const std::string &n) -> const Field & {
            auto fld = in->field_by_name(n);
            if (!fld) throw StreamError::execution("Column '" + n + "' not found in schema");
            return *fld;
        };
        std::vector<Field> f;
        for (auto &o : outputs_) {
            if (!o.computed()) {
                const Field &src = need(o.source);
                f.push_back(Field{o.name, src.data_type(), src.is_nullable()});
                continue;
            }
            for (auto &s : o.program)
                if (s.op == RV_ARITH_COL) need(s.column);
            f.push_back(Field{o.name, o.data_type, true});
        }
        output_schema_ = std::make_shared<Schema>(f);
    }
    SchemaRef schema() const override { return output_schema_; }
    void limit_hint(size_t rows) override { input_->limit_hint(rows); }
    std::optional<RecordBatch> next_batch() override {
        auto batch = input_->next_batch();
        if (!batch) return std::nullopt;
        auto missing = [](const std::string &n) { throw StreamError::execution("Column '" + n + "' not found in schema"); };
        auto column = [&](const std::string &n) { return batch->column_by_name(n); };
        std::vector<ArrayRef> arrays;
        for (auto &o : outputs_) {
            if (o.computed()) {
                arrays.push_back(stream_call([&] { return eval_arith(o.program, column, missing); }));
            } else {
                const ArrayRef *a = column(o.source);
                if (!a) missing(o.source);
                arrays.push_back(*a);
            }
        }
        return RecordBatch::new_unchecked(output_schema_, std::move(arrays), batch->num_rows());
    }

  private:
    DataStreamRef input_;
    std::vector<LoweredSelect> outputs_;
    SchemaRef output_schema_;
};

// Per-batch survivor counts in memory the device can write (rv_host_alloc): rv_filter_project_chunked then lets the fused
// pass drop the counts there itself -- 8 bytes per batch cross PCIe once and the host copies nothing.
class PinnedCounts {
  public:
    PinnedCounts() = default;
    PinnedCounts(const PinnedCounts &) = delete;
    PinnedCounts &operator=(const PinnedCounts &) = delete;
    ~PinnedCounts() { release(); }
    uint64_t *reserve(const ContextRef &ctx, size_t n) {
        if (n > cap_ || ctx != ctx_) {
            release();
            void *p = nullptr;
            check(rv_host_alloc(ctx->raw(), std::max<size_t>(n, 1024) * 8, &p));
            ptr_ = static_cast<uint64_t *>(p);
            cap_ = std::max<size_t>(n, 1024);
            ctx_ = ctx;
        }
        return ptr_;
    }
    uint64_t operator[](size_t i) const { return ptr_[i]; }
    void swap(PinnedCounts &o) {
        std::swap(ptr_, o.ptr_);
        std::swap(cap_, o.cap_);
        std::swap(ctx_, o.ctx_);
    }

  private:
    void release() {
        if (ptr_) rv_host_free(ctx_->raw(), ptr_);
        ptr_ = nullptr;
        cap_ = 0;
    }
    ContextRef ctx_;
    uint64_t *ptr_ = nullptr;
    size_t cap_ = 0;
};

// How many input rows a device stream filters ahead when its consumer has announced a limit (DataStream::limit_hint):
// the survivors still owed divided by the selectivity seen so far (before the first window: the context's last fused
// launch, else 1 in 256), with a margin, and at least twice the previous window after a window that fell short.
class LimitWindow {
  public:
    void hint(size_t rows) { hint_ = hint_ ? std::min(*hint_, rows) : rows; }
    // rows to scan next, at most `cap`
    size_t next(const ContextRef &ctx, size_t cap) {
        if (!hint_ || survivors_ >= *hint_) return cap;  // no limit known / already met: the default window
        double sel = scanned_ ? std::max(static_cast<double>(survivors_) / static_cast<double>(scanned_), 1e-7) : 1.0 / 256;
        if (!scanned_) {
            int64_t ppm = -1;
            if (rv_ctx_get_option(ctx->raw(), "last_selectivity_ppm", &ppm) == RV_OK && ppm > 0) sel = std::max(1e-6 * static_cast<double>(ppm), 1e-7);
        }
        double want = static_cast<double>(*hint_ - survivors_) / sel * 1.5 + 1024.0;
        want = std::max(want, 2.0 * static_cast<double>(last_));
        const size_t rows = want >= static_cast<double>(cap) ? cap : static_cast<size_t>(want);
        return std::max<size_t>(1, rows);
    }
    void record(size_t scanned, size_t survivors) {
        last_ = scanned;
        scanned_ += scanned;
        survivors_ += survivors;
    }
    size_t scanned() const { return scanned_; }
    bool hinted() const { return hint_.has_value(); }

  private:
    std::optional<size_t> hint_;
    size_t scanned_ = 0, survivors_ = 0, last_ = 0;
};

// GpuFilterProjectStream -- SelectStream(FilterStream(input)) fused, the operator behind seam S1 (INTEGRATION.md
// section 3).  The reference pulls 1024-row batches (streaming_planner.rs:32); a device launch per such batch would
// cost ~30 us for ~10 ns of work, so the operator pulls a WINDOW of input batches ahead (at most window_batches
// batches / window_rows rows), hands all of them to ONE rv_filter_project_batches call (one pass over HBM, one
// read-back of the per-batch row counts) and then emits the output batches one by one as zero-copy slices of the
// joint result -- batch for batch what FilterStream + SelectStream would have produced.
class GpuFilterProjectStream : public DataStream {
  public:
    GpuFilterProjectStream(DataStreamRef input, LoweredPredicate predicate, std::vector<std::string> projection,
                           rv_null_policy nulls = RV_NULL_DROPS, size_t window_batches = 4096, size_t window_rows = size_t(1) << 28)
        : input_(std::move(input)), terms_(std::move(predicate.terms)), expr_(std::move(predicate.expr)), projection_(std::move(projection)), nulls_(nulls),
          window_batches_(std::max<size_t>(1, window_batches)), window_rows_(window_rows) {
        auto in = input_->schema();
        std::vector<Field> f;
        for (auto &n : projection_) {
            auto fld = in->field_by_name(n);
            if (!fld) throw StreamError::execution("Column '" + n + "' not found in schema");
            f.push_back(*fld);
        }
        for (auto &t : terms_)
            if (!in->field_by_name(t.column)) throw StreamError::execution("Column '" + t.column + "' not found in schema");
        output_schema_ = std::make_shared<Schema>(f);
    }
    SchemaRef schema() const override { return output_schema_; }
    void limit_hint(size_t rows) override { limit_.hint(rows); }
    size_t rows_scanned() const { return limit_.scanned(); }

    std::optional<RecordBatch> next_batch() override {
        if (next_ready_ == ready_.size()) refill();
        if (next_ready_ < ready_.size()) return std::move(ready_[next_ready_++]);
        if (pending_error_) {  // raised by the call that would have returned the failing batch, as without the look-ahead
            auto e = pending_error_;
            pending_error_ = nullptr;
            std::rethrow_exception(e);
        }
        return std::nullopt;
    }

  private:
    void refill() {
        ready_.clear();
        next_ready_ = 0;
        if (exhausted_ || pending_error_) return;
        std::vector<RecordBatch> window;
        size_t rows = 0;
        size_t want_rows = window_rows_;  // under a limit: only as far ahead as the rows still owed need
        try {
            while (window.size() < window_batches_ && rows < want_rows) {
                auto b = input_->next_batch();
                if (!b) {
                    exhausted_ = true;
                    break;
                }
                if (window.empty() && b->num_columns() > 0) want_rows = limit_.next(b->ctx(), window_rows_);
                rows += b->num_rows();
                window.push_back(std::move(*b));
            }
        } catch (const StreamError &) {
            pending_error_ = std::current_exception();  // the batches pulled so far are still delivered first
            exhausted_ = true;
        }
        if (window.empty()) return;
        try {
            // device columns referenced by the predicate or the projection, each once (the same slots in every batch)
            const RecordBatch &first = window[0];
            std::vector<size_t> batch_index;
            auto slot_of = [&](const std::string &name) -> uint32_t {
                const size_t bi = *first.schema()->index_of(name);
                for (size_t k = 0; k < batch_index.size(); ++k)
                    if (batch_index[k] == bi) return static_cast<uint32_t>(k);
                batch_index.push_back(bi);
                return static_cast<uint32_t>(batch_index.size() - 1);
            };
            std::vector<rv_term> rt;
            for (auto &t : terms_) rt.push_back(to_rv_term(t, slot_of(t.column)));
            std::vector<uint32_t> proj;
            for (auto &n : projection_) proj.push_back(slot_of(n));
            const size_t ncols = batch_index.size(), nb = window.size(), np = proj.size();
            std::vector<const rv_dcolumn *> cols(nb * ncols);
            for (size_t b = 0; b < nb; ++b)
                for (size_t c = 0; c < ncols; ++c) cols[b * ncols + c] = window[b].column(batch_index[c])->handle();
            rv_predicate pred{rt.data(), static_cast<uint32_t>(rt.size()), nulls_, expr_.empty() ? nullptr : expr_.data(), static_cast<uint32_t>(expr_.size())};
            const ContextRef ctx = first.ctx();
            std::vector<rv_dcolumn *> out(np ? np : 1, nullptr);
            std::vector<uint64_t> out_rows(nb, 0);
            std::vector<int64_t> out_nulls(nb * (np ? np : 1), 0);
            uint64_t total = 0;
            check(rv_filter_project_batches(ctx->raw(), cols.data(), static_cast<uint32_t>(nb), static_cast<uint32_t>(ncols), &pred, proj.data(),
                                            static_cast<uint32_t>(np), out.data(), out_rows.data(), out_nulls.data(), &total));
            std::vector<ArrayRef> joined;
            for (size_t j = 0; j < np; ++j) joined.push_back(Array::adopt(ctx, out[j]));
            limit_.record(rows, total);
            uint64_t at = 0;
            for (size_t b = 0; b < nb; ++b) {  // every input batch yields its output batch, empty ones included (stream.rs:156-158)
                std::vector<ArrayRef> arrays;
                for (size_t j = 0; j < np; ++j) {
                    rv_dcolumn *piece = nullptr;
                    check(rv_slice_known(ctx->raw(), joined[j]->handle(), at, out_rows[b], out_nulls[b * np + j], &piece));
                    arrays.push_back(Array::adopt(ctx, piece));
                }
                ready_.push_back(RecordBatch::new_unchecked(output_schema_, std::move(arrays), out_rows[b]));
                at += out_rows[b];
            }
        } catch (const Error &e) {
            ready_.clear();
            pending_error_ = std::make_exception_ptr(StreamError::execution(e.what()));
        }
    }

    DataStreamRef input_;
    std::vector<CompareTerm> terms_;
    std::vector<uint8_t> expr_;
    std::vector<std::string> projection_;
    rv_null_policy nulls_;
    size_t window_batches_, window_rows_;
    SchemaRef output_schema_;
    std::vector<RecordBatch> ready_;
    size_t next_ready_ = 0;
    bool exhausted_ = false;
    std::exception_ptr pending_error_;
    LimitWindow limit_;
};

// GpuChunkedFilterProjectStream -- Select(Filter(DataFrameSource)) fused: the table stays whole in HBM and the library
// is told the batch size (rv_filter_project_chunked) instead of being handed one handle per 1024-row slice.  Emits
// exactly the batches SelectStream(FilterStream(MemoryStream(dataframe_to_batches(df, batch_size)))) would, one per input
// batch, empty ones included; `columns` are the frame's columns after dataframe_to_batches' null fill.
class GpuChunkedFilterProjectStream : public DataStream {
  public:
    GpuChunkedFilterProjectStream(std::vector<std::string> names, std::vector<ArrayRef> columns, size_t batch_size, LoweredPredicate predicate,
                                  std::vector<std::string> projection, rv_null_policy nulls = RV_NULL_DROPS, size_t window_rows = size_t(1) << 28)
        : names_(std::move(names)), columns_(std::move(columns)), batch_size_(batch_size), terms_(std::move(predicate.terms)),
          expr_(std::move(predicate.expr)), projection_(std::move(projection)), nulls_(nulls) {
        std::vector<Field> in;
        for (size_t c = 0; c < columns_.size(); ++c) in.push_back(Field{names_[c], columns_[c]->data_type(), true});
        Schema input_schema(in);
        std::vector<Field> f;
        for (auto &n : projection_) {
            auto fld = input_schema.field_by_name(n);
            if (!fld) throw StreamError::execution("Column '" + n + "' not found in schema");
            f.push_back(*fld);
        }
        for (auto &t : terms_)
            if (!input_schema.field_by_name(t.column)) throw StreamError::execution("Column '" + t.column + "' not found in schema");
        output_schema_ = std::make_shared<Schema>(f);
        rows_ = columns_.empty() ? 0 : columns_[0]->len();
        window_batches_ = std::max<size_t>(1, window_rows / std::max<size_t>(1, batch_size_));
        auto slot_of = [&](const std::string &name) -> uint32_t {
            const size_t ci = *input_schema.index_of(name);
            for (size_t k = 0; k < used_.size(); ++k)
                if (used_[k] == ci) return static_cast<uint32_t>(k);
            used_.push_back(ci);
            return static_cast<uint32_t>(used_.size() - 1);
        };
        for (auto &t : terms_) rt_.push_back(to_rv_term(t, slot_of(t.column)));
        for (auto &n : projection_) proj_.push_back(slot_of(n));
    }
    ~GpuChunkedFilterProjectStream() override {  // a window still in flight: waited for and dropped
        if (ahead_.pending) {
            std::vector<rv_dcolumn *> out(proj_.size() ? proj_.size() : 1, nullptr);
            rv_pending *pending = ahead_.pending;
            ahead_.pending = nullptr;
            if (rv_filter_project_window_finish(columns_[0]->context()->raw(), pending, out.data(), nullptr, nullptr) == RV_OK)
                for (size_t j = 0; j < proj_.size(); ++j) rv_free(columns_[0]->context()->raw(), out[j]);
        }
    }
    SchemaRef schema() const override { return output_schema_; }
    void limit_hint(size_t rows) override { limit_.hint(rows); }
    size_t rows_scanned() const { return limit_.scanned(); }

    std::optional<RecordBatch> next_batch() override {
        if (next_in_window_ == window_batches_out_) {
            if (next_row_ >= rows_ && !ahead_.pending) return std::nullopt;
            refill();
        }
        const size_t b = next_in_window_++, np = proj_.size();
        const ContextRef ctx = columns_[0]->context();
        std::vector<ArrayRef> arrays;
        for (size_t j = 0; j < np; ++j) {
            rv_dcolumn *piece = nullptr;
            check_stream(rv_slice_known(ctx->raw(), joined_[j]->handle(), at_, window_rows_out_[b], window_nulls_[b * np + j], &piece));
            arrays.push_back(Array::adopt(ctx, piece));
        }
        at_ += window_rows_out_[b];
        return RecordBatch::new_unchecked(output_schema_, std::move(arrays), window_rows_out_[b]);
    }

  private:
    // A window whose pass is queued on the device (rv_filter_project_chunked_begin): its views, predicate and count block stay put
    // until rv_filter_project_window_finish has consumed the pending handle.
    struct Ahead {
        rv_pending *pending = nullptr;
        std::vector<ArrayRef> views;
        std::vector<const rv_dcolumn *> cols;
        rv_predicate pred{};
        size_t len = 0, nb = 0;
    };
    void begin_window() {  // rows [next_row_, next_row_ + len): a whole number of batches
        const ContextRef ctx = columns_[0]->context();
        // under a limit (LimitStream told us how many rows it will take) only as far ahead as the rows still owed need
        const size_t want = limit_.next(ctx, window_batches_ * batch_size_);
        const size_t want_batches = std::max<size_t>(1, (want + batch_size_ - 1) / batch_size_);
        Ahead a;
        a.len = std::min(rows_ - next_row_, std::min(window_batches_, want_batches) * batch_size_);
        a.nb = (a.len + batch_size_ - 1) / batch_size_;
        for (size_t c : used_) {
            a.views.push_back(columns_[c]->slice(next_row_, a.len));
            a.cols.push_back(a.views.back()->handle());
        }
        a.pred = rv_predicate{rt_.data(), static_cast<uint32_t>(rt_.size()), nulls_, expr_.empty() ? nullptr : expr_.data(), static_cast<uint32_t>(expr_.size())};
        ahead_ = std::move(a);
        uint64_t *rows_out = next_rows_out_.reserve(ctx, ahead_.nb);  // pinned: written by the device (PinnedCounts)
        check_stream(rv_filter_project_chunked_begin(ctx->raw(), ahead_.cols.data(), static_cast<uint32_t>(ahead_.cols.size()), batch_size_, &ahead_.pred, proj_.data(),
                                                     static_cast<uint32_t>(proj_.size()), rows_out, ahead_.nb, &ahead_.pending));
        next_row_ += ahead_.len;
    }
    void refill() {  // the next window of the table
        const ContextRef ctx = columns_[0]->context();
        const size_t np = proj_.size();
        const size_t row_before = next_row_;
        if (!ahead_.pending) {
            try {
                begin_window();
            } catch (...) {
                next_row_ = row_before;  // a failed refill leaves the stream where it was (next_batch() raises again)
                throw;
            }
        }
        std::vector<rv_dcolumn *> out(np ? np : 1, nullptr);
        // filled in locals and committed only when the call succeeded
        std::vector<int64_t> nulls_out(ahead_.nb * (np ? np : 1), 0);
        uint64_t total = 0;
        rv_pending *pending = ahead_.pending;
        ahead_.pending = nullptr;  // finish consumes it, also on error
        const rv_status st = rv_filter_project_window_finish(ctx->raw(), pending, out.data(), nulls_out.data(), &total);
        if (st != RV_OK) {
            next_row_ -= ahead_.len;
            check_stream(st);
        }
        joined_.clear();
        for (size_t j = 0; j < np; ++j) joined_.push_back(Array::adopt(ctx, out[j]));
        window_rows_out_.swap(next_rows_out_);
        window_batches_out_ = ahead_.nb;
        window_nulls_ = std::move(nulls_out);
        limit_.record(ahead_.len, total);
        next_in_window_ = 0;
        at_ = 0;
        // Two windows in flight (stream.rs:25-28: the consumer pulls batch by batch): the next window's pass is queued now and runs
        // while this window's batches are handed on -- the device does not wait for the host between windows.  Not under a limit:
        // how far to look ahead then follows from what this window kept.
        if (next_row_ < rows_ && !limit_.hinted()) {
            try {
                begin_window();
            } catch (...) {  // reported by the refill that needs the window
                ahead_.pending = nullptr;
            }
        }
    }

    std::vector<std::string> names_;
    std::vector<ArrayRef> columns_;
    size_t batch_size_;
    std::vector<CompareTerm> terms_;
    std::vector<uint8_t> expr_;
    std::vector<std::string> projection_;
    rv_null_policy nulls_;
    SchemaRef output_schema_;
    std::vector<size_t> used_;  // frame columns the predicate or the projection reads, each once
    std::vector<rv_term> rt_;
    std::vector<uint32_t> proj_;
    size_t rows_ = 0, next_row_ = 0, window_batches_ = 1;
    std::vector<ArrayRef> joined_;  // the current window's outputs, all its batches back to back
    PinnedCounts window_rows_out_, next_rows_out_;  // the current window's per-batch counts / the block the next refill fills
    size_t window_batches_out_ = 0;
    std::vector<int64_t> window_nulls_;
    size_t next_in_window_ = 0;
    uint64_t at_ = 0;
    LimitWindow limit_;
    Ahead ahead_;
};

// String join keys.  The join kernels take 64 key bits per cell, so a String key column is reduced to an Int64 ids column by the
// device string dictionary (rv_string_dict_build / rv_string_dict_encode) and the Int64 join runs on the ids, unchanged:
//   - both keys String: the dictionary is built ONCE over the build key, whose ids stand in for it (the build key never reaches
//     the output); every probe frame / window / batch has its key encoded against the dictionary into a HELPER column that rides
//     along as one more probe column and is the key -- the caller drops that one output column afterwards.  Equal strings meet,
//     null meets null, an absent string (-1) meets nothing;
//   - one key String, the other not: the reference pairs null to null only (values of different AnyValue variants never compare
//     equal, series.rs:85-97).  The String side is encoded against an EMPTY dictionary -- its nulls stay nulls -- and handed to
//     the join under a dtype that differs from the other side's (re-wrapped as Float64 when that is Int64), so only the nulls meet;
//   - neither key String: inactive, the join runs as it always did.
class StringKeyEncoder {
  public:
    StringKeyEncoder(DataType build, DataType probe) : build_(build), probe_(probe) {}
    ~StringKeyEncoder() {
        if (dict_) rv_string_dict_free(dict_ctx_->raw(), dict_);
    }
    StringKeyEncoder(const StringKeyEncoder &) = delete;
    StringKeyEncoder &operator=(const StringKeyEncoder &) = delete;
    bool active() const { return build_ == DataType::String || probe_ == DataType::String; }
    bool probe_helper() const { return probe_ == DataType::String; }  // the probe side gets a helper column, which is its key

    // what the join hashes in place of the build key (call once, before any probe_key); nullptr: the build key itself
    ArrayRef build_key(const ArrayRef &key) {
        if (build_ != DataType::String) return nullptr;
        const ContextRef &ctx = key->context();
        if (probe_ != DataType::String) return differing(ctx, encode(ctx, key), probe_);
        rv_dcolumn *ids = nullptr;
        check(rv_string_dict_build(ctx->raw(), key->handle(), &dict_, &ids));
        dict_ctx_ = ctx;
        return Array::adopt(ctx, ids);
    }
    // the helper column of one probe frame / window / batch; nullptr: the probe key itself
    ArrayRef probe_key(const ContextRef &ctx, const ArrayRef &key) {
        if (probe_ != DataType::String) return nullptr;
        ArrayRef ids = encode(ctx, key);
        return build_ == DataType::String ? ids : differing(ctx, ids, build_);
    }

  private:
    // the ids of `key` against the dictionary (an empty one when only one side is String: built on first use)
    ArrayRef encode(const ContextRef &ctx, const ArrayRef &key) {
        if (!dict_) {
            ArrayRef none = NullArray::create(ctx, 0);
            check(rv_string_dict_build(ctx->raw(), none->handle(), &dict_, nullptr));
            dict_ctx_ = ctx;
        }
        rv_dcolumn *ids = nullptr;
        check(rv_string_dict_encode(ctx->raw(), dict_, key->handle(), &ids));
        return Array::adopt(ctx, ids);
    }
    // an ids column whose buffers are read as Float64: a view that keeps the ids alive
    class Float64View : public Array {
      public:
        Float64View(ContextRef ctx, rv_dcolumn *h, ArrayRef owner) : Array(std::move(ctx), h), owner_(std::move(owner)) {}

      private:
        ArrayRef owner_;
    };
    // `ids` (Int64) under a dtype other than `other`
    static ArrayRef differing(const ContextRef &ctx, ArrayRef ids, DataType other) {
        if (other != DataType::Int64) return ids;
        rv_column c{};
        check(rv_device_ptrs(ctx->raw(), ids->handle(), &c));
        c.dtype = RV_FLOAT64;
        rv_dcolumn *h = nullptr;
        check(rv_wrap(ctx->raw(), &c, &h));
        return std::make_shared<const Float64View>(ctx, h, std::move(ids));
    }
    DataType build_, probe_;
    rv_string_dict *dict_ = nullptr;
    ContextRef dict_ctx_;
};

// The helper column around one join call.  with_key_helper: the probe handles with the helper (if any) appended as the key.
struct ProbeColumns {
    std::vector<const rv_dcolumn *> cols;
    uint32_t key = 0;
    std::optional<size_t> helper_at;  // the helper's place among the probe columns, which is its place among the outputs
};
inline ProbeColumns with_key_helper(std::vector<const rv_dcolumn *> probe, uint32_t key, const ArrayRef &helper) {
    ProbeColumns p{std::move(probe), key, std::nullopt};
    if (helper) {
        p.helper_at = p.cols.size();
        p.key = static_cast<uint32_t>(p.cols.size());
        p.cols.push_back(helper->handle());
    }
    return p;
}
// counts[batches][ncols], row-major, without column `at`: [batches][ncols - 1]
inline void drop_count_column(std::vector<int64_t> &counts, size_t batches, size_t ncols, size_t at) {
    size_t w = 0;
    for (size_t k = 0; k < batches; ++k)
        for (size_t j = 0; j < ncols; ++j)
            if (j != at) counts[w++] = counts[k * ncols + j];
    counts.resize(w);
}
// ... and out again: the helper's output column and, where null counts were asked for, its entry in each batch's row of counts
inline void without_key_helper(const ProbeColumns &p, std::vector<ArrayRef> &out, std::vector<int64_t> *nulls = nullptr, size_t batches = 0) {
    if (!p.helper_at) return;
    if (nulls) drop_count_column(*nulls, batches, out.size(), *p.helper_at);
    out.erase(out.begin() + static_cast<long>(*p.helper_at));
}

// The join types of the plans.  The reference has Inner alone (logical_plan/plan.rs: //Left, //Outer) and makes the LEFT frame the
// build side (planner.rs:102-108).  Inner, Right and Outer keep that: Right is rv_join_kind PROBE_OUTER, Outer FULL_OUTER.  For
// Left, Semi and Anti the plan SWAPS the sides -- the left frame probes a table built on the right frame -- so that Left is
// PROBE_OUTER with the left frame's columns first, and Semi / Anti keep (drop) the left frame's rows that have a partner.
enum class JoinType { Inner, Left, Right, Outer, Semi, Anti };
struct JoinShape {
    rv_join_kind kind;
    bool swapped;  // the left frame is the probe side
};
inline JoinShape join_shape(JoinType t) {
    switch (t) {
        case JoinType::Inner: return {RV_JOIN_INNER, false};
        case JoinType::Right: return {RV_JOIN_PROBE_OUTER, false};
        case JoinType::Outer: return {RV_JOIN_FULL_OUTER, false};
        case JoinType::Left: return {RV_JOIN_PROBE_OUTER, true};
        case JoinType::Semi: return {RV_JOIN_PROBE_SEMI, true};
        case JoinType::Anti: return {RV_JOIN_PROBE_ANTI, true};
    }
    throw Panic("unreachable");
}

// materialize_join_result (plan.rs:212-255): every probe field, then every build field but the key, `_right` on a name the probe
// side has too.  The other kinds: FULL_OUTER keeps the build key at its place (under the same rule: `_right` when the probe side
// has the name, as it does for equally named keys); a semi or anti join has the probe fields only.  A side that can lack a partner
// is nullable.
inline std::vector<Field> join_output_fields(const Schema &probe, const Schema &build, size_t build_key, rv_join_kind kind = RV_JOIN_INNER) {
    std::vector<Field> f;
    for (const Field &p : probe.fields()) f.push_back(kind == RV_JOIN_FULL_OUTER ? Field{p.name(), p.data_type(), true} : p);
    if (kind == RV_JOIN_PROBE_SEMI || kind == RV_JOIN_PROBE_ANTI) return f;
    const bool partial = kind == RV_JOIN_PROBE_OUTER || kind == RV_JOIN_FULL_OUTER;
    for (size_t i = 0; i < build.num_fields(); ++i) {
        const Field &b = build.field(i);
        if (i != build_key || kind == RV_JOIN_FULL_OUTER)
            f.push_back(Field{probe.field_by_name(b.name()) ? b.name() + "_right" : b.name(), b.data_type(), partial || b.is_nullable()});
    }
    return f;
}
// FULL_OUTER with a String build key: the ids stand in for the key inside the table, but the key column of the result must be the
// strings.  The original key rides along as one more build column (the last) and takes the ids column's place among the outputs:
// `out` = n_probe probe columns (a key helper included), then the build columns, then the carried key.
inline void restore_build_key(std::vector<ArrayRef> &out, size_t n_probe, size_t build_key) {
    out[n_probe + build_key] = out.back();
    out.pop_back();
}

// The schema of a frame of named columns: every field nullable, as dataframe_to_batches declares them.
inline SchemaRef nullable_schema(const std::vector<std::string> &names, const std::vector<ArrayRef> &columns) {
    std::vector<Field> f;
    for (size_t c = 0; c < columns.size(); ++c) f.push_back(Field{names[c], columns[c]->data_type(), true});
    return std::make_shared<const Schema>(f);
}

// One side of a streaming join, or the input of a pipeline breaker (StreamingPhysicalPlan::as_input): a stream, or a resident frame
// (a DataFrameSource: its columns after dataframe_to_batches' null fill, cut into batch_size-row batches).
struct JoinSide {
    DataStreamRef stream;
    std::vector<std::string> names;
    std::vector<ArrayRef> columns;
    size_t batch_size = 0;
    SchemaRef schema() const { return stream ? stream->schema() : nullable_schema(names, columns); }
};

// GpuHashJoinStream -- StreamingPhysicalPlan::HashJoin (the reference's arm is todo!(), streaming.rs:128-131), for the inner join and
// the probe-preserving kinds PROBE_OUTER, PROBE_SEMI and PROBE_ANTI (rv_hash_join_chunked_kind; a full outer join is refused), defined by
// the eager join: the build side is drained once (one batch as it is, several joined by RecordBatch::concat) and hashed
// (rv_join_build); then EXACTLY one output batch per probe batch, empty ones included, in probe order, each == rv_hash_join of
// the whole build side against that probe batch alone -- names, `_right` suffixes, row order and key rules of the eager join.
//   - a resident probe frame: one rv_hash_join_chunked per WINDOW of window_rows rows (2^28 by default, as the filter streams: one
//     window for most tables, and a launch plus a read-back per window is noise at that size); the output batches are
//     rv_slice_known views of the window's outputs.  max_pairs (2^28 by default: 4 GiB of pair indices plus the gathered columns)
//     bounds what one window materialises: a join larger than HBM streams through windows cut short at their out_batches, each
//     window starting at the first batch the one before did not take;
//   - any other probe stream (CSV, MemoryStream, a filter): one rv_hash_join_chunked per pulled batch against the same table.
//     Correct, but launch-bound like every per-batch device call (about five launches, a read-back and a wait per batch).
// Under a limit (limit_hint) windows are sized by LimitWindow with the pairs counted as its survivors: limit(10) probes a few
// thousand rows, not the table.
class GpuHashJoinStream : public DataStream {
  public:
    GpuHashJoinStream(JoinSide build, JoinSide probe, std::string build_key, std::string probe_key, size_t window_rows = size_t(1) << 28,
                      uint64_t max_pairs = uint64_t(1) << 28, rv_join_kind kind = RV_JOIN_INNER)
        : build_(std::move(build)), probe_(std::move(probe)), build_key_(std::move(build_key)), probe_key_(std::move(probe_key)),
          window_rows_(std::max<size_t>(1, window_rows)), max_pairs_(max_pairs), kind_(kind) {
        if (kind_ == RV_JOIN_FULL_OUTER)
            throw Error(RV_ERR_UNSUPPORTED, "GpuHashJoinStream: a full outer join is not streamed (its unmatched build rows belong to no probe batch); "
                                            "use the eager plan, PhysicalPlan::hash_join");
        build_schema_ = build_.schema();
        probe_schema_ = probe_.schema();
        auto bk = build_schema_->index_of(build_key_);
        if (!bk) throw StreamError::execution("Column '" + build_key_ + "' not found in schema");
        auto pk = probe_schema_->index_of(probe_key_);
        if (!pk) throw StreamError::execution("Column '" + probe_key_ + "' not found in schema");
        bki_ = static_cast<uint32_t>(*bk);
        pki_ = static_cast<uint32_t>(*pk);
        output_schema_ = std::make_shared<const Schema>(join_output_fields(*probe_schema_, *build_schema_, bki_, kind_));
        string_keys_ = std::make_unique<StringKeyEncoder>(build_schema_->field(bki_).data_type(), probe_schema_->field(pki_).data_type());
        probe_rows_ = probe_.stream ? 0 : (probe_.columns.empty() ? 0 : probe_.columns[0]->len());
    }
    ~GpuHashJoinStream() override {
        if (table_) rv_join_table_free(table_ctx_->raw(), table_);
    }
    SchemaRef schema() const override { return output_schema_; }
    void limit_hint(size_t rows) override { limit_.hint(rows); }  // counted in pairs: not passed on to the probe side
    size_t rows_scanned() const { return limit_.scanned(); }

    std::optional<RecordBatch> next_batch() override {
        if (probe_.stream) return next_pulled();
        if (next_in_window_ == window_rows_out_.size()) {
            if (next_row_ >= probe_rows_) return std::nullopt;
            refill();
        }
        const size_t b = next_in_window_++, nout = joined_.size();
        const ContextRef &ctx = probe_.columns[0]->context();
        std::vector<ArrayRef> arrays;
        for (size_t j = 0; j < nout; ++j) {
            rv_dcolumn *piece = nullptr;
            check_stream(rv_slice_known(ctx->raw(), joined_[j]->handle(), at_, window_rows_out_[b], window_nulls_[b * nout + j], &piece));
            arrays.push_back(Array::adopt(ctx, piece));
        }
        at_ += window_rows_out_[b];
        return RecordBatch::new_unchecked(output_schema_, std::move(arrays), window_rows_out_[b]);
    }

  private:
    // the build side drained and hashed, once (ctx: the probe side's, for a build side that yields no batch)
    void ensure_built(const ContextRef &ctx) {
        if (table_) return;
        stream_call([&] {
            if (build_.stream) {
                std::vector<RecordBatch> parts = build_.stream->collect();
                RecordBatch whole = parts.empty() ? RecordBatch::empty(ctx, build_schema_) : parts.size() == 1 ? std::move(parts[0]) : RecordBatch::concat(parts);
                build_.columns = whole.columns();
            } else if (build_.columns.empty()) {
                build_.columns = RecordBatch::empty(ctx, build_schema_).columns();
            }
            for (auto &c : build_.columns) build_handles_.push_back(c->handle());
            table_ctx_ = build_.columns[bki_]->context();
            // a String build key: its ids stand in for it, in the table and among the columns (the key is never gathered)
            if ((build_key_ids_ = string_keys_->build_key(build_.columns[bki_]))) build_handles_[bki_] = build_key_ids_->handle();
            check(rv_join_build(table_ctx_->raw(), build_handles_[bki_], &table_));
        });
    }
    // rv_hash_join_chunked over the n rows of `probe` (columns `arrays`) in batches of `chunk`, into out / rows / nulls; returns the
    // batches taken.  A String probe key is encoded first: its ids ride along as one more probe column, which is the key, and that
    // column leaves the outputs and the null counts again.
    uint64_t join_window(const ContextRef &ctx, std::vector<const rv_dcolumn *> probe, const std::vector<ArrayRef> &arrays, uint64_t n, uint64_t chunk,
                         std::vector<ArrayRef> &out, std::vector<uint64_t> &rows, std::vector<int64_t> &nulls, uint64_t &pairs) {
        const ArrayRef helper = stream_call([&] { return string_keys_->probe_key(ctx, arrays[pki_]); });
        const ProbeColumns p = with_key_helper(std::move(probe), pki_, helper);
        const size_t nout = output_schema_->num_fields() + (helper ? 1 : 0);
        const uint64_t nb = (n + chunk - 1) / chunk;
        std::vector<rv_dcolumn *> raw(nout, nullptr);
        rows.assign(std::max<uint64_t>(nb, 1), 0);
        nulls.assign(std::max<uint64_t>(nb, 1) * nout, 0);
        uint64_t taken = 0;
        if (kind_ == RV_JOIN_INNER)
            check_stream(rv_hash_join_chunked(ctx->raw(), table_, build_handles_.data(), static_cast<uint32_t>(build_handles_.size()), bki_, p.cols.data(),
                                              static_cast<uint32_t>(p.cols.size()), p.key, chunk, max_pairs_, raw.data(), rows.data(), nb, nulls.data(), &pairs,
                                              &taken));
        else
            check_stream(rv_hash_join_chunked_kind(ctx->raw(), table_, build_handles_.data(), static_cast<uint32_t>(build_handles_.size()), bki_, p.cols.data(),
                                                   static_cast<uint32_t>(p.cols.size()), p.key, kind_, chunk, max_pairs_, raw.data(), rows.data(), nb,
                                                   nulls.data(), &pairs, &taken));
        out = adopt_columns(ctx, raw);
        rows.resize(taken);
        without_key_helper(p, out, &nulls, taken);
        return taken;
    }
    void refill() {  // the next window of the resident probe frame
        const ContextRef ctx = probe_.columns[0]->context();
        ensure_built(ctx);
        const size_t batch = probe_.batch_size;
        const size_t want = limit_.next(ctx, window_rows_);
        const size_t want_batches = std::max<size_t>(1, (want + batch - 1) / batch);
        const size_t cap_batches = std::max<size_t>(1, window_rows_ / batch);
        const size_t len = std::min(probe_rows_ - next_row_, std::min(cap_batches, want_batches) * batch);
        std::vector<ArrayRef> views;
        std::vector<const rv_dcolumn *> cols;
        for (auto &c : probe_.columns) {
            views.push_back(c->slice(next_row_, len));
            cols.push_back(views.back()->handle());
        }
        std::vector<ArrayRef> out;
        std::vector<uint64_t> rows;
        std::vector<int64_t> nulls;
        uint64_t pairs = 0;
        const uint64_t taken = join_window(ctx, cols, views, len, batch, out, rows, nulls, pairs);
        const size_t probed = std::min<size_t>(len, taken * batch);
        joined_ = std::move(out);
        window_rows_out_ = std::move(rows);
        window_nulls_ = std::move(nulls);
        next_in_window_ = 0;
        at_ = 0;
        next_row_ += probed;
        limit_.record(probed, pairs);
    }
    std::optional<RecordBatch> next_pulled() {  // one probe batch pulled, one call
        auto batch = probe_.stream->next_batch();
        if (!batch) return std::nullopt;
        const ContextRef ctx = batch_ctx(*batch);
        ensure_built(ctx);
        std::vector<const rv_dcolumn *> cols;
        for (auto &c : batch->columns()) cols.push_back(c->handle());
        std::vector<ArrayRef> out;
        std::vector<uint64_t> rows;
        std::vector<int64_t> nulls;
        uint64_t pairs = 0;
        join_window(ctx, cols, batch->columns(), batch->num_rows(), std::max<size_t>(1, batch->num_rows()), out, rows, nulls, pairs);
        limit_.record(batch->num_rows(), pairs);
        if (rows.empty()) return RecordBatch::new_unchecked(output_schema_, std::move(out), 0);  // a zero-row probe batch
        std::vector<ArrayRef> arrays;
        for (size_t j = 0; j < out.size(); ++j) {
            rv_dcolumn *piece = nullptr;
            check_stream(rv_slice_known(ctx->raw(), out[j]->handle(), 0, rows[0], nulls[j], &piece));
            arrays.push_back(Array::adopt(ctx, piece));
        }
        return RecordBatch::new_unchecked(output_schema_, std::move(arrays), rows[0]);
    }
    static ContextRef batch_ctx(const RecordBatch &b) {
        return stream_call([&] { return b.ctx(); });
    }

    JoinSide build_, probe_;
    std::string build_key_, probe_key_;
    size_t window_rows_;
    uint64_t max_pairs_;
    rv_join_kind kind_;
    SchemaRef build_schema_, probe_schema_, output_schema_;
    uint32_t bki_ = 0, pki_ = 0;
    rv_join_table *table_ = nullptr;
    ContextRef table_ctx_;
    std::vector<const rv_dcolumn *> build_handles_;
    std::unique_ptr<StringKeyEncoder> string_keys_;  // String keys go through the string dictionary
    ArrayRef build_key_ids_;                         // ... the ids that stand in for a String build key
    size_t probe_rows_ = 0, next_row_ = 0;
    std::vector<ArrayRef> joined_;  // the current window's outputs, all its batches back to back
    std::vector<uint64_t> window_rows_out_;
    std::vector<int64_t> window_nulls_;
    size_t next_in_window_ = 0;
    uint64_t at_ = 0;
    LimitWindow limit_;
};

// A PIPELINE BREAKER (group_by, sort, window, top_k): it drains its input and emits EXACTLY ONE batch.  This is the drain -- a resident
// frame is taken as it is, the batches of any other stream are concatenated (RecordBatch::concat), one batch alone is taken as it is --
// and run() is the operator's own step over the whole input.  An input that yields no batch at all gives one zero-row batch with the
// output schema.
class GpuBreakerStream : public DataStream {
  public:
    SchemaRef schema() const override { return schema_; }
    std::optional<RecordBatch> next_batch() override {
        if (done_) return std::nullopt;
        done_ = true;
        std::vector<ArrayRef> columns = input_.columns;
        if (input_.stream) {
            std::vector<RecordBatch> all;
            while (auto b = input_.stream->next_batch()) all.push_back(std::move(*b));
            if (all.empty()) return no_batch();
            RecordBatch whole = all.size() == 1 ? all[0] : stream_call([&] { return RecordBatch::concat(all); });
            columns = whole.columns();
        }
        return stream_call([&] { return run(ctx_of(columns), columns); });
    }

  protected:
    // `op`: the operator's name in the errors; `fallback_ctx`: where the zero-row batch of an input that yields no batch at all is
    // created.  The constructor of the operator sets schema_, which is where its planning errors come from.
    GpuBreakerStream(const char *op, JoinSide input, ContextRef fallback_ctx)
        : op_(op), input_(std::move(input)), ctx_(std::move(fallback_ctx)), input_schema_(input_.schema()) {}
    // the operator over the whole input (`columns` in the order of input_schema_), as its one batch
    virtual RecordBatch run(const ContextRef &ctx, const std::vector<ArrayRef> &columns) = 0;
    RecordBatch batch_of(std::vector<ArrayRef> out) const {
        const size_t rows = out[0]->len();
        return RecordBatch::new_unchecked(schema_, std::move(out), rows);
    }
    RecordBatch no_batch() const {
        if (!ctx_) throw StreamError::execution(std::string(op_) + ": the input yielded no batch and the plan holds no device context");
        return RecordBatch::empty(ctx_, schema_);
    }
    ContextRef ctx_of(const std::vector<ArrayRef> &columns) const { return columns.empty() ? ctx_ : columns[0]->context(); }

    const char *op_;
    JoinSide input_;
    ContextRef ctx_;
    SchemaRef input_schema_, schema_;
    bool done_ = false;
};

// ---------------------------------------------------------------------------------------
// group_by(key).agg([...]) -- the reference has no aggregate operator: include/rivulus_gpu.h, rv_hash_aggregate
// ---------------------------------------------------------------------------------------
enum class AggOp { CountRows, Count, Sum, Min, Max };  // rv_agg_op, in its order
inline const char *to_string(AggOp op) {
    static const char *n[] = {"COUNT(*)", "COUNT", "SUM", "MIN", "MAX"};
    return n[static_cast<int>(op)];
}
// One aggregate: `op` over `column` (ignored by CountRows), under the output name `name`.
struct AggSpec {
    AggOp op;
    std::string column;
    std::string name;
};
struct GroupByPlanError : std::runtime_error {  // what planning a group_by refuses, with the column it refuses it for
    using std::runtime_error::runtime_error;
};

// the aggregates' fields behind the key fields `out` (both forms of group_by_schema)
inline SchemaRef group_by_agg_fields(const Schema &in, std::vector<Field> out, const std::vector<AggSpec> &aggs) {
    if (aggs.empty()) throw GroupByPlanError("group_by: no aggregates");
    for (auto &a : aggs) {
        DataType t = DataType::Int64;
        if (a.op != AggOp::CountRows) {
            const Field *f = in.field_by_name(a.column);
            if (!f) throw GroupByPlanError("group_by: aggregate '" + a.name + "' reads the unknown column '" + a.column + "'");
            if (a.op != AggOp::Count) {
                t = f->data_type();
                if (t != DataType::Int64 && t != DataType::Float64)
                    throw GroupByPlanError(std::string("group_by: ") + to_string(a.op) + " over column '" + a.column + "' of dtype " + to_string(t));
            }
        }
        for (auto &f : out)
            if (f.name() == a.name) throw GroupByPlanError("group_by: duplicate output name '" + a.name + "'");
        out.push_back(Field{a.name, t, a.op == AggOp::Min || a.op == AggOp::Max});
    }
    return std::make_shared<const Schema>(out);
}

// The output schema of group_by(key).agg(aggs) over `in`: the key under its own name, then every aggregate under its name -- counts
// Int64, SUM / MIN / MAX of the column's dtype.  Throws GroupByPlanError for an unknown column, a duplicate output name, SUM / MIN /
// MAX over a column that is not Int64 or Float64, and a key the device does not group by (Float64, Boolean: not built).
inline SchemaRef group_by_schema(const Schema &in, const std::string &key, const std::vector<AggSpec> &aggs) {
    const Field *kf = in.field_by_name(key);
    if (!kf) throw GroupByPlanError("group_by: unknown key column '" + key + "'");
    if (kf->data_type() == DataType::Float64 || kf->data_type() == DataType::Boolean)
        throw GroupByPlanError("group_by: key column '" + key + "' is " + to_string(kf->data_type()) + "; only Int64 and String keys are grouped");
    std::vector<Field> out{Field{key, kf->data_type(), true}};
    return group_by_agg_fields(in, std::move(out), aggs);
}

// group_by over a LIST of key columns (rv_hash_aggregate_keys): the keys first, in the order given and under their own names, each
// nullable and of its own dtype -- Int64, Float64, Boolean, String and Null keys are all grouped -- then the aggregates.  A row's key is
// the tuple of its cells; a Float64 key groups every NaN together and keeps -0.0 and +0.0 apart (the equality the sort's order
// induces), a null cell equals only a null cell of the same column.  The list with ONE name is how a Float64 or Boolean key is
// grouped.  Throws GroupByPlanError for an empty key list, an unknown key, a key named twice, more than 8 keys, an aggregate name that
// collides with a key, and what the aggregates of the single-key form are refused for.
constexpr size_t kGroupByKeysMost = 8;
inline SchemaRef group_by_schema(const Schema &in, const std::vector<std::string> &keys, const std::vector<AggSpec> &aggs) {
    if (keys.empty()) throw GroupByPlanError("group_by: no key columns");
    if (keys.size() > kGroupByKeysMost)
        throw GroupByPlanError("group_by: " + std::to_string(keys.size()) + " key columns; at most " + std::to_string(kGroupByKeysMost) + " are grouped");
    std::vector<Field> out;
    for (auto &key : keys) {
        const Field *kf = in.field_by_name(key);
        if (!kf) throw GroupByPlanError("group_by: unknown key column '" + key + "'");
        for (auto &f : out)
            if (f.name() == key) throw GroupByPlanError("group_by: key column '" + key + "' is named twice");
        out.push_back(Field{key, kf->data_type(), true});
    }
    return group_by_agg_fields(in, std::move(out), aggs);
}

// The single-key form as the list form sees it: `by_list` false is group_by(keys[0]), with that form's refusals.
inline SchemaRef group_by_schema(const Schema &in, const std::vector<std::string> &keys, const std::vector<AggSpec> &aggs, bool by_list) {
    return by_list ? group_by_schema(in, keys, aggs) : group_by_schema(in, keys.at(0), aggs);
}

// The Int64 ids of a String key column, through the string dictionary: equal strings share an id, a null string is a null id, "" is a value.
// Only the ids are needed, so the dictionary is freed at once.
inline ArrayRef string_key_ids(const ContextRef &ctx, const rv_dcolumn *strings) {
    rv_string_dict *dict = nullptr;
    rv_dcolumn *h = nullptr;
    check(rv_string_dict_build(ctx->raw(), strings, &dict, &h));
    const ArrayRef ids = Array::adopt(ctx, h);
    check(rv_string_dict_free(ctx->raw(), dict));
    return ids;
}

// One aggregation over the named columns of one frame (`columns` in the order of `schema`); the output columns in the order of
// group_by_schema: the keys, then the aggregates.  `by_list`: one rv_hash_aggregate_keys over the key tuple; else the single-key form,
// one rv_hash_aggregate over keys[0].  Every String key goes through the string dictionary on its own: its ids (null strings are null
// ids: the null group; "" is a value) stand in for it, and its key cells are gathered from the String column itself at the groups'
// first rows.
inline std::vector<ArrayRef> group_by_columns(const ContextRef &ctx, const Schema &schema, const std::vector<ArrayRef> &columns,
                                              const std::vector<std::string> &keys, const std::vector<AggSpec> &aggs, bool by_list) {
    (void)group_by_schema(schema, keys, aggs, by_list);
    const std::vector<const rv_dcolumn *> handles = column_handles(columns);
    auto handle_of = [&](const std::string &n) { return handles[*schema.index_of(n)]; };
    std::vector<const rv_dcolumn *> values;
    std::vector<rv_agg_spec> specs;
    for (auto &a : aggs) {
        rv_agg_spec s{static_cast<uint32_t>(a.op), 0};
        if (a.op != AggOp::CountRows) {
            const rv_dcolumn *h = handle_of(a.column);
            const auto at = std::find(values.begin(), values.end(), h);
            s.col = static_cast<uint32_t>(at - values.begin());
            if (at == values.end()) values.push_back(h);
        }
        specs.push_back(s);
    }
    std::vector<const rv_dcolumn *> key_cols, strings(keys.size(), nullptr);
    std::vector<ArrayRef> ids;  // keeps the ids of the String keys alive over the call
    for (size_t k = 0; k < keys.size(); ++k) {
        const rv_dcolumn *col = handle_of(keys[k]);
        if (schema.field_by_name(keys[k])->data_type() == DataType::String) {
            ids.push_back(string_key_ids(ctx, col));
            strings[k] = col;
            col = ids.back()->handle();
        }
        key_cols.push_back(col);
    }
    std::vector<rv_dcolumn *> out(keys.size() + specs.size(), nullptr);
    rv_dcolumn *first_row = nullptr;
    uint64_t groups = 0;
    if (by_list)
        check(rv_hash_aggregate_keys(ctx->raw(), key_cols.data(), static_cast<uint32_t>(key_cols.size()), values.data(), static_cast<uint32_t>(values.size()),
                                     specs.data(), static_cast<uint32_t>(specs.size()), out.data(), &first_row, &groups));
    else
        check(rv_hash_aggregate(ctx->raw(), key_cols[0], values.data(), static_cast<uint32_t>(values.size()), specs.data(),
                                static_cast<uint32_t>(specs.size()), out.data(), &first_row, &groups));
    std::vector<ArrayRef> res = adopt_columns(ctx, out);
    const ArrayRef first = Array::adopt(ctx, first_row);
    for (size_t k = 0; k < keys.size(); ++k) {
        if (!strings[k]) continue;  // the strings at the first rows in place of their ids
        rv_dcolumn *cells = nullptr;
        check(rv_take_device(ctx->raw(), &strings[k], 1, first->handle(), &cells));
        res[k] = Array::adopt(ctx, cells);
    }
    return res;
}
inline std::vector<ArrayRef> group_by_columns(const ContextRef &ctx, const Schema &schema, const std::vector<ArrayRef> &columns, const std::string &key,
                                              const std::vector<AggSpec> &aggs) {
    return group_by_columns(ctx, schema, columns, {key}, aggs, false);
}
inline std::vector<ArrayRef> group_by_columns(const ContextRef &ctx, const Schema &schema, const std::vector<ArrayRef> &columns,
                                              const std::vector<std::string> &keys, const std::vector<AggSpec> &aggs) {
    return group_by_columns(ctx, schema, columns, keys, aggs, true);
}

// group_by as a stream (a GpuBreakerStream): its one batch is the groups in first-row order.  An input without rows gives one zero-row
// batch with the output schema.  (Aggregating batch by batch without the concatenation -- a begin / update / finish handle -- is not
// built.)
class GpuGroupByStream : public GpuBreakerStream {
  public:
    GpuGroupByStream(JoinSide input, std::string key, std::vector<AggSpec> aggs, ContextRef fallback_ctx)
        : GpuGroupByStream(std::move(input), std::vector<std::string>{std::move(key)}, std::move(aggs), std::move(fallback_ctx), false) {}
    // the same over a list of key columns (group_by_schema(keys)): one batch, the keys first
    GpuGroupByStream(JoinSide input, std::vector<std::string> keys, std::vector<AggSpec> aggs, ContextRef fallback_ctx)
        : GpuGroupByStream(std::move(input), std::move(keys), std::move(aggs), std::move(fallback_ctx), true) {}
    // either form, as the plans hold it: `by_list` false is the single-key form over keys[0]
    GpuGroupByStream(JoinSide input, std::vector<std::string> keys, std::vector<AggSpec> aggs, ContextRef fallback_ctx, bool by_list)
        : GpuBreakerStream("group_by", std::move(input), std::move(fallback_ctx)), keys_(std::move(keys)), by_list_(by_list), aggs_(std::move(aggs)) {
        schema_ = group_by_schema(*input_schema_, keys_, aggs_, by_list_);
    }

  private:
    RecordBatch run(const ContextRef &ctx, const std::vector<ArrayRef> &columns) override {
        return batch_of(group_by_columns(ctx, *input_schema_, columns, keys_, aggs_, by_list_));
    }
    std::vector<std::string> keys_;  // one name and !by_list_: the single-key form
    bool by_list_;
    std::vector<AggSpec> aggs_;
};

// ---------------------------------------------------------------------------------------
// sort(keys) -- ORDER BY; the reference has no sort: include/rivulus_gpu.h, rv_sort_indices
// ---------------------------------------------------------------------------------------
// One sort key: the column, the direction of its values, and where its nulls go (first unless nulls_last; `descending` does not move them).
struct SortKey {
    std::string column;
    bool descending = false;
    bool nulls_last = false;
};
struct SortPlanError : std::runtime_error {  // what planning a sort refuses, with the column it refuses it for
    using std::runtime_error::runtime_error;
};

// Checks `keys` against `in` and returns the output schema -- the input's: a sort changes neither names nor dtypes.  Throws SortPlanError
// for an empty key list, an unknown column, and a key the device does not sort by (String, Boolean: not built).
inline SchemaRef sort_schema(const Schema &in, const std::vector<SortKey> &keys) {
    if (keys.empty()) throw SortPlanError("sort: no sort keys");
    for (auto &k : keys) {
        const Field *f = in.field_by_name(k.column);
        if (!f) throw SortPlanError("sort: unknown key column '" + k.column + "'");
        if (f->data_type() == DataType::String || f->data_type() == DataType::Boolean)
            throw SortPlanError("sort: key column '" + k.column + "' is " + to_string(f->data_type()) + "; only Int64 and Float64 keys are sorted");
    }
    return std::make_shared<const Schema>(in);
}

// What rv_sort and rv_top_k take of a frame (`columns` in the order of `schema`) and a key list: the handles, and per key the column's index
// and its flag word.
struct SortCall {
    std::vector<const rv_dcolumn *> handles;
    std::vector<uint32_t> key_cols, key_flags;
    SortCall(const Schema &schema, const std::vector<ArrayRef> &columns, const std::vector<SortKey> &keys) : handles(column_handles(columns)) {
        for (auto &k : keys) {
            key_cols.push_back(static_cast<uint32_t>(*schema.index_of(k.column)));
            key_flags.push_back((k.descending ? RV_SORT_DESCENDING : 0u) | (k.nulls_last ? RV_SORT_NULLS_LAST : 0u));
        }
    }
};

// One rv_sort over one frame (`columns` in the order of `schema`): every column reordered, the first key the most significant.  Columns
// that are no key ride along whatever their dtype.
inline std::vector<ArrayRef> sort_columns(const ContextRef &ctx, const Schema &schema, const std::vector<ArrayRef> &columns, const std::vector<SortKey> &keys) {
    (void)sort_schema(schema, keys);
    const SortCall call(schema, columns, keys);
    std::vector<rv_dcolumn *> out(call.handles.size(), nullptr);
    check(rv_sort(ctx->raw(), call.handles.data(), static_cast<uint32_t>(call.handles.size()), call.key_cols.data(), call.key_flags.data(),
                  static_cast<uint32_t>(keys.size()), out.data()));
    return adopt_columns(ctx, out);
}

// sort as a stream (a GpuBreakerStream): its one batch is every row, in order.  An input without rows gives one zero-row batch with the
// schema.  (Merging sorted runs in place of the concatenation is not built.)
class GpuSortStream : public GpuBreakerStream {
  public:
    GpuSortStream(JoinSide input, std::vector<SortKey> keys, ContextRef fallback_ctx)
        : GpuBreakerStream("sort", std::move(input), std::move(fallback_ctx)), keys_(std::move(keys)) {
        schema_ = sort_schema(*input_schema_, keys_);
    }

  private:
    RecordBatch run(const ContextRef &ctx, const std::vector<ArrayRef> &columns) override {
        if (columns.empty() || columns[0]->len() == 0) return RecordBatch::empty(ctx, schema_);
        return batch_of(sort_columns(ctx, *schema_, columns, keys_));
    }
    std::vector<SortKey> keys_;
};

// ---------------------------------------------------------------------------------------
// window(partition_by, order_by, exprs) -- f(...) OVER (PARTITION BY .. ORDER BY ..); the reference has no window expression:
// include/rivulus_gpu.h, rv_window and rv_window_frames
// ---------------------------------------------------------------------------------------
// rv_window_op and then rv_window_frame_op, in their order
enum class WindowOp { RowNumber, Rank, DenseRank, CumCount, CumSum, CumMin, CumMax, Lag, Lead, Count, Sum, Min, Max, Avg, FirstValue, LastValue, Ntile };
inline const char *to_string(WindowOp op) {
    static const char *n[] = {"ROW_NUMBER", "RANK", "DENSE_RANK", "CUM_COUNT", "CUM_SUM", "CUM_MIN", "CUM_MAX", "LAG", "LEAD",
                              "COUNT", "SUM", "MIN", "MAX", "AVG", "FIRST_VALUE", "LAST_VALUE", "NTILE"};
    return n[static_cast<int>(op)];
}
inline bool window_op_reads_a_column(WindowOp op) {
    return op != WindowOp::RowNumber && op != WindowOp::Rank && op != WindowOp::DenseRank && op != WindowOp::Ntile;
}
// Count .. LastValue: the ops that aggregate or pick over the frame [preceding, following]
inline bool window_op_has_a_frame(WindowOp op) { return op >= WindowOp::Count && op <= WindowOp::LastValue; }
// One window expression: `op` over `column` (ignored by the three numberings and Ntile), `offset` rows back or ahead (Lag / Lead) or the
// number of buckets (Ntile), under the output name `alias`.  Count .. LastValue work over the ROWS frame of `preceding` rows before the
// current one to `following` after it: signed, RV_FRAME_UNBOUNDED for the partition's edge (the default is the running frame); the
// other ops ignore the two.
struct WindowExpr {
    WindowOp op;
    std::string column;
    uint64_t offset = 0;
    std::string alias;
    int64_t preceding = RV_FRAME_UNBOUNDED, following = 0;
};
struct WindowPlanError : std::runtime_error {  // what planning a window refuses, with the column it refuses it for
    using std::runtime_error::runtime_error;
};
constexpr size_t kWindowKeysMost = 8;

// Checks the window against `in` and returns the output schema: the input's fields, then one field per expression under its alias --
// numbers, counts and NTILE Int64, SUM / MIN / MAX, LAG / LEAD and FIRST / LAST_VALUE of the column's dtype, AVG Float64; MIN / MAX, AVG,
// LAG / LEAD and FIRST / LAST_VALUE are nullable.
// Partition keys may be of any dtype (String keys go through the dictionary); order keys are what the sort takes.  Throws WindowPlanError
// for an empty expression list, an unknown column, more than 8 partition or order keys, a String / Boolean order key (with the sort's
// words), SUM / MIN / MAX / AVG over a column that is not Int64 or Float64, NTILE with 0 buckets, a frame with preceding + following < 0
// or a finite offset beyond 2^62 (these three name the column and the alias), and an empty or duplicate alias.
inline SchemaRef window_schema(const Schema &in, const std::vector<std::string> &partition_by, const std::vector<SortKey> &order_by,
                               const std::vector<WindowExpr> &exprs) {
    if (exprs.empty()) throw WindowPlanError("window: no window expressions");
    if (partition_by.size() > kWindowKeysMost)
        throw WindowPlanError("window: " + std::to_string(partition_by.size()) + " partition columns; at most " + std::to_string(kWindowKeysMost) + " are taken");
    if (order_by.size() > kWindowKeysMost)
        throw WindowPlanError("window: " + std::to_string(order_by.size()) + " order columns; at most " + std::to_string(kWindowKeysMost) + " are taken");
    for (auto &p : partition_by)
        if (!in.field_by_name(p)) throw WindowPlanError("window: unknown partition column '" + p + "'");
    for (auto &k : order_by) {
        const Field *f = in.field_by_name(k.column);
        if (!f) throw WindowPlanError("window: unknown order column '" + k.column + "'");
        if (f->data_type() == DataType::String || f->data_type() == DataType::Boolean)
            throw WindowPlanError("window: order column '" + k.column + "' is " + to_string(f->data_type()) + "; only Int64 and Float64 keys are sorted");
    }
    std::vector<Field> out = in.fields();
    for (auto &e : exprs) {
        DataType t = DataType::Int64;
        if (window_op_reads_a_column(e.op)) {
            const Field *f = in.field_by_name(e.column);
            if (!f) throw WindowPlanError("window: expression '" + e.alias + "' reads the unknown column '" + e.column + "'");
            if (e.op != WindowOp::CumCount && e.op != WindowOp::Count) t = f->data_type();
            if ((e.op == WindowOp::CumSum || e.op == WindowOp::CumMin || e.op == WindowOp::CumMax) && t != DataType::Int64 && t != DataType::Float64)
                throw WindowPlanError(std::string("window: ") + to_string(e.op) + " over column '" + e.column + "' of dtype " + to_string(t));
            if (e.op >= WindowOp::Sum && e.op <= WindowOp::Avg && t != DataType::Int64 && t != DataType::Float64)
                throw WindowPlanError(std::string("window: ") + to_string(e.op) + " over column '" + e.column + "' of dtype " + to_string(t) + " (expression '" +
                                      e.alias + "')");
            if (e.op == WindowOp::Avg) t = DataType::Float64;
        }
        if (e.op == WindowOp::Ntile && e.offset == 0) throw WindowPlanError("window: NTILE expression '" + e.alias + "' has 0 buckets");
        if (window_op_has_a_frame(e.op)) {
            const int64_t most = int64_t{1} << 62;
            const bool pu = e.preceding == RV_FRAME_UNBOUNDED, fu = e.following == RV_FRAME_UNBOUNDED;
            const std::string what = std::string("window: the frame of the ") + to_string(e.op) + " expression '" + e.alias + "' over column '" + e.column + "' ";
            if ((!pu && (e.preceding < -most || e.preceding > most)) || (!fu && (e.following < -most || e.following > most)))
                throw WindowPlanError(what + "has a finite offset beyond 2^62");
            if (!pu && !fu && e.preceding < -e.following) throw WindowPlanError(what + "has preceding + following < 0");
        }
        if (e.alias.empty()) throw WindowPlanError(std::string("window: the ") + to_string(e.op) + " expression over column '" + e.column + "' has no alias");
        for (auto &f : out)
            if (f.name() == e.alias) throw WindowPlanError("window: duplicate output name '" + e.alias + "'");
        const bool nullable = e.op == WindowOp::CumMin || e.op == WindowOp::CumMax || e.op == WindowOp::Lag || e.op == WindowOp::Lead || e.op == WindowOp::Min ||
                              e.op == WindowOp::Max || e.op == WindowOp::Avg || e.op == WindowOp::FirstValue || e.op == WindowOp::LastValue;
        out.push_back(Field{e.alias, t, nullable});
    }
    return std::make_shared<const Schema>(out);
}

// One rv_window_frames over one frame (`columns` in the order of `schema`): the NEW columns, one per expression, in the frame's row order.
// Every String partition key goes through the string dictionary on its own (string_key_ids): its ids (a null string is a null id; "" is
// a value) stand in the tuple.
inline std::vector<ArrayRef> window_columns(const ContextRef &ctx, const Schema &schema, const std::vector<ArrayRef> &columns,
                                            const std::vector<std::string> &partition_by, const std::vector<SortKey> &order_by,
                                            const std::vector<WindowExpr> &exprs) {
    (void)window_schema(schema, partition_by, order_by, exprs);
    const SortCall call(schema, columns, order_by);
    std::vector<const rv_dcolumn *> handles = call.handles;
    std::vector<ArrayRef> ids;  // keeps the ids of the String keys alive over the call
    std::vector<uint32_t> part_cols;
    for (auto &p : partition_by) {
        const size_t at = *schema.index_of(p);
        if (schema.field_by_name(p)->data_type() != DataType::String) {
            part_cols.push_back(static_cast<uint32_t>(at));
            continue;
        }
        ids.push_back(string_key_ids(ctx, call.handles[at]));
        part_cols.push_back(static_cast<uint32_t>(handles.size()));
        handles.push_back(ids.back()->handle());
    }
    std::vector<rv_window_frame_spec> specs;
    for (auto &e : exprs)
        specs.push_back(rv_window_frame_spec{static_cast<uint32_t>(e.op), window_op_reads_a_column(e.op) ? static_cast<uint32_t>(*schema.index_of(e.column)) : 0u,
                                             e.offset, e.preceding, e.following});
    std::vector<rv_dcolumn *> out(specs.size(), nullptr);
    check(rv_window_frames(ctx->raw(), handles.data(), static_cast<uint32_t>(handles.size()), part_cols.data(), static_cast<uint32_t>(part_cols.size()),
                    call.key_cols.data(), call.key_flags.data(), static_cast<uint32_t>(order_by.size()), specs.data(), static_cast<uint32_t>(specs.size()),
                    out.data()));
    return adopt_columns(ctx, out);
}

// window as a stream (a GpuBreakerStream): its one batch is every row in input order, the new columns appended.  An input without rows
// gives one zero-row batch with the schema.  (Windows over input that arrives partitioned, batch by batch, are not built.)
class GpuWindowStream : public GpuBreakerStream {
  public:
    GpuWindowStream(JoinSide input, std::vector<std::string> partition_by, std::vector<SortKey> order_by, std::vector<WindowExpr> exprs, ContextRef fallback_ctx)
        : GpuBreakerStream("window", std::move(input), std::move(fallback_ctx)), partition_by_(std::move(partition_by)), order_by_(std::move(order_by)),
          exprs_(std::move(exprs)) {
        schema_ = window_schema(*input_schema_, partition_by_, order_by_, exprs_);
    }

  private:
    RecordBatch run(const ContextRef &ctx, const std::vector<ArrayRef> &columns) override {
        if (columns.empty() || columns[0]->len() == 0) return RecordBatch::empty(ctx, schema_);
        std::vector<ArrayRef> out = columns;
        for (auto &c : window_columns(ctx, *input_schema_, columns, partition_by_, order_by_, exprs_)) out.push_back(c);
        return batch_of(std::move(out));
    }
    std::vector<std::string> partition_by_;
    std::vector<SortKey> order_by_;
    std::vector<WindowExpr> exprs_;
};

// ---------------------------------------------------------------------------------------
// top_k(keys, k) -- ORDER BY ... LIMIT k: the first k rows of sort(keys); include/rivulus_gpu.h, rv_top_k_indices
// ---------------------------------------------------------------------------------------
// Checks `keys` against `in` as sort_schema does -- the same SortPlanError, the same texts -- and returns the output schema, the input's.
inline SchemaRef top_k_schema(const Schema &in, const std::vector<SortKey> &keys, size_t /*k*/) { return sort_schema(in, keys); }

// One rv_top_k over one frame: the first min(k, rows) rows of sort_columns, every column.
inline std::vector<ArrayRef> top_k_columns(const ContextRef &ctx, const Schema &schema, const std::vector<ArrayRef> &columns, const std::vector<SortKey> &keys,
                                           size_t k) {
    (void)top_k_schema(schema, keys, k);
    const SortCall call(schema, columns, keys);
    std::vector<rv_dcolumn *> out(call.handles.size(), nullptr);
    check(rv_top_k(ctx->raw(), call.handles.data(), static_cast<uint32_t>(call.handles.size()), call.key_cols.data(), call.key_flags.data(),
                   static_cast<uint32_t>(keys.size()), static_cast<uint64_t>(k), out.data()));
    return adopt_columns(ctx, out);
}

// Rows a GpuTopKStream gathers before it folds them into its best k.  Set by reasoning, not by a sweep: a fold is one rv_top_k -- a dozen
// launches and a few read-backs, a few hundred microseconds whatever the size -- so it is amortised over millions of rows (a pass over
// 4 Mi rows of a key is about 10 us of HBM time per read), while 4 Mi rows of a handful of 8-byte columns stay in the low hundreds of MiB.
constexpr size_t kTopKFoldRows = size_t{1} << 22;

// top_k as a stream: a PIPELINE BREAKER that emits EXACTLY ONE batch of min(k, rows) rows.  A resident frame is taken whole.  The batches
// of any other stream are NOT concatenated: they are gathered until they hold at least `fold_rows` rows and then folded,
//     best = top_k(concat(best, gathered...)),
// so no more than fold_rows + k rows (and the batch that crossed the line) are held at once.  The fold is exact: `best` comes before
// the later rows in the concatenation and the sort is stable, so rows with equal keys come out in input order, whatever batches they
// arrived in.  An input without rows gives one zero-row batch with the schema.
class GpuTopKStream : public GpuBreakerStream {
  public:
    GpuTopKStream(JoinSide input, std::vector<SortKey> keys, size_t k, ContextRef fallback_ctx, size_t fold_rows = kTopKFoldRows)
        : GpuBreakerStream("top_k", std::move(input), std::move(fallback_ctx)), keys_(std::move(keys)), k_(k), fold_rows_(std::max<size_t>(fold_rows, 1)) {
        schema_ = top_k_schema(*input_schema_, keys_, k_);
    }
    size_t folds() const { return folds_; }  // rv_top_k calls so far (tests)
    std::optional<RecordBatch> next_batch() override {  // the fold in place of the drain
        if (done_) return std::nullopt;
        done_ = true;
        auto best_of = [&](const std::vector<ArrayRef> &columns) { return stream_call([&] { return run(ctx_of(columns), columns); }); };
        if (!input_.stream) return best_of(input_.columns);
        std::optional<RecordBatch> best;
        std::vector<RecordBatch> gathered;
        size_t gathered_rows = 0;
        auto fold = [&] {
            std::vector<RecordBatch> all;
            if (best) all.push_back(*best);
            for (auto &b : gathered) all.push_back(std::move(b));
            gathered.clear();
            gathered_rows = 0;
            best = all.size() == 1 ? best_of(all[0].columns()) : best_of(stream_call([&] { return RecordBatch::concat(all); }).columns());
        };
        while (auto b = input_.stream->next_batch()) {
            if (!ctx_ && b->num_columns() > 0) ctx_ = b->column(0)->context();
            if (b->num_rows() == 0) continue;
            gathered_rows += b->num_rows();
            gathered.push_back(std::move(*b));
            if (gathered_rows >= fold_rows_) fold();
        }
        if (!gathered.empty()) fold();
        if (best) return best;
        return no_batch();
    }

  private:
    RecordBatch run(const ContextRef &ctx, const std::vector<ArrayRef> &columns) override {
        if (columns.empty() || columns[0]->len() == 0) return RecordBatch::empty(ctx, schema_);
        ++folds_;
        return batch_of(top_k_columns(ctx, *schema_, columns, keys_, k_));
    }
    std::vector<SortKey> keys_;
    size_t k_, fold_rows_, folds_ = 0;
};

}  // namespace execution

// ---------------------------------------------------------------------------------------
// expressions -- expr.rs:3-139
// ---------------------------------------------------------------------------------------
namespace expressions {
enum class BinaryOperator { Plus, Minus, Multiply, Divide, Eq, NotEq, Lt, Gt, LtEq, GtEq, And, Or };
struct Expr;
using ExprPtr = std::shared_ptr<const Expr>;
struct Expr {
    enum Kind { Column, Literal, BinaryExpr, Alias } kind = Column;
    std::string name;             // Column / Alias
    execution::Literal literal;   // Literal
    ExprPtr left, right;          // BinaryExpr (left, right) / Alias (left)
    BinaryOperator op = BinaryOperator::Eq;

    static Expr col(const std::string &n) {
        Expr e;
        e.kind = Column;
        e.name = n;
        return e;
    }
    static Expr lit(execution::Literal v) {
        Expr e;
        e.kind = Literal;
        e.literal = std::move(v);
        return e;
    }
    static Expr lit(int v) { return lit(execution::Literal(static_cast<int64_t>(v))); }
    static Expr lit(const char *v) { return lit(execution::Literal(std::string(v))); }
    Expr alias(const std::string &n) const {
        Expr e;
        e.kind = Alias;
        e.name = n;
        e.left = std::make_shared<Expr>(*this);
        return e;
    }
    Expr binary(BinaryOperator o, const Expr &r) const {
        Expr e;
        e.kind = BinaryExpr;
        e.op = o;
        e.left = std::make_shared<Expr>(*this);
        e.right = std::make_shared<Expr>(r);
        return e;
    }
    Expr eq(const Expr &o) const { return binary(BinaryOperator::Eq, o); }
    Expr neq(const Expr &o) const { return binary(BinaryOperator::NotEq, o); }
    Expr lt(const Expr &o) const { return binary(BinaryOperator::Lt, o); }
    Expr gt(const Expr &o) const { return binary(BinaryOperator::Gt, o); }
    Expr lte(const Expr &o) const { return binary(BinaryOperator::LtEq, o); }
    Expr gte(const Expr &o) const { return binary(BinaryOperator::GtEq, o); }
    Expr and_(const Expr &o) const { return binary(BinaryOperator::And, o); }
    Expr or_(const Expr &o) const { return binary(BinaryOperator::Or, o); }
    Expr add(const Expr &o) const { return binary(BinaryOperator::Plus, o); }
    Expr sub(const Expr &o) const { return binary(BinaryOperator::Minus, o); }
    Expr mul(const Expr &o) const { return binary(BinaryOperator::Multiply, o); }
    Expr div(const Expr &o) const { return binary(BinaryOperator::Divide, o); }
};
}  // namespace expressions

// ---------------------------------------------------------------------------------------
// physical_plan -- planner.rs, streaming_planner.rs, streaming.rs, plan.rs
// ---------------------------------------------------------------------------------------
namespace physical_plan {
using execution::CompareTerm;
using execution::JoinType;
using expressions::BinaryOperator;
using expressions::Expr;

struct ConversionError : std::runtime_error {  // planner.rs:8-39
    enum Kind { UnsupportedExpression, UnsupportedFilter, InvalidFilterStructure, FilterLeftNotColumn, FilterRightNotLiteral,
                UnsupportedFilterOperator, InvalidSelectExpression } kind;
    ConversionError(Kind k, const std::string &m) : std::runtime_error(m), kind(k) {}
};
struct StreamingPlannerError : std::runtime_error {  // streaming_planner.rs:11-27
    enum Kind { ExpressionError } kind = ExpressionError;
    using std::runtime_error::runtime_error;
};

inline bool is_compare(BinaryOperator op) { return op >= BinaryOperator::Eq && op <= BinaryOperator::GtEq; }
inline rv_cmp to_cmp(BinaryOperator op) {
    switch (op) {
        case BinaryOperator::Eq: return RV_EQ;
        case BinaryOperator::NotEq: return RV_NE;
        case BinaryOperator::Lt: return RV_LT;
        case BinaryOperator::Gt: return RV_GT;
        case BinaryOperator::LtEq: return RV_LE;
        default: return RV_GE;
    }
}

// planner.rs:113-132
inline std::pair<std::string, std::string> convert_select_expr(const Expr &e) {
    switch (e.kind) {
        case Expr::Column: return {e.name, e.name};
        case Expr::Alias:
            if (e.left->kind == Expr::Column) return {e.left->name, e.name};
            throw ConversionError(ConversionError::UnsupportedExpression, "Unsupported expression");
        case Expr::BinaryExpr: throw ConversionError(ConversionError::UnsupportedExpression, "Unsupported expression");
        default: throw ConversionError(ConversionError::InvalidSelectExpression, "Select expression must be a column or alias");
    }
}

// planner.rs:134-189: the eager grammar -- exactly one `Column <cmp> Literal`
inline CompareTerm convert_filter_predicate(const Expr &p) {
    if (p.kind != Expr::BinaryExpr) {
        const char *t = p.kind == Expr::Column ? "Column" : (p.kind == Expr::Literal ? "Literal" : "Alias");
        throw ConversionError(ConversionError::InvalidFilterStructure, std::string("Filter must be a binary comparison, found: ") + t);
    }
    if (p.op == BinaryOperator::And || p.op == BinaryOperator::Or)
        throw ConversionError(ConversionError::UnsupportedFilter, "Unsupported filter: only simple column comparisons supported");
    if (!is_compare(p.op)) throw ConversionError(ConversionError::UnsupportedFilterOperator, "Unsupported binary operator in filter");
    if (p.left->kind != Expr::Column) throw ConversionError(ConversionError::FilterLeftNotColumn, "Filter left side must be a column reference");
    if (p.right->kind != Expr::Literal) throw ConversionError(ConversionError::FilterRightNotLiteral, "Filter right side must be a literal value");
    return CompareTerm{p.left->name, to_cmp(p.op), p.right->literal};
}

// streaming_planner.rs:102-135 (alias name dropped, :110-113)
inline std::vector<std::string> extract_column_names_from_expressions(const std::vector<Expr> &exprs) {
    std::vector<std::string> out;
    for (auto &e : exprs) {
        if (e.kind == Expr::Column) out.push_back(e.name);
        else if (e.kind == Expr::Alias && e.left->kind == Expr::Column) out.push_back(e.left->name);
        else if (e.kind == Expr::Alias) throw StreamingPlannerError("Expression conversion error: Complex expressions with aliases not yet supported");
        else throw StreamingPlannerError("Expression conversion error: Complex expressions not yet supported in streaming mode");
    }
    return out;
}

// streaming_planner.rs:137-168: what the REFERENCE accepts (a bare Boolean column)
inline std::string extract_boolean_predicate_column(const Expr &p) {
    if (p.kind == Expr::Column) return p.name;
    if (p.kind == Expr::BinaryExpr) {
        if (p.left->kind == Expr::Column)
            throw StreamingPlannerError("Expression conversion error: Binary expressions not yet supported in streaming mode. Found expression on column '" +
                                        p.left->name + "'. Currently only simple boolean column references are supported (e.g., .filter(col('is_active')))");
        throw StreamingPlannerError("Expression conversion error: Complex binary expressions not supported in streaming mode");
    }
    throw StreamingPlannerError("Expression conversion error: Unsupported filter expression type");
}

// The lowering the new backend adds: `Column <cmp> Literal`, a bare Boolean column, and AND / OR trees of those
// (BinaryOperator::{And, Or}, expr.rs:27-28) become the term list + postfix program of one fused device pass.
// Arithmetic is not this function's: it keeps refusing it (ExpressionError, like the reference), and
// lower_computed_predicate / lower_select_exprs below take `<arith> <cmp> <literal>` filters and computed select
// expressions to the device through rv_eval_arith.
inline void lower_predicate(const Expr &p, execution::LoweredPredicate &out, bool &has_or) {
    auto push_term = [&](CompareTerm t) {
        if (out.terms.size() >= 16) throw StreamingPlannerError("Expression conversion error: more than 16 compare terms in one filter");
        out.expr.push_back(static_cast<uint8_t>(out.terms.size()));
        out.terms.push_back(std::move(t));
    };
    if (p.kind == Expr::Column) return push_term(CompareTerm{p.name, RV_IS_TRUE, {}});
    if (p.kind == Expr::BinaryExpr && (p.op == BinaryOperator::And || p.op == BinaryOperator::Or)) {
        lower_predicate(*p.left, out, has_or);
        lower_predicate(*p.right, out, has_or);
        out.expr.push_back(p.op == BinaryOperator::And ? RV_EXPR_AND : RV_EXPR_OR);
        has_or = has_or || p.op == BinaryOperator::Or;
        return;
    }
    if (p.kind == Expr::BinaryExpr && is_compare(p.op) && p.left->kind == Expr::Column && p.right->kind == Expr::Literal)
        return push_term(CompareTerm{p.left->name, to_cmp(p.op), p.right->literal});
    throw StreamingPlannerError("Expression conversion error: only AND / OR of `column <cmp> literal` terms and Boolean columns run on the device");
}
inline execution::LoweredPredicate lower_predicate(const Expr &p) {
    execution::LoweredPredicate out;
    bool has_or = false;
    lower_predicate(p, out, has_or);
    if (!has_or) out.expr.clear();  // the AND of the terms: the plain term list (pipelined begin / finish path)
    return out;
}

// ---- arithmetic: Expr::add / sub / mul / div (expr.rs:17-20, 44-74) -----------------------------------------------------------
inline bool is_arithmetic(BinaryOperator op) { return op <= BinaryOperator::Divide; }
inline bool is_arithmetic(const Expr &e) { return e.kind == Expr::BinaryExpr && is_arithmetic(e.op); }
inline rv_arith_op to_arith_op(BinaryOperator op) { return static_cast<rv_arith_op>(RV_ARITH_ADD + static_cast<int>(op)); }
inline execution::DataType literal_data_type(const execution::Literal &v) {  // AnyValue::data_type
    static const execution::DataType t[] = {execution::DataType::Null, execution::DataType::Int64, execution::DataType::Float64,
                                            execution::DataType::Boolean, execution::DataType::String};
    return t[v.index()];
}
// infer_binary_result_type for the four arithmetic operators (logical_plan/plan.rs:250-260).  Where the reference infers Null for a
// Boolean / String operand (:259) this is a type mismatch: there is no arithmetic on those cells.
inline execution::DataType infer_arith_result_type(execution::DataType left, execution::DataType right) {
    using execution::DataType;
    for (DataType t : {left, right})
        if (t == DataType::Boolean || t == DataType::String) throw Error(RV_ERR_TYPE_MISMATCH, std::string("no arithmetic on ") + to_string(t) + " operands");
    if (left == DataType::Float64 || right == DataType::Float64) return DataType::Float64;
    if (left == DataType::Int64 || right == DataType::Int64) return DataType::Int64;
    return DataType::Null;
}
// resolve_expr_schema (plan.rs:204-233) of an arithmetic tree, and its postfix program: {name of the left-most leaf, dtype}.
// An alias inside the tree names its subtree and changes nothing else; a column the schema lacks types as Null, as there.
inline std::pair<std::string, execution::DataType> lower_arith(const Expr &e, const execution::Schema &schema, std::vector<execution::ArithStep> &out) {
    switch (e.kind) {
        case Expr::Column: {
            out.push_back(execution::ArithStep{RV_ARITH_COL, e.name, {}});
            const execution::Field *f = schema.field_by_name(e.name);
            return {e.name, f ? f->data_type() : execution::DataType::Null};
        }
        case Expr::Literal: out.push_back(execution::ArithStep{RV_ARITH_LIT, "", e.literal}); return {"literal", literal_data_type(e.literal)};
        case Expr::Alias: return {e.name, lower_arith(*e.left, schema, out).second};
        default: {
            if (!is_arithmetic(e.op)) throw ConversionError(ConversionError::UnsupportedExpression, "Unsupported expression: a comparison inside an arithmetic expression");
            auto l = lower_arith(*e.left, schema, out);
            auto r = lower_arith(*e.right, schema, out);
            out.push_back(execution::ArithStep{to_arith_op(e.op), "", {}});
            return {l.first, infer_arith_result_type(l.second, r.second)};
        }
    }
}
inline bool reads_a_column(const std::vector<execution::ArithStep> &program) {
    return std::any_of(program.begin(), program.end(), [](const execution::ArithStep &s) { return s.op == RV_ARITH_COL; });
}

// select([...]) with arithmetic: every expression becomes a plain column (Column, or an alias of one: convert_select_expr's two
// forms) or an arithmetic program; name and dtype follow resolve_expr_schema.  A bare literal stays InvalidSelectExpression.
inline std::vector<execution::LoweredSelect> lower_select_exprs(const std::vector<Expr> &exprs, const execution::Schema &schema) {
    std::vector<execution::LoweredSelect> out;
    for (const Expr &top : exprs) {
        execution::LoweredSelect s;
        const Expr *e = &top;
        std::optional<std::string> alias;
        while (e->kind == Expr::Alias) {  // the outermost alias names the column
            if (!alias) alias = e->name;
            e = e->left.get();
        }
        if (e->kind == Expr::Literal) {
            if (alias) throw ConversionError(ConversionError::UnsupportedExpression, "Unsupported expression");
            throw ConversionError(ConversionError::InvalidSelectExpression, "Select expression must be a column or alias");
        }
        if (e->kind == Expr::Column) {
            const execution::Field *f = schema.field_by_name(e->name);
            s.source = e->name;
            s.name = e->name;
            s.data_type = f ? f->data_type() : execution::DataType::Null;
        } else {
            if (!is_arithmetic(*e)) throw ConversionError(ConversionError::UnsupportedExpression, "Unsupported expression");
            auto named = lower_arith(*e, schema, s.program);
            if (!reads_a_column(s.program)) throw ConversionError(ConversionError::UnsupportedExpression, "Unsupported expression: arithmetic over literals alone");
            s.name = named.first;
            s.data_type = named.second;
        }
        if (alias) s.name = *alias;
        out.push_back(std::move(s));
    }
    return out;
}

// filter(...) with arithmetic on the left of a compare: `<arith> <cmp> <literal>`, alone or under AND / OR with the terms
// lower_predicate takes.  Every computed left side becomes the helper column "__arith<k>".
inline void lower_computed_predicate(const Expr &p, const execution::Schema &schema, execution::ComputedPredicate &out, bool &has_or) {
    auto push_term = [&](CompareTerm t) {
        if (out.predicate.terms.size() >= 16) throw StreamingPlannerError("Expression conversion error: more than 16 compare terms in one filter");
        out.predicate.expr.push_back(static_cast<uint8_t>(out.predicate.terms.size()));
        out.predicate.terms.push_back(std::move(t));
    };
    if (p.kind == Expr::BinaryExpr && (p.op == BinaryOperator::And || p.op == BinaryOperator::Or)) {
        lower_computed_predicate(*p.left, schema, out, has_or);
        lower_computed_predicate(*p.right, schema, out, has_or);
        out.predicate.expr.push_back(p.op == BinaryOperator::And ? RV_EXPR_AND : RV_EXPR_OR);
        has_or = has_or || p.op == BinaryOperator::Or;
        return;
    }
    if (p.kind == Expr::BinaryExpr && is_compare(p.op) && is_arithmetic(*p.left) && p.right->kind == Expr::Literal) {
        execution::LoweredSelect helper;
        helper.data_type = lower_arith(*p.left, schema, helper.program).second;
        if (!reads_a_column(helper.program)) throw StreamingPlannerError("Expression conversion error: arithmetic over literals alone");
        helper.name = "__arith" + std::to_string(out.helpers.size());
        push_term(CompareTerm{helper.name, to_cmp(p.op), p.right->literal});
        out.helpers.push_back(std::move(helper));
        return;
    }
    execution::LoweredPredicate plain;  // a term of the existing grammar (or its refusal)
    bool unused = false;
    lower_predicate(p, plain, unused);
    push_term(std::move(plain.terms.at(0)));
}
inline execution::ComputedPredicate lower_computed_predicate(const Expr &p, const execution::Schema &schema) {
    execution::ComputedPredicate out;
    bool has_or = false;
    lower_computed_predicate(p, schema, out, has_or);
    if (!has_or) out.predicate.expr.clear();
    return out;
}
// the columns of `in` and then the helper columns: the projection that feeds a computed filter
inline std::vector<execution::LoweredSelect> with_arith_helpers(const execution::Schema &in, const std::vector<execution::LoweredSelect> &helpers) {
    std::vector<execution::LoweredSelect> all;
    for (auto &f : in.fields()) {
        execution::LoweredSelect s;
        s.name = s.source = f.name();
        s.data_type = f.data_type();
        all.push_back(std::move(s));
    }
    all.insert(all.end(), helpers.begin(), helpers.end());
    return all;
}

// StreamingPhysicalPlan -- streaming.rs:29-133, collect :235-238 + :343-352
struct StreamingExecutionError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct DeviceFrame {  // the typed-column stand-in for datatypes::DataFrame
    std::vector<std::string> names;
    std::vector<execution::ArrayRef> columns;
    size_t height() const { return columns.empty() ? 0 : columns[0]->len(); }
    size_t width() const { return columns.size(); }
    std::optional<size_t> index_of(const std::string &n) const {
        for (size_t i = 0; i < names.size(); ++i)
            if (names[i] == n) return i;
        return std::nullopt;
    }
    const execution::ArrayRef *column(const std::string &n) const {
        const auto i = index_of(n);
        return i ? &columns[*i] : nullptr;
    }
};

inline execution::Schema frame_schema(const DeviceFrame &df) { return *execution::nullable_schema(df.names, df.columns); }

// dataframe_to_batches -- streaming.rs:135-233: batch_size-row chunks (zero-copy slices); the null cells of
// Int64 / Float64 / Boolean columns become 0 / 0.0 / false and the column loses its bitmap (the reference
// builds those arrays with from_values / from_bools); String columns keep their nulls; every field nullable.
inline std::vector<execution::RecordBatch> dataframe_to_batches(const DeviceFrame &df, size_t batch_size) {
    using namespace execution;
    std::vector<RecordBatch> batches;
    if (df.columns.empty() || df.height() == 0) return batches;  // df.is_empty()
    if (batch_size == 0) throw Panic("attempt to divide by zero");
    const SchemaRef schema = nullable_schema(df.names, df.columns);
    const size_t rows = df.height();
    for (size_t start = 0; start < rows; start += batch_size) {
        const size_t len = std::min(batch_size, rows - start);
        std::vector<ArrayRef> arrays;
        for (auto &col : df.columns) {
            ArrayRef piece = col->slice(start, len);
            rv_dcolumn *filled = nullptr;
            check(rv_fill_nulls(piece->context()->raw(), piece->handle(), &filled));
            arrays.push_back(Array::adopt(piece->context(), filled));
        }
        batches.push_back(RecordBatch::try_new(schema, std::move(arrays)));
    }
    return batches;
}

class StreamingPhysicalPlan;
using StreamingPlanPtr = std::shared_ptr<const StreamingPhysicalPlan>;
class StreamingPhysicalPlan {
  public:
    enum Kind { MemorySource, DataFrameSource, CsvFileSource, Filter, GpuFilterProject, Select, Limit, HashJoin, Project, ComputedFilterProject, GroupBy, Sort, TopK, Window } kind = MemorySource;
    std::vector<Expr> exprs;  // Project: select expressions, arithmetic included
    Expr predicate_expr;      // ComputedFilterProject: a filter with `<arith> <cmp> <literal>` terms
    // DataFrameSource (streaming.rs:85-94)
    DeviceFrame df;
    size_t df_batch_size = 0;
    // CsvFileSource (streaming.rs:95-105)
    ContextRef csv_ctx;
    std::string csv_path;
    execution::SchemaRef csv_schema;
    std::optional<size_t> csv_batch_size;
    std::optional<char> csv_delimiter;
    execution::CsvNulls csv_nulls = execution::CsvNulls::AsReference;
    execution::CsvScan csv_scan = execution::CsvScan::Host;
    std::vector<execution::RecordBatch> batches;
    StreamingPlanPtr input;
    std::string predicate_column;
    execution::LoweredPredicate predicate;
    std::vector<std::string> columns;
    size_t n = 0;
    StreamingPlanPtr build_side;  // HashJoin { build_side, probe_side = input, build_key, probe_key, join_kind }: the sides as joined
    rv_join_kind join_kind = RV_JOIN_INNER;
    std::string build_key, probe_key;
    std::vector<std::string> group_keys;  // GroupBy { input, group_keys, aggs }: the key list, or the one key of the single-key form
    bool group_by_list = false;           // ... which of the two forms
    std::vector<execution::AggSpec> aggs;
    std::vector<execution::SortKey> sort_keys;  // Sort { input, sort_keys }, TopK { input, sort_keys, top_k_rows, top_k_fold_rows }
    size_t top_k_rows = 0, top_k_fold_rows = execution::kTopKFoldRows;
    std::vector<std::string> partition_keys;  // Window { input, partition_keys, sort_keys (the window order), window_exprs }
    std::vector<execution::WindowExpr> window_exprs;

    static StreamingPlanPtr memory_source(std::vector<execution::RecordBatch> b) {
        auto p = node(MemorySource);
        p->batches = std::move(b);
        return p;
    }
    static StreamingPlanPtr dataframe_source(DeviceFrame df, size_t batch_size) {
        auto p = node(DataFrameSource);
        p->df = std::move(df);
        p->df_batch_size = batch_size;
        return p;
    }
    static StreamingPlanPtr csv_file_source(ContextRef ctx, std::string path, execution::SchemaRef schema, std::optional<size_t> batch_size = std::nullopt,
                                            std::optional<char> delimiter = std::nullopt, execution::CsvNulls nulls = execution::CsvNulls::AsReference,
                                            execution::CsvScan scan = execution::CsvScan::Host) {
        auto p = node(CsvFileSource);
        p->csv_ctx = std::move(ctx);
        p->csv_path = std::move(path);
        p->csv_schema = std::move(schema);
        p->csv_batch_size = batch_size;
        p->csv_delimiter = delimiter;
        p->csv_nulls = nulls;
        p->csv_scan = scan;
        return p;
    }
    static StreamingPlanPtr filter(StreamingPlanPtr in, std::string predicate_column) {
        auto p = node(Filter, std::move(in));
        p->predicate_column = std::move(predicate_column);
        return p;
    }
    // Filter(expr) followed by Select(columns): one fused operator
    static StreamingPlanPtr gpu_filter_project(StreamingPlanPtr in, execution::LoweredPredicate predicate, std::vector<std::string> columns) {
        auto p = node(GpuFilterProject, std::move(in));
        p->predicate = std::move(predicate);
        p->columns = std::move(columns);
        return p;
    }
    static StreamingPlanPtr select(StreamingPlanPtr in, std::vector<std::string> columns) {
        auto p = node(Select, std::move(in));
        p->columns = std::move(columns);
        return p;
    }
    // select([...]) whose expressions may be arithmetic (lower_select_exprs): GpuProjectStream
    static StreamingPlanPtr project(StreamingPlanPtr in, std::vector<Expr> exprs) {
        auto p = node(Project, std::move(in));
        p->exprs = std::move(exprs);
        return p;
    }
    // Filter(expr) with computed terms (lower_computed_predicate) followed by Select(columns): the helper columns are appended by a
    // GpuProjectStream and dropped again by the fused operator's projection
    static StreamingPlanPtr computed_filter_project(StreamingPlanPtr in, Expr predicate, std::vector<std::string> columns) {
        auto p = node(ComputedFilterProject, std::move(in));
        p->predicate_expr = std::move(predicate);
        p->columns = std::move(columns);
        return p;
    }
    static StreamingPlanPtr limit(StreamingPlanPtr in, size_t n) {
        auto p = node(Limit, std::move(in));
        p->n = n;
        return p;
    }

    // streaming.rs:128-131 (todo!() in the reference), defined by the eager join: the left plan is the build side, the right the
    // probe side (planner.rs:102-108); one output batch per probe batch
    // `type`: Inner, Left, Right, Semi or Anti (execution::join_shape: Left, Semi and Anti swap the sides, so the left plan is then the
    // streamed probe side).  Outer is refused: a trailing batch of unmatched build rows is not built; the eager plan has it.
    static StreamingPlanPtr hash_join(StreamingPlanPtr build, StreamingPlanPtr probe, std::string build_key, std::string probe_key,
                                      JoinType type = JoinType::Inner) {
        if (type == JoinType::Outer)
            throw Error(RV_ERR_UNSUPPORTED, "StreamingPhysicalPlan::hash_join: JoinType::Outer is not streamed (its unmatched build rows belong to no probe "
                                            "batch); use the eager plan, PhysicalPlan::hash_join");
        const execution::JoinShape shape = execution::join_shape(type);
        if (shape.swapped) {
            std::swap(build, probe);
            std::swap(build_key, probe_key);
        }
        auto p = node(HashJoin, std::move(probe));
        p->build_side = std::move(build);
        p->build_key = std::move(build_key);
        p->probe_key = std::move(probe_key);
        p->join_kind = shape.kind;
        return p;
    }

    // group_by(key).agg(aggs): a pipeline breaker that emits exactly one batch (GpuGroupByStream); the reference has no such operator
    static StreamingPlanPtr group_by(StreamingPlanPtr in, std::string key, std::vector<execution::AggSpec> aggs) {
        auto p = node(GroupBy, std::move(in));
        p->group_keys = {std::move(key)};
        p->aggs = std::move(aggs);
        return p;
    }
    // group_by([k0, k1, ...]).agg(aggs): the same over tuples of up to 8 key columns of any dtype (group_by_schema(keys)); the keys come
    // first in the batch
    static StreamingPlanPtr group_by(StreamingPlanPtr in, std::vector<std::string> keys, std::vector<execution::AggSpec> aggs) {
        auto p = node(GroupBy, std::move(in));
        p->group_keys = std::move(keys);
        p->group_by_list = true;
        p->aggs = std::move(aggs);
        return p;
    }
    // sort(keys): a pipeline breaker that emits exactly one batch (GpuSortStream); the reference has no such operator
    static StreamingPlanPtr sort(StreamingPlanPtr in, std::vector<execution::SortKey> keys) {
        auto p = node(Sort, std::move(in));
        p->sort_keys = std::move(keys);
        return p;
    }
    // top_k(keys, k): the first k rows of sort(keys) without sorting the input; a pipeline breaker that emits exactly one batch
    // (GpuTopKStream, which folds the input every `fold_rows` rows).  What a planner makes of Limit(Sort(x)).
    static StreamingPlanPtr top_k(StreamingPlanPtr in, std::vector<execution::SortKey> keys, size_t k, size_t fold_rows = execution::kTopKFoldRows) {
        auto p = node(TopK, std::move(in));
        p->sort_keys = std::move(keys);
        p->top_k_rows = k;
        p->top_k_fold_rows = fold_rows;
        return p;
    }
    // window(partition_by, order_by, exprs): the input's rows in input order with one new column per expression; a pipeline breaker that
    // emits exactly one batch (GpuWindowStream); the reference has no such operator
    static StreamingPlanPtr window(StreamingPlanPtr in, std::vector<std::string> partition_by, std::vector<execution::SortKey> order_by,
                                   std::vector<execution::WindowExpr> exprs) {
        auto p = node(Window, std::move(in));
        p->partition_keys = std::move(partition_by);
        p->sort_keys = std::move(order_by);
        p->window_exprs = std::move(exprs);
        return p;
    }
    // a device context some source of the plan holds (nullptr: none does)
    ContextRef any_context() const {
        if (csv_ctx) return csv_ctx;
        for (auto &c : df.columns)
            if (c->on_device()) return c->context();
        for (auto &b : batches)
            for (auto &c : b.columns())
                if (c->on_device()) return c->context();
        for (const StreamingPlanPtr &p : {input, build_side})
            if (p)
                if (ContextRef c = p->any_context()) return c;
        return nullptr;
    }

    execution::DataStreamRef execute() const {  // streaming.rs:71-133
        using namespace execution;
        try {
            switch (kind) {
                case MemorySource:
                    if (batches.empty()) throw StreamingExecutionError("Invalid operation: Cannot create stream from empty batch list");
                    return std::make_unique<MemoryStream>(batches[0].schema(), batches);
                case DataFrameSource: {  // streaming.rs:85-94: an empty frame gives an empty stream with an empty schema
                    auto b = dataframe_to_batches(df, df_batch_size);
                    auto schema = b.empty() ? std::make_shared<const Schema>() : b[0].schema();
                    return std::make_unique<MemoryStream>(schema, std::move(b));
                }
                case CsvFileSource:
                    try {
                        return std::make_unique<CsvFileStream>(csv_ctx, csv_path, csv_schema, csv_batch_size, csv_delimiter, csv_nulls, csv_scan);
                    } catch (const Error &e) {
                        throw StreamingExecutionError(std::string("Invalid operation: ") + e.what());  // streaming.rs:102-103
                    }
                case Filter: return std::make_unique<FilterStream>(input->execute(), predicate_column);
                case GpuFilterProject:
                    // over a resident frame the chunker and the operator fuse: no per-batch handles (rv_filter_project_chunked)
                    if (input->kind == DataFrameSource && !input->df.columns.empty() && input->df.height() > 0 && input->df_batch_size > 0)
                        return std::make_unique<GpuChunkedFilterProjectStream>(input->df.names, input->filled_columns(), input->df_batch_size, predicate, columns);
                    return std::make_unique<GpuFilterProjectStream>(input->execute(), predicate, columns);
                case Select: return std::make_unique<SelectStream>(input->execute(), columns);
                case Limit: return std::make_unique<LimitStream>(input->execute(), n);
                case Project: {
                    auto in = input->execute();
                    auto lowered = lower_select_exprs(exprs, *in->schema());
                    return std::make_unique<GpuProjectStream>(std::move(in), std::move(lowered));
                }
                case ComputedFilterProject: {  // RV_NULL_DROPS on the helper columns, exactly as on any other column
                    auto in = input->execute();
                    const SchemaRef schema = in->schema();
                    ComputedPredicate lowered = lower_computed_predicate(predicate_expr, *schema);
                    auto widened = std::make_unique<GpuProjectStream>(std::move(in), with_arith_helpers(*schema, lowered.helpers));
                    return std::make_unique<GpuFilterProjectStream>(std::move(widened), std::move(lowered.predicate), columns);
                }
                case HashJoin:  // windows of a resident probe frame, a resident build frame as it is
                    return std::make_unique<GpuHashJoinStream>(build_side->as_input(), input->as_input(), build_key, probe_key, size_t(1) << 28,
                                                               uint64_t(1) << 28, join_kind);
                case GroupBy: return std::make_unique<GpuGroupByStream>(input->as_input(), group_keys, aggs, any_context(), group_by_list);
                case Sort: return std::make_unique<GpuSortStream>(input->as_input(), sort_keys, any_context());
                case Window: return std::make_unique<GpuWindowStream>(input->as_input(), partition_keys, sort_keys, window_exprs, any_context());
                case TopK: return std::make_unique<GpuTopKStream>(input->as_input(), sort_keys, top_k_rows, any_context(), top_k_fold_rows);
            }
        } catch (const StreamError &e) {
            throw StreamingExecutionError(std::string("Stream error: ") + e.what());
        }
        throw Panic("unreachable");
    }
    // dataframe_to_batches' null fill, once per column instead of once per batch (a DataFrameSource)
    std::vector<execution::ArrayRef> filled_columns() const {
        std::vector<execution::ArrayRef> filled;
        for (auto &col : df.columns) {
            rv_dcolumn *f = nullptr;
            check(rv_fill_nulls(col->context()->raw(), col->handle(), &f));
            filled.push_back(execution::Array::adopt(col->context(), f));
        }
        return filled;
    }
    // This node as the input of a join or of a pipeline breaker: a resident frame (a DataFrameSource with a batch size) is taken whole,
    // after the null fill -- an empty frame too: it still has its columns' names and dtypes --, anything else is its stream.
    execution::JoinSide as_input() const {
        execution::JoinSide s;
        if (kind == DataFrameSource && !df.columns.empty() && df_batch_size > 0) {
            s.names = df.names;
            s.columns = filled_columns();
            s.batch_size = df_batch_size;
        } else {
            s.stream = execute();
        }
        return s;
    }
    std::vector<execution::RecordBatch> collect_batches() const {
        auto s = execute();
        try {
            return s->collect();
        } catch (const execution::StreamError &e) {
            throw StreamingExecutionError(std::string("Stream error: ") + e.what());
        }
    }
    // collect(): concat of every batch, or RecordBatch::empty(schema) when the stream yields nothing
    execution::RecordBatch collect(const ContextRef &ctx) const {
        auto s = execute();
        try {
            auto schema = s->schema();
            auto all = s->collect();
            if (all.empty()) return execution::RecordBatch::empty(ctx, schema);
            try {
                return execution::RecordBatch::concat(all);
            } catch (const Error &e) {
                throw StreamingExecutionError(std::string("Conversion error: ") + e.what());
            }
        } catch (const execution::StreamError &e) {
            throw StreamingExecutionError(std::string("Stream error: ") + e.what());
        }
    }

  private:
    static std::shared_ptr<StreamingPhysicalPlan> node(Kind kind, StreamingPlanPtr input = nullptr) {  // what every factory starts from
        auto p = std::make_shared<StreamingPhysicalPlan>();
        p->kind = kind;
        p->input = std::move(input);
        return p;
    }
};

// Eager PhysicalPlan (plan.rs:8-150) over a frame of named, typed device columns.  Filter keeps
// ALL columns and uses the AnyValue ordering for nulls (RV_NULL_IS_LEAST); Select renames.
struct ExecutionError : std::runtime_error {  // plan.rs:36-62
    enum Kind { ColumnNotFound, InvalidOperation, General } kind;
    ExecutionError(Kind k, const std::string &m) : std::runtime_error(m), kind(k) {}
};
class PhysicalPlan;
using PhysicalPlanPtr = std::shared_ptr<const PhysicalPlan>;
class PhysicalPlan {
  public:
    enum Kind { DataFrameSource, Select, Filter, HashJoin, Project, ComputedFilter, GroupBy, Sort, TopK, Window } kind = DataFrameSource;
    DeviceFrame df;
    std::vector<Expr> exprs;  // Project: select expressions, arithmetic included
    Expr predicate_expr;      // ComputedFilter: `<arith> <cmp> <literal>` terms, alone or under AND / OR
    PhysicalPlanPtr input;
    std::vector<std::string> columns, final_names;
    CompareTerm term;  // Filter { column, value, op }
    PhysicalPlanPtr build_side;          // HashJoin { build_side, probe_side = input, build_key, probe_key, join_kind }: the sides as joined
    rv_join_kind join_kind = RV_JOIN_INNER;
    std::string build_key, probe_key;
    std::vector<std::string> group_keys;  // GroupBy { input, group_keys, aggs }: the key list, or the one key of the single-key form
    bool group_by_list = false;           // ... which of the two forms
    std::vector<execution::AggSpec> aggs;
    std::vector<execution::SortKey> sort_keys;  // Sort { input, sort_keys }, TopK { input, sort_keys, top_k_rows }
    size_t top_k_rows = 0;
    std::vector<std::string> partition_keys;  // Window { input, partition_keys, sort_keys (the window order), window_exprs }
    std::vector<execution::WindowExpr> window_exprs;

    static PhysicalPlanPtr source(DeviceFrame f) {
        auto p = node(DataFrameSource);
        p->df = std::move(f);
        return p;
    }
    static PhysicalPlanPtr filter(PhysicalPlanPtr in, CompareTerm t) {
        auto p = node(Filter, std::move(in));
        p->term = std::move(t);
        return p;
    }
    static PhysicalPlanPtr select(PhysicalPlanPtr in, std::vector<std::string> cols, std::vector<std::string> finals) {
        auto p = node(Select, std::move(in));
        p->columns = std::move(cols);
        p->final_names = std::move(finals);
        return p;
    }
    // Select whose expressions may be arithmetic (lower_select_exprs): plain columns pass through as Select passes them, computed
    // ones are one rv_eval_arith each
    static PhysicalPlanPtr project(PhysicalPlanPtr in, std::vector<Expr> exprs) {
        auto p = node(Project, std::move(in));
        p->exprs = std::move(exprs);
        return p;
    }
    // Filter over computed terms (lower_computed_predicate): every column kept, AnyValue ordering for nulls -- on the helper
    // columns as on any other
    static PhysicalPlanPtr computed_filter(PhysicalPlanPtr in, Expr predicate) {
        auto p = node(ComputedFilter, std::move(in));
        p->predicate_expr = std::move(predicate);
        return p;
    }
    // planner.rs:102-108: the left frame is the build side, the right frame the probe side -- for Inner, Right and Outer; Left, Semi
    // and Anti swap the sides (execution::join_shape), so their output starts with the left frame's columns
    static PhysicalPlanPtr hash_join(PhysicalPlanPtr build, PhysicalPlanPtr probe, std::string build_key, std::string probe_key,
                                     JoinType type = JoinType::Inner) {
        const execution::JoinShape shape = execution::join_shape(type);
        if (shape.swapped) {
            std::swap(build, probe);
            std::swap(build_key, probe_key);
        }
        auto p = node(HashJoin, std::move(probe));
        p->build_side = std::move(build);
        p->build_key = std::move(build_key);
        p->probe_key = std::move(probe_key);
        p->join_kind = shape.kind;
        return p;
    }
    // group_by(key).agg(aggs), eager: one rv_hash_aggregate; the key under its own name, then every aggregate under its name, the
    // groups in the order of their first rows.  The nulls of the frame stay nulls (no fill: this is not a stream).
    static PhysicalPlanPtr group_by(PhysicalPlanPtr in, std::string key, std::vector<execution::AggSpec> aggs) {
        auto p = node(GroupBy, std::move(in));
        p->group_keys = {std::move(key)};
        p->aggs = std::move(aggs);
        return p;
    }
    // group_by([k0, k1, ...]).agg(aggs), eager: one rv_hash_aggregate_keys over tuples of up to 8 key columns -- Int64, Float64, Boolean,
    // String or Null, each with its nulls; the keys under their own names in the order given, then the aggregates.  The list with one
    // name is how a Float64 or Boolean key is grouped.
    static PhysicalPlanPtr group_by(PhysicalPlanPtr in, std::vector<std::string> keys, std::vector<execution::AggSpec> aggs) {
        auto p = node(GroupBy, std::move(in));
        p->group_keys = std::move(keys);
        p->group_by_list = true;
        p->aggs = std::move(aggs);
        return p;
    }
    // sort(keys), eager: one rv_sort; names and dtypes unchanged, the first key the most significant, equal rows in input order.  The nulls
    // of the frame stay nulls (no fill: this is not a stream).
    static PhysicalPlanPtr sort(PhysicalPlanPtr in, std::vector<execution::SortKey> keys) {
        auto p = node(Sort, std::move(in));
        p->sort_keys = std::move(keys);
        return p;
    }
    // top_k(keys, k), eager: one rv_top_k -- the first min(k, rows) rows of sort(keys), without sorting the frame
    static PhysicalPlanPtr top_k(PhysicalPlanPtr in, std::vector<execution::SortKey> keys, size_t k) {
        auto p = node(TopK, std::move(in));
        p->sort_keys = std::move(keys);
        p->top_k_rows = k;
        return p;
    }
    // window(partition_by, order_by, exprs), eager: one rv_window -- the frame as it is, rows in place, with one new column per expression
    // appended under its alias.  The nulls of the frame stay nulls (no fill: this is not a stream).
    static PhysicalPlanPtr window(PhysicalPlanPtr in, std::vector<std::string> partition_by, std::vector<execution::SortKey> order_by,
                                  std::vector<execution::WindowExpr> exprs) {
        auto p = node(Window, std::move(in));
        p->partition_keys = std::move(partition_by);
        p->sort_keys = std::move(order_by);
        p->window_exprs = std::move(exprs);
        return p;
    }
    DeviceFrame execute() const {
        switch (kind) {
            case DataFrameSource: return df;  // plan.rs:67
            case Window: {
                DeviceFrame in = input->execute();
                const execution::Schema schema = frame_schema(in);
                const execution::SchemaRef out_schema = execution::window_schema(schema, partition_keys, sort_keys, window_exprs);  // the planning errors
                if (in.columns.empty()) throw Error(RV_ERR_INVALID_ARG, "window: the frame has no columns");
                DeviceFrame out = in;
                for (auto &c : execution::window_columns(in.columns[0]->context(), schema, in.columns, partition_keys, sort_keys, window_exprs)) out.columns.push_back(c);
                out.names.clear();
                for (auto &f : out_schema->fields()) out.names.push_back(f.name());
                return out;
            }
            case TopK: {
                DeviceFrame in = input->execute();
                const execution::Schema schema = frame_schema(in);
                (void)execution::top_k_schema(schema, sort_keys, top_k_rows);  // the planning errors
                if (in.height() == 0) return in;
                DeviceFrame out;
                out.names = in.names;
                out.columns = execution::top_k_columns((*in.column(sort_keys[0].column))->context(), schema, in.columns, sort_keys, top_k_rows);
                return out;
            }
            case Sort: {
                DeviceFrame in = input->execute();
                const execution::Schema schema = frame_schema(in);
                (void)execution::sort_schema(schema, sort_keys);  // the planning errors
                if (in.height() == 0) return in;
                DeviceFrame out;
                out.names = in.names;
                out.columns = execution::sort_columns((*in.column(sort_keys[0].column))->context(), schema, in.columns, sort_keys);
                return out;
            }
            case GroupBy: {
                DeviceFrame in = input->execute();
                const execution::Schema schema = frame_schema(in);
                const execution::SchemaRef out_schema = execution::group_by_schema(schema, group_keys, aggs, group_by_list);  // the planning errors
                DeviceFrame out;
                out.columns = execution::group_by_columns((*in.column(group_keys[0]))->context(), schema, in.columns, group_keys, aggs, group_by_list);
                for (auto &f : out_schema->fields()) out.names.push_back(f.name());
                return out;
            }
            case Select: {                     // plan.rs:68-96
                DeviceFrame in = input->execute();
                DeviceFrame out;
                for (auto &c : columns)
                    if (!in.column(c)) throw ExecutionError(ExecutionError::ColumnNotFound, "Column not found: '" + c + "'");
                for (size_t i = 0; i < columns.size() && i < final_names.size(); ++i) {
                    out.names.push_back(final_names[i]);
                    out.columns.push_back(*in.column(columns[i]));
                }
                return out;
            }
            case Filter: {  // plan.rs:97-150: mask over one column, every column kept
                DeviceFrame in = input->execute();
                const auto pred_col = in.index_of(term.column);
                if (!pred_col) throw ExecutionError(ExecutionError::ColumnNotFound, "Column not found: '" + term.column + "'");
                const std::vector<const rv_dcolumn *> cols = execution::column_handles(in.columns, "String columns are outside the device path");
                std::vector<uint32_t> proj;
                for (uint32_t i = 0; i < cols.size(); ++i) proj.push_back(i);
                rv_term t = execution::to_rv_term(term, static_cast<uint32_t>(*pred_col));
                rv_predicate pred{&t, 1, RV_NULL_IS_LEAST, nullptr, 0};
                std::vector<rv_dcolumn *> out(cols.size(), nullptr);
                uint64_t rows = 0;
                const ContextRef ctx = in.columns[*pred_col]->context();
                check(rv_filter_project(ctx->raw(), cols.data(), static_cast<uint32_t>(cols.size()), &pred, proj.data(),
                                        static_cast<uint32_t>(proj.size()), out.data(), &rows, nullptr));
                return DeviceFrame{in.names, execution::adopt_columns(ctx, out)};
            }
            case Project: {
                DeviceFrame in = input->execute();
                const auto lowered = lower_select_exprs(exprs, frame_schema(in));
                auto missing = [](const std::string &c) { throw ExecutionError(ExecutionError::ColumnNotFound, "Column not found: '" + c + "'"); };
                auto column = [&](const std::string &c) { return in.column(c); };
                for (auto &o : lowered) {  // as Select: every name is checked before anything is built
                    if (!o.computed() && !in.column(o.source)) missing(o.source);
                    for (auto &s : o.program)
                        if (s.op == RV_ARITH_COL && !in.column(s.column)) missing(s.column);
                }
                DeviceFrame out;
                for (auto &o : lowered) {
                    out.names.push_back(o.name);
                    out.columns.push_back(o.computed() ? execution::eval_arith(o.program, column, missing) : *in.column(o.source));
                }
                return out;
            }
            case ComputedFilter: {  // helper columns behind the frame's, one rv_filter_project, the helpers left out of its projection
                DeviceFrame in = input->execute();
                if (in.columns.empty()) throw Error(RV_ERR_INVALID_ARG, "filter over a frame without columns");
                const execution::ComputedPredicate lowered = lower_computed_predicate(predicate_expr, frame_schema(in));
                auto missing = [](const std::string &c) { throw ExecutionError(ExecutionError::ColumnNotFound, "Column not found: '" + c + "'"); };
                auto column = [&](const std::string &c) { return in.column(c); };
                std::vector<std::string> names = in.names;
                std::vector<execution::ArrayRef> helpers;
                for (auto &h : lowered.helpers) {
                    helpers.push_back(execution::eval_arith(h.program, column, missing));
                    names.push_back(h.name);
                }
                std::vector<const rv_dcolumn *> cols = execution::column_handles(in.columns);
                std::vector<uint32_t> proj;
                for (uint32_t i = 0; i < in.columns.size(); ++i) proj.push_back(i);
                for (auto &h : helpers) cols.push_back(h->handle());
                std::vector<rv_term> terms;
                for (auto &t : lowered.predicate.terms) {
                    const auto at = std::find(names.begin(), names.end(), t.column);
                    if (at == names.end()) missing(t.column);  // a plain term beside the computed ones that names no column of the frame
                    terms.push_back(execution::to_rv_term(t, static_cast<uint32_t>(at - names.begin())));
                }
                const auto &expr = lowered.predicate.expr;
                rv_predicate pred{terms.data(), static_cast<uint32_t>(terms.size()), RV_NULL_IS_LEAST, expr.empty() ? nullptr : expr.data(),
                                  static_cast<uint32_t>(expr.size())};
                const ContextRef ctx = in.columns[0]->context();
                std::vector<rv_dcolumn *> out(proj.size(), nullptr);
                uint64_t rows = 0;
                check(rv_filter_project(ctx->raw(), cols.data(), static_cast<uint32_t>(cols.size()), &pred, proj.data(), static_cast<uint32_t>(proj.size()),
                                        out.data(), &rows, nullptr));
                return DeviceFrame{in.names, execution::adopt_columns(ctx, out)};
            }
            case HashJoin: {  // plan.rs:174-207 (JoinType::Inner), one rv_hash_join; the other kinds one rv_hash_join_kind
                DeviceFrame b = build_side->execute();
                const auto build_at = b.index_of(build_key);
                if (!build_at) throw Panic("called `Option::unwrap()` on a `None` value");  // plan.rs:184: build_df.column(..).unwrap()
                DeviceFrame p = input->execute();
                const auto probe_at = p.index_of(probe_key);
                if (!probe_at) throw Panic("called `Option::unwrap()` on a `None` value");  // plan.rs:195
                const uint32_t bki = static_cast<uint32_t>(*build_at), pki = static_cast<uint32_t>(*probe_at);
                const execution::ArrayRef &bk = b.columns[bki], &pk = p.columns[pki];
                std::vector<const rv_dcolumn *> bcols = execution::column_handles(b.columns), pcols = execution::column_handles(p.columns);
                // String keys go through the string dictionary: ids in place of the build key, a helper column as the probe key
                const ContextRef ctx = pk->context();
                execution::StringKeyEncoder string_keys(bk->data_type(), pk->data_type());
                const execution::ArrayRef build_ids = string_keys.build_key(bk), helper = string_keys.probe_key(ctx, pk);
                if (build_ids) bcols[bki] = build_ids->handle();
                // a full outer join returns the build key: the strings, carried as one more build column, not their ids
                const bool carried_key = build_ids && join_kind == RV_JOIN_FULL_OUTER;
                if (carried_key) bcols.push_back(bk->handle());
                const execution::ProbeColumns probe = execution::with_key_helper(std::move(pcols), pki, helper);
                const bool probe_only = join_kind == RV_JOIN_PROBE_SEMI || join_kind == RV_JOIN_PROBE_ANTI;
                const size_t nout = probe_only ? probe.cols.size() : probe.cols.size() + bcols.size() - (join_kind == RV_JOIN_FULL_OUTER ? 0 : 1);
                std::vector<rv_dcolumn *> out(nout, nullptr);
                uint64_t rows = 0;
                if (join_kind == RV_JOIN_INNER)
                    check(rv_hash_join(ctx->raw(), bcols.data(), static_cast<uint32_t>(bcols.size()), bki, probe.cols.data(),
                                       static_cast<uint32_t>(probe.cols.size()), probe.key, out.data(), &rows));
                else
                    check(rv_hash_join_kind(ctx->raw(), bcols.data(), static_cast<uint32_t>(bcols.size()), bki, probe.cols.data(),
                                            static_cast<uint32_t>(probe.cols.size()), probe.key, join_kind, out.data(), &rows));
                DeviceFrame res{{}, execution::adopt_columns(ctx, out)};
                if (carried_key) execution::restore_build_key(res.columns, probe.cols.size(), bki);
                execution::without_key_helper(probe, res.columns);  // the helper column's pairs: not part of the frame
                for (auto &f : execution::join_output_fields(frame_schema(p), frame_schema(b), bki, join_kind)) res.names.push_back(f.name());
                return res;
            }
        }
        throw Panic("unreachable");
    }

  private:
    static std::shared_ptr<PhysicalPlan> node(Kind kind, PhysicalPlanPtr input = nullptr) {  // what every factory starts from
        auto p = std::make_shared<PhysicalPlan>();
        p->kind = kind;
        p->input = std::move(input);
        return p;
    }
};

}  // namespace physical_plan
}  // namespace rivulus
