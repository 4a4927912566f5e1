// The device CSV scan (rv_csv_open / rv_csv_next, CsvFileStream with CsvScan::Device) against the host CsvFileStream and
// the oracle's rvo::CsvFileStream, call by call: the same batches (rows, values bit for bit, bitmaps, null counts) and the
// same errors at the same calls, in both CsvNulls modes.
//   csv_device_tests [tmp_dir]     every case (needs an MI355X)
// Output: "ok <name>" / "FAIL <name>: why"; exit status 0 iff all pass.
#include <algorithm>
#include <cstring>
#include <random>

#include "../../oracle/oracle_csv.hpp"
#include "../../rivulus_amd/csrc/csv_parse.hpp"
#define HOST_TEST_ARG_DEFAULT "/tmp"
#include "host_test_main.hpp"

using namespace rivulus;
using namespace rivulus::execution;

namespace {
std::string write_file(const std::string &name, const std::string &text) {
    const std::string path = g_arg + "/" + name;
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) throw Fail("cannot write " + path);
    std::fwrite(text.data(), 1, text.size(), f);
    std::fclose(f);
    return path;
}

// the device reader with an explicit chunk size, wrapped as the host layer wraps it
class DeviceCsv {
  public:
    DeviceCsv(const std::string &path, SchemaRef schema, size_t batch, char delim, CsvNulls nulls, uint64_t chunk) : schema_(std::move(schema)) {
        std::vector<rv_dtype> types;
        for (auto &f : schema_->fields()) types.push_back(to_rv(f.data_type()));
        check(rv_csv_open(ctx()->raw(), path.c_str(), types.data(), static_cast<uint32_t>(types.size()), static_cast<unsigned char>(delim), batch,
                          nulls == CsvNulls::AsReference ? RV_CSV_NULLS_AS_REFERENCE : 0u, chunk, &r_));
    }
    ~DeviceCsv() { rv_csv_close(r_); }
    std::optional<RecordBatch> next_batch() {
        const size_t n = schema_->num_fields();
        std::vector<rv_dcolumn *> out(std::max<size_t>(n, 1));
        uint64_t rows = 0;
        const rv_status s = rv_csv_next(r_, out.data(), &rows);
        if (s == RV_ERR_PARSE) throw StreamError::execution(std::string("Parse error: ") + rv_last_error());
        check(s);
        if (rows == 0) return std::nullopt;
        std::vector<ArrayRef> cols;
        for (size_t c = 0; c < n; ++c) cols.push_back(Array::adopt(ctx(), out[c]));
        return RecordBatch::try_new(schema_, std::move(cols));
    }
    rv_csv_reader *raw() const { return r_; }

  private:
    SchemaRef schema_;
    rv_csv_reader *r_ = nullptr;
};

// every bit of a device column's logical range
struct Dump {
    rv_column_info info{};
    uint64_t nulls = 0;
    std::vector<uint8_t> values, validity;
    std::vector<int32_t> offsets;
};
Dump dump(const ArrayRef &a) {
    Dump d;
    rv_ctx *c = ctx()->raw();
    check(rv_column_info_get(c, a->handle(), &d.info));
    check(rv_null_count(c, a->handle(), &d.nulls));
    const uint64_t n = d.info.length, nb = (n + 7) / 8;
    int hv = 0;
    d.validity.assign(std::max<uint64_t>(nb, 1), 0);
    if (d.info.dtype == RV_STRING) {
        d.offsets.resize(n + 1);
        d.values.resize(std::max<uint64_t>(d.info.data_bytes, 1));
        check(rv_download_string(c, a->handle(), d.offsets.data(), d.values.data(), d.validity.data(), &hv));
        d.values.resize(d.info.data_bytes);
    } else {
        d.values.assign(std::max<uint64_t>(d.info.dtype == RV_BOOLEAN ? nb : n * 8, 1), 0);
        check(rv_download(c, a->handle(), d.values.data(), d.validity.data(), &hv));
        if (d.info.dtype == RV_BOOLEAN && n % 8) d.values[nb - 1] &= static_cast<uint8_t>((1u << (n % 8)) - 1);
    }
    if (!hv) d.validity.clear();
    else if (n % 8) d.validity[nb - 1] &= static_cast<uint8_t>((1u << (n % 8)) - 1);
    return d;
}
std::string diff_batches(const RecordBatch &h, const RecordBatch &d) {
    if (h.num_rows() != d.num_rows()) return "rows " + std::to_string(h.num_rows()) + " != " + std::to_string(d.num_rows());
    if (h.num_columns() != d.num_columns()) return "columns";
    for (size_t c = 0; c < h.num_columns(); ++c) {
        const Dump x = dump(h.column(c)), y = dump(d.column(c));
        const std::string col = "column " + std::to_string(c) + ": ";
        if (x.info.dtype != y.info.dtype) return col + "dtype";
        if (x.info.has_validity != y.info.has_validity) return col + "bitmap present " + std::to_string(x.info.has_validity) + " vs " + std::to_string(y.info.has_validity);
        if (x.nulls != y.nulls) return col + "null count " + std::to_string(x.nulls) + " vs " + std::to_string(y.nulls);
        if (x.validity != y.validity) return col + "bitmap bits";
        if (x.values != y.values) return col + "values";
        if (x.offsets != y.offsets) return col + "offsets";
    }
    return "";
}

// one call of each stream: a batch, the end, or an error text
struct Step {
    std::optional<RecordBatch> batch;
    std::string error;
};
template <class S>
Step step(S &s) {
    Step r;
    try {
        r.batch = s.next_batch();
    } catch (const std::exception &e) {
        r.error = e.what();
        if (r.error.empty()) r.error = "?";
    }
    return r;
}

rvo::SchemaRef oracle_schema(const Schema &s) {
    std::vector<rvo::Field> f;
    for (auto &x : s.fields()) f.push_back({x.name(), static_cast<rvo::DataType>(static_cast<int>(x.data_type())), true});
    return std::make_shared<rvo::Schema>(f);
}

// the oracle's batch as the host layer's arrays would hold it (value-level comparison, CsvNulls::AsReference only)
std::string diff_oracle(const rvo::RecordBatch &o, const RecordBatch &d) {
    if (o.num_rows() != d.num_rows()) return "oracle rows " + std::to_string(o.num_rows()) + " != " + std::to_string(d.num_rows());
    for (size_t c = 0; c < d.num_columns(); ++c) {
        const ArrayRef &a = d.column(c);
        const rvo::ArrayRef &b = o.column(c);
        if (a->null_count() != b->null_count()) return "oracle null count, column " + std::to_string(c);
        for (size_t i = 0; i < a->len(); ++i) {
            bool eq = true;
            switch (a->data_type()) {
                case DataType::Int64:
                    eq = std::dynamic_pointer_cast<const Int64Array>(a)->value(i) == std::static_pointer_cast<const rvo::Int64Array>(b)->value(i);
                    break;
                case DataType::Float64: {
                    auto x = std::dynamic_pointer_cast<const Float64Array>(a)->value(i);
                    auto y = std::static_pointer_cast<const rvo::Float64Array>(b)->value(i);
                    eq = x.has_value() == y.has_value() && (!x || (std::isnan(*x) && std::isnan(*y)) || std::memcmp(&*x, &*y, 8) == 0);
                    break;
                }
                case DataType::String:
                    eq = std::dynamic_pointer_cast<const StringArray>(a)->value(i) == std::static_pointer_cast<const rvo::StringArray>(b)->value(i);
                    break;
                default:
                    eq = std::dynamic_pointer_cast<const BooleanArray>(a)->value(i) == std::static_pointer_cast<const rvo::BooleanArray>(b)->value(i);
            }
            if (!eq) return "oracle value, column " + std::to_string(c) + " row " + std::to_string(i);
        }
    }
    return "";
}

struct Stats {
    size_t batches = 0, errors = 0, rows = 0;
};

// host stream, device stream (and, under AsReference, the oracle) call by call until all three end
Stats compare(const std::string &path, SchemaRef schema, std::optional<size_t> batch, char delim, CsvNulls nulls, uint64_t chunk,
              bool through_host_layer = false) {
    CsvFileStream host(ctx(), path, schema, batch, delim, nulls);
    std::unique_ptr<DeviceCsv> dev_raw;
    std::unique_ptr<CsvFileStream> dev_layer;
    if (through_host_layer) dev_layer = std::make_unique<CsvFileStream>(ctx(), path, schema, batch, delim, nulls, CsvScan::Device);
    else dev_raw = std::make_unique<DeviceCsv>(path, schema, batch ? *batch : 0, delim, nulls, chunk);
    std::optional<rvo::CsvFileStream> ora;
    if (nulls == CsvNulls::AsReference) ora.emplace(path, oracle_schema(*schema), batch, delim);
    Stats st;
    for (size_t call = 0;; ++call) {
        const std::string at = "call " + std::to_string(call) + ": ";
        Step h = step(host);
        Step d = through_host_layer ? step(*dev_layer) : step(*dev_raw);
        if (h.error != d.error) throw Fail(at + "error '" + h.error + "' vs '" + d.error + "'");
        if (h.batch.has_value() != d.batch.has_value()) throw Fail(at + (h.batch ? "device ended early" : "device has an extra batch"));
        if (h.batch) {
            const std::string why = diff_batches(*h.batch, *d.batch);
            if (!why.empty()) throw Fail(at + why);
        }
        if (ora) {
            std::optional<rvo::RecordBatch> ob;
            std::string oe;
            try {
                ob = ora->next_batch();
            } catch (const std::exception &e) {
                oe = e.what();
            }
            if (oe != d.error) throw Fail(at + "oracle error '" + oe + "' vs '" + d.error + "'");
            if (ob.has_value() != d.batch.has_value()) throw Fail(at + "oracle end");
            if (ob) {
                const std::string why = diff_oracle(*ob, *d.batch);
                if (!why.empty()) throw Fail(at + why);
            }
        }
        if (!h.error.empty()) {
            ++st.errors;
            continue;
        }
        if (!h.batch) break;
        ++st.batches;
        st.rows += h.batch->num_rows();
        if (call > 1000000) throw Fail("no end");
    }
    return st;
}

// ---- random files --------------------------------------------------------------------------------------------------
struct Gen {
    std::mt19937_64 rng;
    explicit Gen(uint64_t seed) : rng(seed) {}
    uint64_t u(uint64_t n) { return rng() % n; }
    char delim = ',';
    std::string pad(const std::string &s) {  // padding the trim removes (no tab where the tab is the delimiter)
        static const char *sp[] = {"", "", "", " ", "  ", "\t", " \t "};
        const int k = delim == '\t' ? 5 : 7;
        return std::string(sp[u(k)]) + s + sp[u(k)];
    }
    std::string cell(DataType t, bool allow_bad) {
        const uint64_t r = u(100);
        if (r < 6) return pad(u(2) ? "null" : "");
        if (allow_bad && r < 7) return pad(t == DataType::String ? "x" : "b@d");
        char buf[64];
        switch (t) {
            case DataType::Int64: {
                const uint64_t k = u(10);
                if (k == 0) return pad(u(2) ? "9223372036854775807" : "-9223372036854775808");
                if (k == 1) return pad("+" + std::to_string(u(1000)));
                if (k == 2) return pad("00" + std::to_string(u(1000)));
                return pad(std::to_string(static_cast<int64_t>(rng()) >> u(64)));
            }
            case DataType::Float64: {
                const uint64_t k = u(20);
                static const char *sp[] = {"inf", "-inf", "NaN", "-nan", "Infinity", "-0.0", "0", ".5", "5.", "1e308", "2.4703282292062328e-324",
                                           "1.7976931348623157e308", "1e-400", "123456789012345678901234567890e-20", "0.30000000000000004"};
                if (k == 0) return pad(sp[u(15)]);
                uint64_t b = rng();
                double d;
                std::memcpy(&d, &b, 8);
                if (!std::isfinite(d) || k < 10) d = static_cast<double>(static_cast<int64_t>(rng() % 2000000) - 1000000) / 1000.0;
                std::snprintf(buf, sizeof buf, k % 3 == 0 ? "%.17g" : (k % 3 == 1 ? "%.6e" : "%.3f"), d);
                return pad(buf);
            }
            case DataType::Boolean: {
                static const char *b[] = {"true", "false", "TRUE", "False", "t", "F", "1", "0"};
                return pad(b[u(8)]);
            }
            default: {
                std::string s;
                const size_t n = 1 + u(12);
                for (size_t i = 0; i < n; ++i) {
                    uint8_t c;
                    const uint64_t k = u(10);
                    if (k == 0) c = static_cast<uint8_t>(0x80 + u(128));  // non-ASCII bytes
                    else if (k == 1) c = ' ';
                    else c = static_cast<uint8_t>('a' + u(26));
                    if (c == static_cast<uint8_t>(delim)) c = 'z';
                    s.push_back(static_cast<char>(c));
                }
                if (s == "null") s = "nul";
                return pad(s);
            }
        }
    }
    std::string file(const Schema &schema, size_t rows, char delim_, int bad_lines, bool crlf, bool trailing_newline) {
        delim = delim_;
        std::string out;
        const char *eol = crlf ? "\r\n" : "\n";
        for (size_t c = 0; c < schema.num_fields(); ++c) out += (c ? std::string(1, delim) : "") + schema.field(c).name();
        out += eol;
        std::vector<size_t> bad;
        for (int k = 0; k < bad_lines; ++k) bad.push_back(u(rows + 1));
        for (size_t r = 0; r < rows; ++r) {
            const uint64_t k = u(100);
            if (k < 3) out += eol;                                  // blank line
            else if (k < 5) out += std::string(" \t ") + eol;       // whitespace only
            const bool is_bad = std::find(bad.begin(), bad.end(), r) != bad.end();
            size_t ncells = schema.num_fields();
            if (is_bad && u(2)) ncells = ncells + (u(2) ? 1 : size_t(-1));  // a field too many / too few
            for (size_t c = 0; c < ncells && c < schema.num_fields() + 1; ++c) {
                if (c) out += delim;
                out += cell(c < schema.num_fields() ? schema.field(c).data_type() : DataType::Int64, is_bad);
            }
            if (r + 1 < rows || trailing_newline) out += eol;
        }
        return out;
    }
};

SchemaRef schema_of(const std::vector<DataType> &t) {
    std::vector<Field> f;
    for (size_t i = 0; i < t.size(); ++i) f.emplace_back("c" + std::to_string(i), t[i], true);
    return std::make_shared<Schema>(f);
}

const std::vector<std::vector<DataType>> kSchemas = {
    {DataType::Int64, DataType::String, DataType::Float64, DataType::Boolean},
    {DataType::Float64},
    {DataType::String, DataType::String, DataType::Int64},
    {DataType::Boolean, DataType::Int64, DataType::Float64, DataType::Float64, DataType::String, DataType::Boolean},
};
}  // namespace

GPU_TEST(random_files_every_dtype_both_null_modes) {
    int file_no = 0;
    for (uint64_t seed = 1; seed <= 6; ++seed) {
        Gen g(seed);
        const auto &types = kSchemas[seed % kSchemas.size()];
        const char delim = ",;\t"[seed % 3];
        const auto schema = schema_of(types);
        const size_t rows = 200 + g.u(3000);
        const std::string path = write_file("rand" + std::to_string(file_no++) + ".csv", g.file(*schema, rows, delim, 0, seed % 2, seed % 3 != 0));
        for (CsvNulls nulls : {CsvNulls::AsReference, CsvNulls::AsIntended})
            for (std::optional<size_t> batch : {std::optional<size_t>(), std::optional<size_t>(97), std::optional<size_t>(1)}) {
                if (batch && *batch == 1 && rows > 1000) continue;
                const Stats st = compare(path, schema, batch, delim, nulls, 0);
                CHECK(st.rows > 0 && st.errors == 0);
            }
        std::remove(path.c_str());
    }
}

GPU_TEST(small_chunks_cut_lines_and_batches) {
    Gen g(77);
    const auto schema = schema_of(kSchemas[0]);
    const std::string path = write_file("chunks.csv", g.file(*schema, 5000, ',', 0, true, false));
    for (uint64_t chunk : {16ull, 100ull, 1000ull, 4096ull, 65536ull})
        for (std::optional<size_t> batch : {std::optional<size_t>(50), std::optional<size_t>(1000), std::optional<size_t>()}) {
            const Stats st = compare(path, schema, batch, ',', CsvNulls::AsReference, chunk);
            CHECK(st.rows > 4000);
        }
    std::remove(path.c_str());
}

GPU_TEST(several_bad_lines_interleave_like_the_host) {
    for (uint64_t seed = 11; seed <= 14; ++seed) {
        Gen g(seed);
        const auto schema = schema_of(kSchemas[seed % kSchemas.size()]);
        const std::string path = write_file("bad.csv", g.file(*schema, 3000, ',', 12, seed % 2, true));
        size_t errors = 0;
        for (uint64_t chunk : {0ull, 777ull})
            for (std::optional<size_t> batch : {std::optional<size_t>(64), std::optional<size_t>(5), std::optional<size_t>()})
                for (CsvNulls nulls : {CsvNulls::AsReference, CsvNulls::AsIntended}) errors += compare(path, schema, batch, ',', nulls, chunk).errors;
        CHECK(errors > 0);
        std::remove(path.c_str());
    }
    // the reference's two texts
    const auto schema = schema_of({DataType::Int64, DataType::String, DataType::Float64, DataType::Boolean});
    const std::string path = write_file("texts.csv", "a,b,c,d\n1,x,1.5,true\nx2,y,2,false\n3,z\n4,w,4.5,maybe\n");
    DeviceCsv d(path, schema, 100, ',', CsvNulls::AsReference, 0);
    std::string e1, e2, e3;
    try {
        d.next_batch();
    } catch (const std::exception &e) {
        e1 = e.what();
    }
    try {
        d.next_batch();
    } catch (const std::exception &e) {
        e2 = e.what();
    }
    try {
        d.next_batch();
    } catch (const std::exception &e) {
        e3 = e.what();
    }
    CHECK(e1 == "Stream execution error: Parse error: Line 3, field 0: Cannot parse 'x2' as Int64");
    CHECK(e2 == "Stream execution error: Parse error: Line 4: Expected 4 fields, found 2");
    CHECK(e3 == "Stream execution error: Parse error: Line 5, field 3: Cannot parse 'maybe' as Boolean");
    CHECK(!d.next_batch().has_value());
    std::remove(path.c_str());
}

int64_t ctx_counter(const char *key) {
    int64_t v = 0;
    check(rv_ctx_get_option(ctx()->raw(), key, &v));
    return v;
}

// Float64 cells Eisel-Lemire cannot round: near and exact halfway points between two doubles, and exact halfway points
// followed by more than 768 digits (the slow path's digit buffer: a truncated tail decides the rounding)
GPU_TEST(float_cells_only_the_slow_path_decides) {
    std::mt19937_64 rng(2024);
    auto pick = [&](uint64_t n) { return rng() % n; };
    char buf[512];
    std::string text = "a,b,c\n";
    uint64_t slow_cells = 0, rows = 0;
    auto slow = [](const std::string &s) {
        double v;
        return rvcsv::parse_f64(reinterpret_cast<const uint8_t *>(s.data()), static_cast<uint32_t>(s.size()), &v) == rvcsv::kF64Slow;
    };
    for (int r = 0; r < 4000; ++r) {
        std::string cells[2];
        for (auto &cell : cells) {
            const uint64_t k = pick(10);
            // a double m * 2^e with a short exact decimal expansion of the midpoint to its upper neighbour
            const double d = std::ldexp(static_cast<double>((rng() >> 11) | 1), static_cast<int>(pick(120)) - 110);
            const long double mid = (static_cast<long double>(d) + static_cast<long double>(std::nextafter(d, INFINITY))) / 2;
            if (k < 4) {  // near halfway, 20-40 digits
                std::snprintf(buf, sizeof buf, "%.*Le", 19 + static_cast<int>(pick(21)), mid);
                cell = buf;
            } else if (k < 7) {  // exactly halfway (every digit), maybe a zero tail past 768 digits, maybe a 1 after it
                std::snprintf(buf, sizeof buf, "%.200Le", mid);
                std::string s = buf;
                const size_t e = s.find('e');
                std::string mant = s.substr(0, e), ex = s.substr(e);
                while (mant.back() == '0') mant.pop_back();
                if (pick(2)) mant += std::string(800, '0') + (pick(2) ? "1" : "");
                cell = mant + ex;
            } else if (k < 8) {
                cell = "null";
            } else {
                std::snprintf(buf, sizeof buf, "%.17g", d);
                cell = buf;
            }
            if (cell != "null" && pick(2)) cell = "-" + cell;
            slow_cells += slow(cell);
        }
        text += cells[0] + "," + std::to_string(r) + "," + cells[1] + "\n";
        ++rows;
    }
    CHECK(slow_cells > 1000);
    const std::string path = write_file("slow.csv", text);
    const auto schema = schema_of({DataType::Float64, DataType::Int64, DataType::Float64});
    // one chunk (the file is small): every undecided cell goes through csv_f64_slow exactly once
    const int64_t before = ctx_counter("csv_slow_cells");
    CHECK(compare(path, schema, 97, ',', CsvNulls::AsReference, 0).rows == rows);
    CHECK(ctx_counter("csv_slow_cells") - before == static_cast<int64_t>(slow_cells));
    compare(path, schema, std::nullopt, ',', CsvNulls::AsIntended, 0);
    compare(path, schema, 500, ',', CsvNulls::AsReference, 20000);  // many chunks, carried rows parsed again
    // a first list too small for the chunk's undecided cells: the chunk is parsed again with a list of the exact size
    const int64_t reparses = ctx_counter("csv_slow_reparses");
    check(rv_ctx_set_option(ctx()->raw(), "csv_slow_cap", 5));
    try {
        compare(path, schema, 1000, ',', CsvNulls::AsReference, 0);
    } catch (...) {
        check(rv_ctx_set_option(ctx()->raw(), "csv_slow_cap", 0));
        throw;
    }
    check(rv_ctx_set_option(ctx()->raw(), "csv_slow_cap", 0));
    CHECK(ctx_counter("csv_slow_reparses") > reparses);
    std::remove(path.c_str());
}

GPU_TEST(edge_files_empty_header_only_no_newline) {
    const auto schema = schema_of({DataType::Int64, DataType::String});
    const char *files[] = {"", "a,b", "a,b\n", "\n", "\n1,x\n", "a,b\n1,x", "a,b\r\n1,x\r\n\r\n  \r\n2,y", "a,b\n\n\n", "a,b\n1,x\n\n",
                           "a,b\n 1 , null \n null,\n,\n", "a,b\n1"};
    int k = 0;
    for (const char *text : files) {
        const std::string path = write_file("edge" + std::to_string(k++) + ".csv", text);
        for (CsvNulls nulls : {CsvNulls::AsReference, CsvNulls::AsIntended})
            for (uint64_t chunk : {0ull, 16ull}) compare(path, schema, 2, ',', nulls, chunk);
        std::remove(path.c_str());
    }
}

GPU_TEST(ten_mib_field) {
    const auto schema = schema_of({DataType::Int64, DataType::String});
    std::string big(10u << 20, 'q');
    for (size_t i = 0; i < big.size(); i += 4099) big[i] = static_cast<char>(0xC3);
    const std::string path = write_file("big.csv", "a,b\n1,short\n2, " + big + " \n3,after\n");
    const Stats st = compare(path, schema, 2, ',', CsvNulls::AsReference, 1u << 20);  // the chunk has to grow past 10 MiB
    CHECK(st.rows == 3);
    compare(path, schema, std::nullopt, ',', CsvNulls::AsIntended, 0);
    std::remove(path.c_str());
}

GPU_TEST(host_layer_device_scan_and_errors) {
    Gen g(5);
    const auto schema = schema_of(kSchemas[0]);
    const std::string path = write_file("layer.csv", g.file(*schema, 2000, ',', 3, false, true));
    for (CsvNulls nulls : {CsvNulls::AsReference, CsvNulls::AsIntended}) compare(path, schema, 300, ',', nulls, 0, true);
    CHECK(compare(path, schema, 0, ',', CsvNulls::AsReference, 0, true).rows == 0);  // batch size 0: every call is the end
    std::remove(path.c_str());
    auto what = [](std::function<void()> f) -> std::pair<std::string, int> {
        try {
            f();
        } catch (const Error &e) {
            return {e.what(), static_cast<int>(e.status)};
        }
        return {"", 0};
    };
    const auto missing_h = what([&] { CsvFileStream s(ctx(), "/nonexistent/x.csv", schema); });
    const auto missing_d = what([&] { CsvFileStream s(ctx(), "/nonexistent/x.csv", schema, std::nullopt, std::nullopt, CsvNulls::AsReference, CsvScan::Device); });
    CHECK(missing_h == missing_d && missing_d.second == RV_ERR_INVALID_ARG && missing_d.first.rfind("Failed to open file: ", 0) == 0);
    const std::string p2 = write_file("nullcol.csv", "a\n1\n");
    const auto nullschema = schema_of({DataType::Null});
    const auto null_h = what([&] { CsvFileStream s(ctx(), p2, nullschema); });
    const auto null_d = what([&] { CsvFileStream s(ctx(), p2, nullschema, std::nullopt, std::nullopt, CsvNulls::AsReference, CsvScan::Device); });
    CHECK(null_h == null_d && null_d.second == RV_ERR_UNSUPPORTED);
    std::remove(p2.c_str());
}

GPU_TEST(csv_source_through_the_gpu_filter_project_plan_device_scan) {  // the host_tests query with CsvScan::Device
    using namespace physical_plan;
    const std::string path = write_file("plan.csv", "id,name,score,active\n1,Alice,85.5,true\n2,Bob,92.0,false\n3,Charlie,78.5,true\n4,,90.0,false\n5,Eve,null,true\n");
    std::vector<Field> f{{"id", DataType::Int64, true}, {"name", DataType::String, true}, {"score", DataType::Float64, true}, {"active", DataType::Boolean, true}};
    const auto schema = std::make_shared<Schema>(f);
    const LoweredPredicate pred{CompareTerm{"score", RV_GT, Literal(80.0)}, CompareTerm{"active", RV_EQ, Literal(true)}};
    for (CsvNulls nulls : {CsvNulls::AsIntended, CsvNulls::AsReference}) {
        auto host = StreamingPhysicalPlan::gpu_filter_project(StreamingPhysicalPlan::csv_file_source(ctx(), path, schema, 2, std::nullopt, nulls), pred, {"name", "id"});
        auto dev = StreamingPhysicalPlan::gpu_filter_project(
            StreamingPhysicalPlan::csv_file_source(ctx(), path, schema, 2, std::nullopt, nulls, CsvScan::Device), pred, {"name", "id"});
        RecordBatch a = host->collect(ctx()), b = dev->collect(ctx());
        CHECK(diff_batches(a, b).empty());
        if (nulls == CsvNulls::AsIntended) {
            auto name = std::dynamic_pointer_cast<const StringArray>(b.column(0));
            CHECK(b.num_rows() == 1 && *name->value(0) == "Alice");
        }
    }
    std::remove(path.c_str());
}
