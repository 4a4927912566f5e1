// Device CSV scan (csv.hip): the kernels that turn one chunk of file bytes -- whole lines only, the file's last line
// closed by a '\n' -- into typed columns.  Per chunk:
//   csv_newline_count  16-byte loads, newlines per 16-byte word            -> exclusive scan (device_exclusive_scan)
//   csv_newline_write  the position of every '\n', in order: line j ends at line_end[j]
//   csv_classify       per line: strip one trailing '\r', blank (empty after the trim) or not; the header is not a row
//                      -> exclusive scan of the flags = every row's index
//   csv_rows           row -> line
//   csv_parse          one lane per row: split on the delimiter, check the field count, parse every cell by its
//                      dtype, write values, and the bit columns (Boolean values, null bitmaps) a wave's 64 rows at a time
//                      by ballot; bad rows go to a compact error list, Float64 cells Eisel-Lemire cannot decide to the
//                      slow list
//   csv_f64_slow       (only when the slow list is not empty) the exact decimal path, with its digits in scratch
//   csv_str_copy       String columns: offsets from the scanned lengths, then the trimmed bytes
//   csv_segment_pop    set bits of every (batch, column) bitmap range: the null counts of the batches
// No kernel but csv_f64_slow uses scratch (make resources; DESIGN.md section "Device CSV scan").
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/rivulus_gpu.h"
#include "csv_parse.hpp"

namespace rvk {

constexpr int kCsvBlock = 256;

enum CsvErrKind : uint32_t { kCsvErrFields = 1, kCsvErrInt64 = 2, kCsvErrFloat64 = 3, kCsvErrBoolean = 4 };

struct CsvErr {  // one bad row
    uint32_t row, kind;
    uint32_t field;  // kCsvErrFields: the number of fields found; else the index of the first bad field
    uint32_t line;   // line index inside the chunk
    uint32_t b, e;   // kind != kCsvErrFields: the trimmed field's bytes
};

struct CsvSlow {  // a Float64 cell for csv_f64_slow
    uint32_t row, col, b, e;
};

struct CsvCol {
    uint32_t dtype;       // rv_dtype
    uint32_t ref_bitmap;  // Int64 / Float64 under RV_CSV_NULLS_AS_REFERENCE: the bitmap holds null = 1
    void *values;         // int64 / double per row; RV_BOOLEAN: value bits
    uint64_t *bitmap;     // per row: valid = 1 (ref_bitmap: null = 1)
    uint32_t *str_start;  // RV_STRING: first byte of the trimmed cell
    uint32_t *str_len;    // RV_STRING: its length (0 for a null)
};

struct CsvParseArgs {
    const uint8_t *bytes;
    const uint32_t *line_end;
    const uint32_t *row_line;
    uint32_t rows;
    uint32_t ncols;
    uint32_t delimiter;
    const CsvCol *cols;
    CsvErr *errs;
    unsigned int *n_errs;  // [0] errors, [1] slow cells
    CsvSlow *slow;
    uint32_t slow_cap;
};

__device__ __forceinline__ uint32_t count_byte16(uint4 v, uint32_t valid, uint8_t target) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) n += (k < static_cast<int>(valid)) & (((w[k >> 2] >> ((k & 3) * 8)) & 0xFF) == target);
    return n;
}

// counts[i] = newlines in bytes [16 i, 16 i + 16); `bytes` is readable up to a multiple of 16
static __global__ __launch_bounds__(kCsvBlock) void csv_newline_count(const uint8_t *bytes, uint64_t n, uint64_t nwords, uint32_t *counts) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCsvBlock + threadIdx.x;
    if (i >= nwords) return;
    const uint4 v = reinterpret_cast<const uint4 *>(bytes)[i];
    const uint64_t left = n - i * 16;
    counts[i] = count_byte16(v, left < 16 ? static_cast<uint32_t>(left) : 16u, '\n');
}

static __global__ __launch_bounds__(kCsvBlock) void csv_newline_write(const uint8_t *bytes, uint64_t n, uint64_t nwords, const uint64_t *excl,
                                                                      uint32_t *line_end) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCsvBlock + threadIdx.x;
    if (i >= nwords) return;
    const uint4 v = reinterpret_cast<const uint4 *>(bytes)[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint64_t o = excl[i];
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (i * 16 + k < n && ((w[k >> 2] >> ((k & 3) * 8)) & 0xFF) == '\n') line_end[o++] = static_cast<uint32_t>(i * 16 + k);
}

__device__ __forceinline__ void csv_line(const uint8_t *bytes, const uint32_t *line_end, uint32_t j, uint32_t *s, uint32_t *e) {
    *s = j == 0 ? 0u : line_end[j - 1] + 1;
    *e = line_end[j];
    if (*e > *s && bytes[*e - 1] == '\r') --*e;
}

// flags[j] = 1: line j is a row (not blank, not the header)
static __global__ __launch_bounds__(kCsvBlock) void csv_classify(const uint8_t *bytes, const uint32_t *line_end, uint32_t nlines, uint32_t skip_first,
                                                                 uint32_t *flags) {
    const uint32_t j = blockIdx.x * kCsvBlock + threadIdx.x;
    if (j >= nlines) return;
    uint32_t s, e;
    csv_line(bytes, line_end, j, &s, &e);
    uint32_t k = s;
    while (k < e && rvcsv::is_space(bytes[k])) ++k;
    flags[j] = (k < e && !(j == 0 && skip_first)) ? 1u : 0u;
}

static __global__ __launch_bounds__(kCsvBlock) void csv_rows(const uint32_t *flags, const uint64_t *excl, uint32_t nlines, uint32_t *row_line) {
    const uint32_t j = blockIdx.x * kCsvBlock + threadIdx.x;
    if (j >= nlines || !flags[j]) return;
    row_line[excl[j]] = j;
}

__device__ __forceinline__ void csv_store_bits(uint64_t *dst, uint32_t row, bool bit) {
    const uint64_t word = __ballot(bit);
    if ((threadIdx.x & 63) == 0) dst[row >> 6] = word;
}

// One lane per row; the 64 rows of a wave are consecutive and start at a multiple of 64, so a ballot is one bitmap word.
static __global__ __launch_bounds__(kCsvBlock) void csv_parse(CsvParseArgs a) {
    const uint32_t r = blockIdx.x * kCsvBlock + threadIdx.x;
    const uint32_t wave_row = r & ~63u;
    if (wave_row >= a.rows) return;  // whole waves only: the ballots below need every lane of a live wave
    const bool active = r < a.rows;
    uint32_t s = 0, e = 0, line = 0;
    if (active) {
        line = a.row_line[r];
        csv_line(a.bytes, a.line_end, line, &s, &e);
    }
    const uint8_t delim = static_cast<uint8_t>(a.delimiter);
    uint32_t pos = s;
    bool more = active;  // field c exists
    uint32_t fields = 0;  // fields of the line the loop saw
    uint32_t bad_field = ~0u, bad_b = 0, bad_e = 0, bad_kind = 0;
    for (uint32_t c = 0; c < a.ncols; ++c) {
        const CsvCol col = a.cols[c];
        uint32_t fb = pos, fe = pos;
        if (more) {
            while (fe < e && a.bytes[fe] != delim) ++fe;
        }
        const bool have = more;
        fields += have;
        more = have && fe < e;
        pos = fe + 1;
        rvcsv::trim(a.bytes, &fb, &fe);
        const uint8_t *cell = a.bytes + fb;
        const uint32_t len = fe - fb;
        const bool null = !have || rvcsv::is_null_cell(cell, len);
        bool bit = false;  // RV_BOOLEAN value
        bool ok = true;
        switch (col.dtype) {
            case RV_INT64: {
                int64_t v = 0;
                if (!null) ok = rvcsv::parse_i64(cell, len, &v);
                if (active) static_cast<int64_t *>(col.values)[r] = ok ? v : 0;
                if (!ok && bad_field == ~0u) bad_kind = kCsvErrInt64;
                break;
            }
            case RV_FLOAT64: {
                double v = 0.0;
                if (!null) {
                    const rvcsv::F64Status st = rvcsv::parse_f64(cell, len, &v);
                    ok = st != rvcsv::kF64Bad;
                    if (st == rvcsv::kF64Slow) {
                        const unsigned int k = atomicAdd(&a.n_errs[1], 1u);
                        if (k < a.slow_cap) a.slow[k] = CsvSlow{r, c, fb, fe};
                    }
                    if (st != rvcsv::kF64Ok) v = 0.0;
                }
                if (active) static_cast<double *>(col.values)[r] = v;
                if (!ok && bad_field == ~0u) bad_kind = kCsvErrFloat64;
                break;
            }
            case RV_BOOLEAN: {
                if (!null) ok = rvcsv::parse_bool(cell, len, &bit);
                if (!ok && bad_field == ~0u) bad_kind = kCsvErrBoolean;
                csv_store_bits(static_cast<uint64_t *>(col.values), r, active && ok && bit);
                break;
            }
            default: {  // RV_STRING
                if (active) {
                    col.str_start[r] = fb;
                    col.str_len[r] = null ? 0u : len;
                }
                break;
            }
        }
        if (!ok && bad_field == ~0u) {
            bad_field = c;
            bad_b = fb;
            bad_e = fe;
        }
        csv_store_bits(col.bitmap, r, active && (col.ref_bitmap ? null : !null));
    }
    if (!active) return;
    // the field count comes first (the host stream checks it before any cell)
    uint32_t found = fields;
    if (more) {  // fields beyond the schema's: one more per delimiter left in the line
        found = a.ncols + 1;
        for (uint32_t k = pos; k < e; ++k) found += a.bytes[k] == delim;
    }
    const bool count_bad = found != a.ncols;
    if (count_bad || bad_field != ~0u) {
        const unsigned int k = atomicAdd(&a.n_errs[0], 1u);
        CsvErr err;
        err.row = r;
        err.line = line;
        err.kind = count_bad ? static_cast<uint32_t>(kCsvErrFields) : bad_kind;
        err.field = count_bad ? found : bad_field;
        err.b = bad_b;
        err.e = bad_e;
        a.errs[k] = err;  // the list has room for every row
    }
}

// the cells parse_f64 left undecided; one lane per cell, the ~800 digits of rvcsv::Decimal in scratch
static __global__ __launch_bounds__(64) void csv_f64_slow(const uint8_t *bytes, const CsvSlow *slow, uint32_t n, const CsvCol *cols) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const CsvSlow c = slow[i];
    rvcsv::Decimal dec;
    static_cast<double *>(cols[c.col].values)[c.row] = rvcsv::parse_f64_slow(bytes + c.b, c.e - c.b, &dec);
}

// String column: offsets (int32, from the exclusive scan of the lengths) and the bytes of every cell.  A cell longer than
// kCsvLongCell is copied by its whole wave, 64 bytes a step, not by its own lane.
constexpr uint32_t kCsvLongCell = 256;
static __global__ __launch_bounds__(kCsvBlock) void csv_str_copy(const uint8_t *bytes, const uint32_t *start, const uint32_t *len, const uint64_t *excl,
                                                                 uint32_t rows, int32_t *offsets, uint8_t *data) {
    const uint32_t r = blockIdx.x * kCsvBlock + threadIdx.x;
    if ((r & ~63u) > rows) return;  // whole waves only: long cells are copied by every lane of the wave
    if (r <= rows) offsets[r] = static_cast<int32_t>(excl[r]);
    const uint32_t n = r < rows ? len[r] : 0u;
    const uint8_t *src = r < rows ? bytes + start[r] : bytes;
    uint8_t *dst = r < rows ? data + excl[r] : data;
    if (n <= kCsvLongCell) {
        for (uint32_t k = 0; k < n; ++k) dst[k] = src[k];
    }
    uint64_t longs = __ballot(n > kCsvLongCell);
    const uint32_t lane = threadIdx.x & 63;
    while (longs) {
        const int l = __ffsll(static_cast<long long>(longs)) - 1;
        longs &= longs - 1;
        const uint32_t ln = __shfl(n, l, 64);
        const uint32_t r_l = (r & ~63u) + static_cast<uint32_t>(l);
        const uint8_t *s = bytes + start[r_l];
        uint8_t *d = data + excl[r_l];
        for (uint32_t k = lane; k < ln; k += 64) d[k] = s[k];
    }
}

// counts[s * ncols + c] = set bits of cols[c].bitmap over rows [seg[2s], seg[2s+1]); one wave per (segment, column)
static __global__ __launch_bounds__(64) void csv_segment_pop(const CsvCol *cols, uint32_t ncols, const uint32_t *seg, uint32_t nseg, uint32_t *counts) {
    const uint32_t s = blockIdx.x, c = blockIdx.y;
    if (s >= nseg || c >= ncols) return;
    const uint64_t *bm = cols[c].bitmap;
    const uint32_t a = seg[2 * s], b = seg[2 * s + 1];
    uint32_t n = 0;
    if (b > a) {
        const uint32_t w0 = a >> 6, w1 = (b - 1) >> 6;
        for (uint32_t w = w0 + threadIdx.x; w <= w1; w += 64) {
            uint64_t x = bm[w];
            if (w == w0) x &= ~uint64_t(0) << (a & 63);
            if (w == w1 && (b & 63)) x &= ~(~uint64_t(0) << (b & 63));
            n += __popcll(x);
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d, 64);
    if (threadIdx.x == 0) counts[s * ncols + c] = n;
}

}  // namespace rvk
