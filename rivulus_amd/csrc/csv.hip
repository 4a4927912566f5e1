// CSV scan on the device (reference CsvFileStream, file_stream.rs:10-368): the file is read in pinned chunks, each chunk
// is uploaded and parsed by the kernels of csv_kernels.hpp, and rv_csv_next hands out the batches CsvFileStream::next_batch
// would return -- zero-copy slices of the parsed chunk, no launch per batch.
//
// A chunk holds whole lines only.  Rows of a chunk are cut into batches of batch_rows from its first row on; a bad row ends
// the batch it falls in (the error is returned and the next batch starts after it, as the host stream does).  The rows
// left over at the end of a chunk that do not fill a batch are not returned from it: their bytes are carried over to the
// front of the next chunk (with the partial line after the chunk's last '\n') and parsed again there.  Only the chunk
// that ends the file returns a short batch.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstring>
#include <future>

#include "csv_kernels.hpp"
#include "launch.hpp"

using namespace rvh;
using namespace rvl;

namespace {

constexpr uint64_t kDefaultChunk = 64ull << 20;
constexpr size_t kPad = 64;  // bytes past a chunk: the appended '\n' and the 16-byte loads of the last word

uint64_t adaptive_batch_rows(const std::vector<rv_dtype> &dtypes) {  // file_stream.rs:345-368
    uint64_t row = 0;
    for (rv_dtype t : dtypes) row += (t == RV_INT64 || t == RV_FLOAT64) ? 8 : (t == RV_BOOLEAN ? 1 : (t == RV_STRING ? 32 : 0));
    if (row == 0) return 10000;
    return std::min<uint64_t>(100000, std::max<uint64_t>(1000, (8ull << 20) / row));
}

struct PinnedBuf {
    uint8_t *ptr = nullptr;
    size_t cap = 0;  // bytes
    size_t head = 0; // room kept in front of the raw bytes for the carry of the previous chunk
    void ensure(size_t head_bytes, size_t raw_bytes) {
        const size_t need = head_bytes + raw_bytes + kPad;
        if (need <= cap) {
            head = head_bytes;
            return;
        }
        release();
        const size_t want = need + need / 4;
        RV_HIP(hipHostMalloc(reinterpret_cast<void **>(&ptr), want, hipHostMallocDefault));
        cap = want;
        head = head_bytes;
    }
    void release() {
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

struct ReadResult {
    size_t got = 0;
    int err = 0;
};

}  // namespace

struct rv_csv_reader {
    rv_ctx *ctx = nullptr;
    int fd = -1;
    std::vector<rv_dtype> dtypes;
    uint8_t delimiter = ',';
    uint64_t batch_rows = 0;
    bool as_reference = false;
    uint64_t chunk_bytes = kDefaultChunk;

    // file -> pinned buffers: buf[cur] holds the chunk being handed out, the read of the next raw segment goes to buf[1 - cur]
    PinnedBuf buf[2];
    int cur = 0;
    uint64_t file_off = 0;  // next byte of the file to read
    uint64_t file_size = 0; // at open (a read that comes short ends the file whatever this says)
    bool read_pending = false;
    size_t pending_want = 0;
    std::future<ReadResult> pending;

    // the chunk
    bool have_chunk = false, final_chunk = false, done = false;
    const uint8_t *chunk = nullptr;  // host bytes of the chunk (inside buf[cur])
    uint64_t chunk_len = 0;          // bytes parsed (whole lines)
    uint64_t chunk_total = 0;        // bytes in the buffer (the partial last line included)
    uint64_t base_line = 0;          // file lines before the chunk's first line
    uint32_t nlines = 0, rows = 0;
    std::vector<rvk::CsvErr> errs;  // by row
    size_t next_err = 0;
    uint64_t p = 0;  // next row to hand out
    struct Seg {
        uint32_t a, b;
    };
    std::vector<Seg> segs;          // the batches of the chunk, in order
    std::vector<uint32_t> seg_pop;  // set bitmap bits per (batch, column)
    size_t next_seg = 0;
    std::vector<std::shared_ptr<rv_dcolumn>> cols;  // the chunk's parsed columns (full length)

    // carry into the next chunk
    const uint8_t *carry = nullptr;
    uint64_t carry_len = 0;
    uint64_t carry_lines = 0;  // lines of the current chunk before the carried bytes

    // device scratch reused across chunks
    DevBufRef d_bytes, d_counts, d_line_end, d_flags, d_row_line, d_errs, d_nerr, d_slow, d_cols, d_seg, d_pop;

    uint64_t lines_total = 0, bytes_read = 0;

    ~rv_csv_reader() {
        if (read_pending) pending.wait();
        if (fd >= 0) close(fd);
        buf[0].release();
        buf[1].release();
    }

    void start_read(int which, size_t head, size_t want) {
        // no more than the file holds, + 1: the read that comes short is the end
        if (file_off >= file_size) want = std::min<size_t>(want, 4096);
        else if (file_size - file_off < want) want = file_size - file_off + 1;
        buf[which].ensure(head, want);
        uint8_t *dst = buf[which].ptr + buf[which].head;
        const int f = fd;
        const uint64_t off = file_off;
        file_off += want;
        pending_want = want;
        read_pending = true;
        pending = std::async(std::launch::async, [f, dst, off, want] {
            ReadResult r;
            while (r.got < want) {
                const ssize_t k = pread(f, dst + r.got, want - r.got, static_cast<off_t>(off + r.got));
                if (k < 0) {
                    if (errno == EINTR) continue;
                    r.err = errno;
                    break;
                }
                if (k == 0) break;
                r.got += static_cast<size_t>(k);
            }
            return r;
        });
    }

    DevBufRef &grow(DevBufRef &b, size_t bytes) {
        if (!b || b->bytes < bytes) b = pool_alloc(ctx, std::max<size_t>(bytes, 256));
        return b;
    }

    // the next chunk: the carry of this one + the raw segment read behind it; parsed on the device
    void load_chunk() {
        const int nb = 1 - cur;
        if (!read_pending) start_read(nb, carry_len, std::max<uint64_t>(chunk_bytes, 2 * carry_len));
        const ReadResult rr = pending.get();
        read_pending = false;
        if (rr.err) throw Error(RV_ERR_INVALID_ARG, std::string("Failed to read file: ") + std::strerror(rr.err));
        bytes_read += rr.got;
        const bool eof = rr.got < pending_want;
        PinnedBuf &B = buf[nb];
        uint8_t *raw = B.ptr + B.head;
        uint8_t *start;
        if (carry_len <= B.head) {
            start = raw - carry_len;
            if (carry_len) std::memcpy(start, carry, carry_len);
        } else {  // a read that was started before the carry was known: make room
            PinnedBuf nbuf;
            nbuf.ensure(carry_len, rr.got);
            start = nbuf.ptr + nbuf.head - carry_len;
            std::memcpy(start, carry, carry_len);
            std::memcpy(nbuf.ptr + nbuf.head, raw, rr.got);
            B.release();
            B = nbuf;
        }
        base_line += carry_lines;
        carry_lines = 0;
        cur = nb;
        uint64_t total = carry_len + rr.got;
        carry = nullptr;
        const uint64_t carried = carry_len;
        carry_len = 0;
        uint64_t cut;  // bytes of whole lines
        if (eof) {
            if (total > 0 && start[total - 1] != '\n') start[total++] = '\n';  // a last line without '\n' still counts
            cut = total;
        } else {
            const void *nl = total ? memrchr(start, '\n', total) : nullptr;
            cut = nl ? static_cast<uint64_t>(static_cast<const uint8_t *>(nl) - start) + 1 : 0;
        }
        chunk = start;
        chunk_len = cut;
        chunk_total = total;
        final_chunk = eof;
        have_chunk = true;
        // the read of the next raw segment runs while this chunk is parsed and handed out
        // (room in front for the carry it will get: a batch's bytes, usually -- a larger one is copied into place)
        if (!eof) start_read(1 - cur, std::max<uint64_t>(chunk_bytes / 4, 2 * carried), std::max<uint64_t>(chunk_bytes, 2 * carried));
        parse();
    }

    void parse() {
        rv_ctx *c = ctx;
        hipStream_t st = c->stream;
        const uint32_t ncols = static_cast<uint32_t>(dtypes.size());
        nlines = 0;
        rows = 0;
        errs.clear();
        next_err = 0;
        p = 0;
        segs.clear();
        seg_pop.clear();
        next_seg = 0;
        cols.clear();
        // batches do not cross chunks: a batch's rows (or one line) must fit in a chunk, and a chunk in 2^31 bytes
        require(chunk_len < (1ull << 31), RV_ERR_UNSUPPORTED, "rv_csv: one batch of rows (or one line) spans 2 GiB or more of the file");
        const uint64_t n = chunk_len;
        if (n > 0) {
            const uint64_t nwords = (n + 15) / 16;
            grow(d_bytes, nwords * 16 + kPad);
            RV_HIP(hipMemcpyAsync(d_bytes->ptr, chunk, n, hipMemcpyHostToDevice, st));
            const uint8_t *bytes = static_cast<const uint8_t *>(d_bytes->ptr);
            grow(d_counts, nwords * 4);
            hipLaunchKernelGGL(rvk::csv_newline_count, dim3(static_cast<uint32_t>((nwords + rvk::kCsvBlock - 1) / rvk::kCsvBlock)), dim3(rvk::kCsvBlock), 0, st,
                               bytes, n, nwords, static_cast<uint32_t *>(d_counts->ptr));
            DevBufRef excl;
            nlines = static_cast<uint32_t>(device_exclusive_scan(c, d_counts->ptr, nwords, excl));
            grow(d_line_end, static_cast<size_t>(nlines) * 4);
            hipLaunchKernelGGL(rvk::csv_newline_write, dim3(static_cast<uint32_t>((nwords + rvk::kCsvBlock - 1) / rvk::kCsvBlock)), dim3(rvk::kCsvBlock), 0, st,
                               bytes, n, nwords, static_cast<const uint64_t *>(excl->ptr), static_cast<uint32_t *>(d_line_end->ptr));
            const uint32_t lgrid = (nlines + rvk::kCsvBlock - 1) / rvk::kCsvBlock;
            grow(d_flags, static_cast<size_t>(nlines) * 4);
            if (nlines)
                hipLaunchKernelGGL(rvk::csv_classify, dim3(lgrid), dim3(rvk::kCsvBlock), 0, st, bytes, static_cast<const uint32_t *>(d_line_end->ptr), nlines,
                               base_line == 0 ? 1u : 0u, static_cast<uint32_t *>(d_flags->ptr));
            DevBufRef rexcl;
            rows = static_cast<uint32_t>(device_exclusive_scan(c, d_flags->ptr, nlines, rexcl));
            grow(d_row_line, static_cast<size_t>(rows) * 4);
            if (rows)
                hipLaunchKernelGGL(rvk::csv_rows, dim3(lgrid), dim3(rvk::kCsvBlock), 0, st, static_cast<const uint32_t *>(d_flags->ptr),
                                   static_cast<const uint64_t *>(rexcl->ptr), nlines, static_cast<uint32_t *>(d_row_line->ptr));
            RV_HIP(hipGetLastError());
        }
        lines_total = base_line + nlines;

        // the columns of the chunk
        const uint64_t nwords_rows = (rows + 63) / 64;
        std::vector<rvk::CsvCol> dc(ncols);
        std::vector<DevBufRef> starts(ncols), lens(ncols);
        for (uint32_t k = 0; k < ncols; ++k) {
            auto col = std::make_shared<rv_dcolumn>();
            col->dtype = dtypes[k];
            col->length = rows;
            col->null_count = -1;
            const size_t bm_bytes = std::max<size_t>(nwords_rows * 8, 8) + 8;
            col->validity = pool_alloc(c, bm_bytes);
            dc[k].dtype = dtypes[k];
            dc[k].ref_bitmap = as_reference && (dtypes[k] == RV_INT64 || dtypes[k] == RV_FLOAT64);
            dc[k].bitmap = static_cast<uint64_t *>(col->validity->ptr);
            if (dtypes[k] == RV_BOOLEAN) {
                col->values = pool_alloc(c, bm_bytes);
            } else if (dtypes[k] == RV_STRING) {
                starts[k] = pool_alloc(c, static_cast<size_t>(rows) * 4 + 8);
                lens[k] = pool_alloc(c, static_cast<size_t>(rows) * 4 + 8);
                dc[k].str_start = static_cast<uint32_t *>(starts[k]->ptr);
                dc[k].str_len = static_cast<uint32_t *>(lens[k]->ptr);
            } else {
                col->values = pool_alloc(c, std::max<size_t>(static_cast<size_t>(rows) * 8, 8));
            }
            if (col->values) dc[k].values = col->values->ptr;
            cols.push_back(col);
        }
        if (rows > 0) {
            grow(d_cols, std::max<size_t>(ncols, 1) * sizeof(rvk::CsvCol));
            if (ncols) RV_HIP(hipMemcpyAsync(d_cols->ptr, dc.data(), ncols * sizeof(rvk::CsvCol), hipMemcpyHostToDevice, st));
            grow(d_errs, static_cast<size_t>(rows) * sizeof(rvk::CsvErr));
            grow(d_nerr, 16);
            RV_HIP(hipMemsetAsync(d_nerr->ptr, 0, 8, st));
            uint32_t nfloat = 0;
            for (rv_dtype t : dtypes) nfloat += t == RV_FLOAT64;
            uint64_t slow_cap = std::min<uint64_t>(static_cast<uint64_t>(rows) * nfloat, 1u << 20);
            if (c->opt_csv_slow_cap > 0) slow_cap = std::min<uint64_t>(slow_cap, static_cast<uint64_t>(c->opt_csv_slow_cap));
            grow(d_slow, std::max<uint64_t>(slow_cap, 1) * sizeof(rvk::CsvSlow));
            rvk::CsvParseArgs a{};
            a.bytes = static_cast<const uint8_t *>(d_bytes->ptr);
            a.line_end = static_cast<const uint32_t *>(d_line_end->ptr);
            a.row_line = static_cast<const uint32_t *>(d_row_line->ptr);
            a.rows = rows;
            a.ncols = ncols;
            a.delimiter = delimiter;
            a.cols = static_cast<const rvk::CsvCol *>(d_cols->ptr);
            a.errs = static_cast<rvk::CsvErr *>(d_errs->ptr);
            a.n_errs = static_cast<unsigned int *>(d_nerr->ptr);
            a.slow = static_cast<rvk::CsvSlow *>(d_slow->ptr);
            a.slow_cap = static_cast<uint32_t>(slow_cap);
            hipLaunchKernelGGL(rvk::csv_parse, dim3((rows + rvk::kCsvBlock - 1) / rvk::kCsvBlock), dim3(rvk::kCsvBlock), 0, st, a);
            RV_HIP(hipGetLastError());
            unsigned int counts[2] = {0, 0};
            RV_HIP(hipMemcpyAsync(counts, d_nerr->ptr, 8, hipMemcpyDeviceToHost, st));
            RV_HIP(hipStreamSynchronize(st));
            if (counts[1] > 0) {
                if (counts[1] > slow_cap) {  // more undecided cells than the list holds: a list of that size, parse again
                    ++c->csv_slow_reparses;
                    grow(d_slow, static_cast<size_t>(counts[1]) * sizeof(rvk::CsvSlow));
                    a.slow = static_cast<rvk::CsvSlow *>(d_slow->ptr);
                    a.slow_cap = counts[1];
                    RV_HIP(hipMemsetAsync(d_nerr->ptr, 0, 8, st));
                    hipLaunchKernelGGL(rvk::csv_parse, dim3((rows + rvk::kCsvBlock - 1) / rvk::kCsvBlock), dim3(rvk::kCsvBlock), 0, st, a);
                    RV_HIP(hipMemcpyAsync(counts, d_nerr->ptr, 8, hipMemcpyDeviceToHost, st));
                    RV_HIP(hipStreamSynchronize(st));
                }
                hipLaunchKernelGGL(rvk::csv_f64_slow, dim3((counts[1] + 63) / 64), dim3(64), 0, st, static_cast<const uint8_t *>(d_bytes->ptr),
                                   static_cast<const rvk::CsvSlow *>(d_slow->ptr), counts[1], static_cast<const rvk::CsvCol *>(d_cols->ptr));
                RV_HIP(hipGetLastError());
                c->csv_slow_cells += counts[1];
            }
            if (counts[0] > 0) {
                errs.resize(counts[0]);
                RV_HIP(hipMemcpyAsync(errs.data(), d_errs->ptr, counts[0] * sizeof(rvk::CsvErr), hipMemcpyDeviceToHost, st));
                RV_HIP(hipStreamSynchronize(st));
                std::sort(errs.begin(), errs.end(), [](const rvk::CsvErr &x, const rvk::CsvErr &y) { return x.row < y.row; });
            }
            // String columns: offsets and bytes
            for (uint32_t k = 0; k < ncols; ++k) {
                if (dtypes[k] != RV_STRING) continue;
                DevBufRef sexcl;
                const uint64_t total = device_exclusive_scan(c, lens[k]->ptr, rows, sexcl);
                require(total < (1ull << 31), RV_ERR_UNSUPPORTED, "rv_csv: more than 2 GiB of String bytes in one chunk");
                rv_dcolumn &col = *cols[k];
                col.offsets = pool_alloc(c, (static_cast<size_t>(rows) + 1) * 4);
                col.values = pool_alloc(c, std::max<uint64_t>(total, 8));
                col.data_bytes = total;
                hipLaunchKernelGGL(rvk::csv_str_copy, dim3((rows + 1 + rvk::kCsvBlock - 1) / rvk::kCsvBlock), dim3(rvk::kCsvBlock), 0, st,
                                   static_cast<const uint8_t *>(d_bytes->ptr), dc[k].str_start, dc[k].str_len, static_cast<const uint64_t *>(sexcl->ptr), rows,
                                   static_cast<int32_t *>(col.offsets->ptr), static_cast<uint8_t *>(col.values->ptr));
                RV_HIP(hipGetLastError());
            }
        }
        for (uint32_t k = 0; k < ncols; ++k)
            if (dtypes[k] == RV_STRING && !cols[k]->offsets) {  // no rows: offsets {0}
                cols[k]->offsets = pool_alloc(c, 8);
                RV_HIP(hipMemsetAsync(cols[k]->offsets->ptr, 0, 8, st));
                cols[k]->values = pool_alloc(c, 8);
            }
        plan_batches();
    }

    // the batches this chunk hands out (the host stream's cut: batch_rows rows, a bad row ends a batch) and their null counts
    void plan_batches() {
        uint64_t q = 0;
        size_t ei = 0;
        for (;;) {
            while (ei < errs.size() && errs[ei].row < q) ++ei;
            if (ei < errs.size() && errs[ei].row - q < batch_rows) {
                q = errs[ei].row + 1;
                continue;
            }
            if (rows - q >= batch_rows) {
                segs.push_back({static_cast<uint32_t>(q), static_cast<uint32_t>(q + batch_rows)});
                q += batch_rows;
                continue;
            }
            if (final_chunk && q < rows) segs.push_back({static_cast<uint32_t>(q), rows});
            break;
        }
        const uint32_t ncols = static_cast<uint32_t>(dtypes.size());
        if (segs.empty() || ncols == 0) return;
        hipStream_t st = ctx->stream;
        grow(d_seg, segs.size() * 8);
        grow(d_pop, segs.size() * ncols * 4);
        RV_HIP(hipMemcpyAsync(d_seg->ptr, segs.data(), segs.size() * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(rvk::csv_segment_pop, dim3(static_cast<uint32_t>(segs.size()), ncols), dim3(64), 0, st, static_cast<const rvk::CsvCol *>(d_cols->ptr),
                           ncols, static_cast<const uint32_t *>(d_seg->ptr), static_cast<uint32_t>(segs.size()), static_cast<uint32_t *>(d_pop->ptr));
        RV_HIP(hipGetLastError());
        seg_pop.resize(segs.size() * ncols);
        RV_HIP(hipMemcpyAsync(seg_pop.data(), d_pop->ptr, seg_pop.size() * 4, hipMemcpyDeviceToHost, st));
        RV_HIP(hipStreamSynchronize(st));
    }

    std::string error_text(const rvk::CsvErr &e) const {
        const uint64_t line = base_line + e.line + 1;
        if (e.kind == rvk::kCsvErrFields)
            return "Line " + std::to_string(line) + ": Expected " + std::to_string(dtypes.size()) + " fields, found " + std::to_string(e.field);
        const char *type = e.kind == rvk::kCsvErrInt64 ? "Int64" : (e.kind == rvk::kCsvErrFloat64 ? "Float64" : "Boolean");
        return "Line " + std::to_string(line) + ", field " + std::to_string(e.field) + ": Cannot parse '" +
               std::string(reinterpret_cast<const char *>(chunk) + e.b, e.e - e.b) + "' as " + type;
    }

    // leave the rows from `p` on (and the partial last line) to the next chunk
    void carry_from_p() {
        uint32_t line = nlines;
        if (p < rows) {
            RV_HIP(hipMemcpy(&line, static_cast<const uint32_t *>(d_row_line->ptr) + p, 4, hipMemcpyDeviceToHost));
        }
        uint64_t byte = chunk_len;
        if (line < nlines && line > 0) {
            uint32_t prev_end = 0;
            RV_HIP(hipMemcpy(&prev_end, static_cast<const uint32_t *>(d_line_end->ptr) + line - 1, 4, hipMemcpyDeviceToHost));
            byte = prev_end + 1;
        } else if (line == 0) {
            byte = 0;
        }
        carry = chunk + byte;
        carry_len = chunk_total - byte;
        carry_lines = line;
        have_chunk = false;
        cols.clear();
    }

    // one call of CsvFileStream::next_batch
    uint64_t next(rv_dcolumn **out) {
        for (;;) {
            if (done) return 0;
            if (!have_chunk) {
                load_chunk();
                continue;
            }
            while (next_err < errs.size() && errs[next_err].row < p) ++next_err;
            if (next_err < errs.size() && errs[next_err].row - p < batch_rows) {
                const rvk::CsvErr e = errs[next_err++];
                p = e.row + 1;
                while (next_seg < segs.size() && segs[next_seg].a < p) ++next_seg;
                throw Error(RV_ERR_PARSE, error_text(e));
            }
            if (next_seg < segs.size() && segs[next_seg].a == p) {
                const Seg s = segs[next_seg];
                const uint32_t ncols = static_cast<uint32_t>(dtypes.size());
                const uint64_t len = s.b - s.a;
                std::vector<std::unique_ptr<rv_dcolumn>> made;
                for (uint32_t k = 0; k < ncols; ++k) {
                    auto o = std::make_unique<rv_dcolumn>(*cols[k]);
                    o->offset = s.a;
                    o->length = len;
                    const uint64_t set = seg_pop[next_seg * ncols + k];
                    const bool ref = as_reference && (dtypes[k] == RV_INT64 || dtypes[k] == RV_FLOAT64);
                    const uint64_t nulls = ref ? set : len - set;
                    if (nulls == 0) {
                        o->validity.reset();
                        o->null_count = 0;
                    } else {
                        o->null_count = static_cast<int64_t>(ref ? len - set : nulls);  // zero bits of the bitmap handed out
                    }
                    made.push_back(std::move(o));
                }
                for (uint32_t k = 0; k < ncols; ++k) out[k] = made[k].release();
                ++next_seg;
                p = s.b;
                return len;
            }
            if (final_chunk) {  // every row handed out
                done = true;
                have_chunk = false;
                cols.clear();
                return 0;
            }
            carry_from_p();
        }
    }
};

extern "C" {

rv_status rv_csv_open(rv_ctx *ctx, const char *path, const rv_dtype *dtypes, uint32_t ncols, uint32_t delimiter, uint64_t batch_rows, uint32_t flags,
                      uint64_t chunk_bytes, rv_csv_reader **out) {
    return guarded([&] {
        require(ctx && path && out && (dtypes || ncols == 0), RV_ERR_INVALID_ARG, "rv_csv_open: NULL argument");
        require((flags & ~RV_CSV_NULLS_AS_REFERENCE) == 0, RV_ERR_INVALID_ARG, "rv_csv_open: unknown flags");
        require(delimiter < 256, RV_ERR_INVALID_ARG, "rv_csv_open: the delimiter is one byte");
        for (uint32_t k = 0; k < ncols; ++k) {
            require(dtypes[k] >= RV_NULL && dtypes[k] <= RV_STRING, RV_ERR_INVALID_ARG, "rv_csv_open: unknown dtype");
        }
        const int fd = open(path, O_RDONLY | O_CLOEXEC);
        if (fd < 0) throw Error(RV_ERR_INVALID_ARG, std::string("Failed to open file: ") + std::strerror(errno));
        auto r = std::make_unique<rv_csv_reader>();
        r->fd = fd;
        struct stat sb;
        if (fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode)) r->file_size = static_cast<uint64_t>(sb.st_size);
        else r->file_size = ~0ull;
        for (uint32_t k = 0; k < ncols; ++k)
            if (dtypes[k] == RV_NULL) throw Error(RV_ERR_UNSUPPORTED, "Null columns are outside the device path");
        set_device(ctx);
        r->ctx = ctx;
        r->dtypes.assign(dtypes, dtypes + ncols);
        r->delimiter = static_cast<uint8_t>(delimiter);
        r->as_reference = (flags & RV_CSV_NULLS_AS_REFERENCE) != 0;
        r->batch_rows = batch_rows ? batch_rows : adaptive_batch_rows(r->dtypes);
        require(r->batch_rows < (1ull << 31), RV_ERR_INVALID_ARG, "rv_csv_open: batch_rows of 2^31 or more");
        r->chunk_bytes = chunk_bytes ? std::max<uint64_t>(chunk_bytes, 16) : kDefaultChunk;
        require(r->chunk_bytes < (1ull << 30), RV_ERR_INVALID_ARG, "rv_csv_open: chunk_bytes of 1 GiB or more");
        r->start_read(1, 0, r->chunk_bytes);  // the first chunk is read while the caller gets on
        *out = r.release();
    });
}

rv_status rv_csv_next(rv_csv_reader *reader, rv_dcolumn **out, uint64_t *out_rows) {
    return guarded([&] {
        require(reader && out_rows && (out || reader->dtypes.empty()), RV_ERR_INVALID_ARG, "rv_csv_next: NULL argument");
        *out_rows = 0;
        set_device(reader->ctx);
        *out_rows = reader->next(out);
    });
}

rv_status rv_csv_reader_info(const rv_csv_reader *reader, uint64_t *batch_rows, uint64_t *lines, uint64_t *bytes_read) {
    return guarded([&] {
        require(reader, RV_ERR_INVALID_ARG, "rv_csv_reader_info: NULL argument");
        if (batch_rows) *batch_rows = reader->batch_rows;
        if (lines) *lines = reader->lines_total;
        if (bytes_read) *bytes_read = reader->bytes_read;
    });
}

rv_status rv_csv_close(rv_csv_reader *reader) {
    return guarded([&] { delete reader; });
}

}  // extern "C"
