// The host-side steps the device units behind the pipeline breakers share (sort / topk / group_agg / window / window_frame / join .hip; the
// timer also string_dict / aggregate .hip): the timer round a unit's own passes, the read-back of striped null counts, the Int64 index
// column, the check of a key list's column indices and the body of an entry point.  The chain of sorts is sort.hip's (launch.hpp).
#pragma once

#include "launch.hpp"

namespace rvl {

// Events round a unit's own passes (option profile_kernels): start() marks the stream, the passes count themselves in `launches`, and the
// time between the marks goes to the context's kernel statistics with them.  The end comes in two forms, so that no unit waits more than
// it has to: stop() marks the stream and add() reads the marks after a wait the caller makes anyway; stop_and_wait() waits on the mark.
struct PassTimer {
    rv_ctx *ctx;
    uint64_t launches = 0;
    bool open = false;
    explicit PassTimer(rv_ctx *c) : ctx(c) {}
    void start() {  // a timer that is open stays where it was started
        if (ctx->opt_profile && !open) RV_HIP(hipEventRecord(ctx->evk0, ctx->stream));
        open = true;
    }
    void stop() {
        if (ctx->opt_profile && open) RV_HIP(hipEventRecord(ctx->evk1, ctx->stream));
    }
    void add() {  // after a wait for the stream
        if (!open) return;
        open = false;
        if (!ctx->opt_profile) return;
        float ms = 0.f;
        RV_HIP(hipEventElapsedTime(&ms, ctx->evk0, ctx->evk1));
        ctx->kernel_ms += ms;
        ctx->kernel_launches += launches;
        launches = 0;
    }
    void stop_and_wait() {
        stop();
        if (ctx->opt_profile && open) RV_HIP(hipEventSynchronize(ctx->evk1));
        add();
    }
};

// The outputs whose null count a kernel leaves in a striped counter of the control block (MIN / MAX / AVG): eight to a read-back.
// `prepared`: a control block the caller has prepared and queued work on already (the group table's id pass and its error flag); the
// first eight counters are then its, and settle() hands the fetched block back for the caller to read that flag.
struct NullCounts {
    rv_ctx *ctx;
    std::vector<std::unique_ptr<rv_dcolumn>> &outs;
    std::vector<std::pair<uint32_t, int>> pending;  // (output, slot)
    Ctrl *ctrl;
    NullCounts(rv_ctx *c, std::vector<std::unique_ptr<rv_dcolumn>> &o, Ctrl *prepared = nullptr) : ctx(c), outs(o), ctrl(prepared) {}
    // attaches a zeroed bitmap to outs[j] and returns the counter its kernel adds the null results to
    unsigned long long *attach(uint32_t j, uint64_t n) {
        if (pending.size() == 8) settle();
        if (!ctrl) ctrl = prepare_ctrl(ctx, 0);
        const int slot = static_cast<int>(pending.size());
        outs[j]->validity = pool_alloc(ctx, zeroed_bitmap_bytes(n));
        RV_HIP(hipMemsetAsync(outs[j]->validity->ptr, 0, zeroed_bitmap_bytes(n), ctx->stream));
        pending.emplace_back(j, slot);
        return striped(ctx, &ctrl->valid_pop[slot]);
    }
    // reads the null counts of the outputs queued so far; the fetched block, or nullptr when none was queued and nothing was fetched
    const Ctrl *settle() {
        if (pending.empty()) return nullptr;
        const Ctrl *hc = fetch_ctrl(ctx);
        for (const auto &w : pending) {
            outs[w.first]->null_count = static_cast<int64_t>(hc->valid_pop[w.second]);
            if (outs[w.first]->null_count == 0) outs[w.first]->validity.reset();  // attached iff some cell is null
        }
        pending.clear();
        ctrl = nullptr;
        return hc;
    }
};

// a column of `rows` rows without nulls over `buf`, by value: what a pass reads a working buffer through
inline rv_dcolumn plain_view(rv_dtype dtype, const DevBufRef &buf, uint64_t rows) {
    rv_dcolumn c;
    c.dtype = dtype;
    c.values = buf;
    c.length = rows;
    c.null_count = 0;
    return c;
}
// an Int64 column without nulls over the first `rows` rows of `buf`: the row ids an entry point hands out
inline rv_dcolumn *index_column(const DevBufRef &buf, uint64_t rows) { return new rv_dcolumn(plain_view(RV_INT64, buf, rows)); }

// every index of a key list names a column of the frame; `label`: "" or the list's name with a blank ("order ")
inline void check_key_columns(const char *who, const char *label, const uint32_t *key_cols, uint32_t nkeys, uint32_t ncols) {
    for (uint32_t k = 0; k < nkeys; ++k)
        require(key_cols[k] < ncols, RV_ERR_INVALID_ARG, fmt("%s: %skey %u is column %u of %u", who, label, k, key_cols[k], ncols));
}

// The body of a breaker's entry point behind its checks.  On any exception whatever was queued has run before its buffers go back to the
// pool, and the outputs made so far are freed and the caller's slots nulled: a failed call creates no outputs.
template <class Body>
void breaker_call(rv_ctx *ctx, rv_dcolumn **out, uint32_t nout, Body body) {
    try {
        body();
    } catch (...) {
        (void)hipStreamSynchronize(ctx->stream);
        drop_outputs(out, nout);
        throw;
    }
}

}  // namespace rvl
