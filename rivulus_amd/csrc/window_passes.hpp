// What window.hip and window_frame.hip share on the host side: the sequence of a call, the timer round its passes, the read-back of the
// null counts, and the two halves of the operator.  rv_window and rv_window_frames both run window_call (window.hip); the expressions
// with a frame op (RV_WINF_COUNT and up) are window_frame_passes' (window_frame.hip), over the same sequence.
#pragma once

#include "launch.hpp"
#include "window_frame_rule.hpp"
#include "window_kernel.hpp"

namespace rvl {

// the rows of a call in window order, and where its partitions and peer groups begin
struct Sequence {
    uint64_t n = 0;
    DevBufRef ids;   // Int64 partition id per row; null: one partition
    DevBufRef perm;  // null: the identity
    DevBufRef part_heads, peer_heads;
    const uint64_t *d_perm() const { return perm ? static_cast<const uint64_t *>(perm->ptr) : nullptr; }
    const int64_t *d_ids() const { return ids ? static_cast<const int64_t *>(ids->ptr) : nullptr; }
};

// events around the window's own passes (option profile_kernels); the sorts before them time themselves
struct PassTimer {
    rv_ctx *ctx;
    uint64_t launches = 0;
    bool open = false;
    explicit PassTimer(rv_ctx *c) : ctx(c) {}
    void start() {
        if (ctx->opt_profile) RV_HIP(hipEventRecord(ctx->evk0, ctx->stream));
        open = true;
    }
    void stop_after_wait_for(hipStream_t s) {
        if (!open) return;
        open = false;
        if (!ctx->opt_profile) return;
        RV_HIP(hipEventRecord(ctx->evk1, s));
        RV_HIP(hipEventSynchronize(ctx->evk1));
        float ms = 0.f;
        RV_HIP(hipEventElapsedTime(&ms, ctx->evk0, ctx->evk1));
        ctx->kernel_ms += ms;
        ctx->kernel_launches += launches;
        launches = 0;
    }
};

// the outputs whose null count a kernel leaves in a striped counter of the control block (MIN / MAX / AVG): eight to a read-back
struct NullCounts {
    rv_ctx *ctx;
    std::vector<std::unique_ptr<rv_dcolumn>> &outs;
    std::vector<std::pair<uint32_t, int>> pending;  // (output, slot)
    Ctrl *ctrl = nullptr;
    NullCounts(rv_ctx *c, std::vector<std::unique_ptr<rv_dcolumn>> &o) : ctx(c), outs(o) {}
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
    void settle() {  // read the null counts of the outputs queued so far
        if (pending.empty()) return;
        const Ctrl *hc = fetch_ctrl(ctx);
        for (const auto &w : pending) {
            outs[w.first]->null_count = static_cast<int64_t>(hc->valid_pop[w.second]);
            if (outs[w.first]->null_count == 0) outs[w.first]->validity.reset();  // attached iff some cell is null
        }
        pending.clear();
        ctrl = nullptr;
    }
};

// a LAG / LEAD / FIRST_VALUE / LAST_VALUE whose nullable index list is made: gathered once the passes are timed
struct IndexGather {
    uint32_t j;
    DevBufRef idx;
};

inline bool is_window_shift(uint32_t op) { return op == RV_WIN_LAG || op == RV_WIN_LEAD; }
inline bool is_window_frame_op(uint32_t op) { return op >= RV_WINF_COUNT && op <= RV_WINF_NTILE; }

// ---- window.hip ----------------------------------------------------------------------------------------------------------------------
// every check of rv_window / rv_window_frames under the caller's name `who` (ops above `op_most` are unknown), then the operator
void window_call(const char *who, uint32_t op_most, rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const uint32_t *partition_cols,
                 uint32_t npart, const uint32_t *order_cols, const uint32_t *order_flags, uint32_t norder, const rv_window_frame_spec *specs,
                 uint32_t nspecs, rv_dcolumn **out);

// ---- window_frame.hip ----------------------------------------------------------------------------------------------------------------
// the dtype of a frame op's output over `col`
rv_dtype window_frame_dtype(uint32_t op, const rv_dcolumn *col);
// the expressions with a frame op, over a sequence whose partition heads are made: their outputs into `outs`, FIRST / LAST as index lists
// into `gathers`
void window_frame_passes(rv_ctx *ctx, const Sequence &q, const rv_dcolumn *const *cols, const rv_window_frame_spec *specs, uint32_t nspecs,
                         std::vector<std::unique_ptr<rv_dcolumn>> &outs, NullCounts &nulls, std::vector<IndexGather> &gathers, PassTimer &timer);

}  // namespace rvl
