// What window.hip and window_frame.hip share on the host side: the sequence of a call and the two halves of the operator; the timer round
// its passes and the read-back of the null counts are every breaker's (breaker_steps.hpp).  rv_window and rv_window_frames both run
// window_call (window.hip); the expressions with a frame op (RV_WINF_COUNT and up) are window_frame_passes' (window_frame.hip), over the
// same sequence.
#pragma once

#include "breaker_steps.hpp"
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
