// Window functions on the device: rv_window -- rank, running aggregates and lag / lead over PARTITION BY ... ORDER BY.  One unit of the
// backend library behind include/rivulus_gpu.h (gfx950 only; compiled with hipcc).  Shared helpers are declared in launch.hpp (namespace
// rvl); the kernels, the shape of the passes and the bracketing of the scan are in window_kernel.hpp, the combine in window_combine.hpp.
// The partition ids are rv_group_ids_keys' (group_agg.hip), the sequence is sort_chain (sort.hip) over the ids and the order keys, the
// timer and the null counts are breaker_steps.hpp's, LAG / LEAD gather through
// take_nullable_on_device (take_nullable.hip): what is new here is the heads pass, the segmented scan and the shift.
#include "window_passes.hpp"

using namespace rvh;
using namespace rvl;

namespace rvl {
namespace {

static_assert(rvk::kWinTileRows == rvk::kWinThreads * rvk::kWinItems, "a tile is one workgroup x kWinItems positions per thread");
static_assert(sizeof(rvk::WinTriple) == 24, "tile aggregates and carries are 24-byte records");

template <uint32_t OP>
void launch_scan(rv_ctx *ctx, const rvk::WinScanParams &p) {
    const dim3 grid(static_cast<uint32_t>(p.ntiles)), block(rvk::kWinThreads);
    hipLaunchKernelGGL(rvk::window_tile_agg<OP>, grid, block, 0, ctx->stream, p);
    RV_HIP(hipGetLastError());
    hipLaunchKernelGGL(rvk::window_carry_scan<OP>, dim3(1), block, 0, ctx->stream, static_cast<const rvk::WinTriple *>(p.tile_agg), p.ntiles, p.carry);
    RV_HIP(hipGetLastError());
    hipLaunchKernelGGL(rvk::window_apply<OP>, grid, block, 0, ctx->stream, p);
    RV_HIP(hipGetLastError());
}

void window(const char *who, rv_ctx *ctx, const rv_dcolumn *const *cols, const uint32_t *partition_cols, uint32_t npart, const uint32_t *order_cols,
            const uint32_t *order_flags, uint32_t norder, const rv_window_frame_spec *specs, uint32_t nspecs, rv_dcolumn **out) {
    Sequence q;
    q.n = cols[0]->length;
    const uint64_t n = q.n;
    std::vector<std::unique_ptr<rv_dcolumn>> outs(nspecs);
    if (n == 0) {  // zero-row outputs of the right dtypes
        for (uint32_t j = 0; j < nspecs; ++j) {
            const rv_dcolumn *col = cols[specs[j].col];
            if (is_window_shift(specs[j].op) || specs[j].op == RV_WINF_FIRST_VALUE || specs[j].op == RV_WINF_LAST_VALUE) {
                rv_dcolumn *o = nullptr;
                take_nullable_on_device(ctx, &col, 1, nullptr, 0, &o, false, IndexNulls{});
                outs[j].reset(o);
            } else if (is_window_frame_op(specs[j].op)) {
                outs[j] = new_value_column(ctx, window_frame_dtype(specs[j].op, col), 0);
            } else {
                outs[j] = new_value_column(ctx, specs[j].op >= RV_WIN_CUM_SUM ? col->dtype : RV_INT64, 0);
            }
        }
        RV_HIP(hipStreamSynchronize(ctx->stream));
        for (uint32_t j = 0; j < nspecs; ++j) out[j] = outs[j].release();
        ctx->last_kernel.clear();
        return;
    }

    // 1. the sequence: partition ids, then the sort's chain from the last order key to the first and over the ids last
    if (npart) {
        std::vector<const rv_dcolumn *> keys(npart);
        for (uint32_t k = 0; k < npart; ++k) keys[k] = cols[partition_cols[k]];
        q.ids = partition_ids(ctx, keys.data(), npart, who);
    }
    {
        const rv_dcolumn id_col = plain_view(RV_INT64, q.ids, n);
        std::vector<const rv_dcolumn *> keys;
        std::vector<uint32_t> flags;
        if (npart) keys.push_back(&id_col), flags.push_back(0);
        for (uint32_t k = 0; k < norder; ++k) keys.push_back(cols[order_cols[k]]), flags.push_back(order_flags[k]);
        q.perm = sort_chain(ctx, keys.data(), flags.data(), static_cast<uint32_t>(keys.size()));
    }

    PassTimer timer(ctx);
    timer.start();
    bool scanned = false, shifted = false, framed = false;

    // 2. the heads (needed by the scans and the frames only: the shift compares the ids themselves)
    bool any_scan = false;
    for (uint32_t j = 0; j < nspecs; ++j) any_scan = any_scan || !is_window_shift(specs[j].op);
    const uint64_t nwords = (n + 63) / 64, ntiles = (n + rvk::kWinTileRows - 1) / rvk::kWinTileRows;
    DevBufRef tile_agg, carry;
    if (any_scan) {
        q.part_heads = pool_alloc(ctx, nwords * 8 + 16);
        q.peer_heads = pool_alloc(ctx, nwords * 8 + 16);
        rvk::WinHeadsParams h{};
        h.perm = q.d_perm();
        h.ids = q.d_ids();
        h.n = n;
        h.norder = norder;
        for (uint32_t k = 0; k < norder; ++k) h.order[k] = dev_view(cols[order_cols[k]]);
        h.part_heads = static_cast<uint64_t *>(q.part_heads->ptr);
        h.peer_heads = static_cast<uint64_t *>(q.peer_heads->ptr);
        hipLaunchKernelGGL(rvk::window_heads, dim3(static_cast<uint32_t>((n + rvk::kWinThreads - 1) / rvk::kWinThreads)), dim3(rvk::kWinThreads), 0, ctx->stream, h);
        RV_HIP(hipGetLastError());
        ++timer.launches;
        tile_agg = pool_alloc(ctx, ntiles * sizeof(rvk::WinTriple) + 16);
        carry = pool_alloc(ctx, ntiles * sizeof(rvk::WinTriple) + 16);
    }

    // 3. the scans, one spec after the other over the one sequence
    NullCounts nulls(ctx, outs);  // of the MIN / MAX outputs: the next read-back brings them
    for (uint32_t j = 0; j < nspecs; ++j) {
        const uint32_t op = specs[j].op;
        if (is_window_shift(op) || is_window_frame_op(op)) continue;
        const rv_dcolumn *col = cols[specs[j].col];
        rvk::WinScanParams p{};
        p.perm = q.d_perm();
        p.part_heads = static_cast<const uint64_t *>(q.part_heads->ptr);
        p.peer_heads = static_cast<const uint64_t *>(q.peer_heads->ptr);
        p.n = n;
        p.ntiles = ntiles;
        p.tile_agg = static_cast<rvk::WinTriple *>(tile_agg->ptr);
        p.carry = static_cast<rvk::WinTriple *>(carry->ptr);
        const bool numeric = op >= RV_WIN_CUM_SUM;
        outs[j] = new_value_column(ctx, numeric ? col->dtype : RV_INT64, n);
        p.out = static_cast<uint64_t *>(outs[j]->values->ptr);
        p.is_float = numeric && col->dtype == RV_FLOAT64;
        p.is_max = op == RV_WIN_CUM_MAX;
        switch (op) {
            case RV_WIN_ROW_NUMBER: p.src = rvk::WS_ONE; break;
            case RV_WIN_DENSE_RANK: p.src = rvk::WS_PEER; break;
            case RV_WIN_RANK: p.src = rvk::WS_PEER_POS, p.fin = rvk::WF_RANK; break;
            case RV_WIN_CUM_COUNT: p.src = rvk::WS_VALID, p.col = dev_view(col); break;
            default: p.src = rvk::WS_CELL, p.col = dev_view(col); break;
        }
        if (op == RV_WIN_CUM_MIN || op == RV_WIN_CUM_MAX) {
            p.fin = rvk::WF_MINMAX;
            p.nulls = nulls.attach(j, n);
            p.out_validity = static_cast<uint64_t *>(outs[j]->validity->ptr);
            if (op == RV_WIN_CUM_MIN) launch_scan<rvwin::WC_MIN_U64>(ctx, p);
            else launch_scan<rvwin::WC_MAX_U64>(ctx, p);
        }
        else if (op == RV_WIN_RANK) launch_scan<rvwin::WC_MAX_U64>(ctx, p);
        else if (op == RV_WIN_CUM_SUM && col->dtype == RV_FLOAT64) launch_scan<rvwin::WC_ADD_F64>(ctx, p);
        else launch_scan<rvwin::WC_ADD_I64>(ctx, p);
        timer.launches += 3;
        scanned = true;
    }

    // 4. the shifts: a nullable index list in row order, gathered like any other
    std::vector<IndexGather> shifts;
    for (uint32_t j = 0; j < nspecs; ++j) {
        if (!is_window_shift(specs[j].op)) continue;
        rvk::WinShiftParams s{};
        s.perm = q.d_perm();
        s.ids = q.d_ids();
        s.n = n;
        s.k = specs[j].offset;
        s.lead = specs[j].op == RV_WIN_LEAD;
        shifts.push_back(IndexGather{j, pool_alloc(ctx, n * 8 + 16)});
        s.idx = static_cast<uint64_t *>(shifts.back().idx->ptr);
        hipLaunchKernelGGL(rvk::window_shift, dim3(grid_for_words(ctx, n, rvk::kWinThreads)), dim3(rvk::kWinThreads), 0, ctx->stream, s);
        RV_HIP(hipGetLastError());
        ++timer.launches;
        shifted = true;
    }
    // 5. the frames, first / last value and ntile, over the same sequence
    for (uint32_t j = 0; j < nspecs; ++j) framed = framed || is_window_frame_op(specs[j].op);
    if (framed) window_frame_passes(ctx, q, cols, specs, nspecs, outs, nulls, shifts, timer);
    timer.stop_and_wait();
    nulls.settle();
    for (const IndexGather &s : shifts) {
        const rv_dcolumn *col = cols[specs[s.j].col];
        rv_dcolumn *o = nullptr;
        take_nullable_on_device(ctx, &col, 1, static_cast<const uint64_t *>(s.idx->ptr), n, &o, false, IndexNulls{});
        outs[s.j].reset(o);
    }
    RV_HIP(hipStreamSynchronize(ctx->stream));  // the sequence and the working buffers go back to the pool
    for (uint32_t j = 0; j < nspecs; ++j) out[j] = outs[j].release();
    ctx->last_kernel = framed ? "window_frame" : scanned ? "window_scan" : shifted ? "window_shift" : "";
}

}  // namespace

void window_call(const char *who, uint32_t op_most, rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const uint32_t *partition_cols,
                 uint32_t npart, const uint32_t *order_cols, const uint32_t *order_flags, uint32_t norder, const rv_window_frame_spec *specs,
                 uint32_t nspecs, rv_dcolumn **out) {
    const std::string w = who;
    require(ctx && cols && specs && out && (npart == 0 || partition_cols) && (norder == 0 || (order_cols && order_flags)), RV_ERR_INVALID_ARG,
            w + ": NULL argument");
    require(ncols >= 1, RV_ERR_INVALID_ARG, w + ": no columns");
    require(nspecs >= 1, RV_ERR_INVALID_ARG, w + ": no window expressions");
    check_batch(cols, ncols);
    check_key_columns(who, "partition ", partition_cols, npart, ncols);
    check_key_columns(who, "order ", order_cols, norder, ncols);
    require(norder <= static_cast<uint32_t>(rvk::kWinOrderKeysMost), RV_ERR_INVALID_ARG,
            fmt("%s: %u order keys; at most %d are taken", who, norder, rvk::kWinOrderKeysMost));
    for (uint32_t j = 0; j < nspecs; ++j) {
        require(specs[j].op <= op_most, RV_ERR_INVALID_ARG, fmt("%s: expression %u has the unknown op %u", who, j, specs[j].op));
        require(specs[j].col < ncols, RV_ERR_INVALID_ARG, fmt("%s: expression %u reads column %u of %u", who, j, specs[j].col, ncols));
        if (specs[j].op >= RV_WINF_COUNT && specs[j].op <= RV_WINF_LAST_VALUE)
            require(rvframe::frame_ok(specs[j].preceding, specs[j].following), RV_ERR_INVALID_ARG,
                    fmt("%s: expression %u: a frame's finite offsets are at most 2^62 in magnitude and preceding + following >= 0", who, j));
        if (specs[j].op == RV_WINF_NTILE) require(specs[j].offset >= 1, RV_ERR_INVALID_ARG, fmt("%s: expression %u: NTILE of 0 buckets", who, j));
    }
    require(cols[0]->length < (uint64_t{1} << 32), RV_ERR_UNSUPPORTED, w + ": frames of 2^32 rows or more are not supported (32-bit row ids inside, as the sort)");
    if (npart) {
        std::vector<const rv_dcolumn *> keys(npart);
        for (uint32_t k = 0; k < npart; ++k) keys[k] = cols[partition_cols[k]];
        check_partition_keys(keys.data(), npart, who);
    }
    for (uint32_t k = 0; k < norder; ++k) check_sort_key(cols[order_cols[k]], order_flags[k], who);
    for (uint32_t j = 0; j < nspecs; ++j) {
        const rv_dtype d = cols[specs[j].col]->dtype;
        const uint32_t op = specs[j].op;
        if (op >= RV_WIN_CUM_SUM && op <= RV_WIN_CUM_MAX)
            require(is_value_type(d), RV_ERR_TYPE_MISMATCH, fmt("%s: expression %u: CUM_SUM / CUM_MIN / CUM_MAX take an Int64 or Float64 column", who, j));
        else if (op >= RV_WINF_SUM && op <= RV_WINF_AVG)
            require(is_value_type(d), RV_ERR_TYPE_MISMATCH, fmt("%s: expression %u: SUM / MIN / MAX / AVG take an Int64 or Float64 column", who, j));
        else if (op == RV_WIN_CUM_COUNT || is_window_shift(op) || op == RV_WINF_COUNT || op == RV_WINF_FIRST_VALUE || op == RV_WINF_LAST_VALUE)
            require(is_value_type(d) || d == RV_BOOLEAN || d == RV_STRING || d == RV_NULL, RV_ERR_UNSUPPORTED, fmt("%s: expression %u: unsupported dtype", who, j));
    }
    for (uint32_t j = 0; j < nspecs; ++j) out[j] = nullptr;
    set_device(ctx);
    breaker_call(ctx, out, nspecs, [&] { window(who, ctx, cols, partition_cols, npart, order_cols, order_flags, norder, specs, nspecs, out); });
}

}  // namespace rvl

extern "C" {

rv_status rv_window(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const uint32_t *partition_cols, uint32_t npart,
                    const uint32_t *order_cols, const uint32_t *order_flags, uint32_t norder, const rv_window_spec *specs, uint32_t nspecs,
                    rv_dcolumn **out) {
    return guarded([&] {
        // the general form's specs: rv_window's one frame is ROWS UNBOUNDED PRECEDING .. CURRENT ROW, and its ops end at RV_WIN_LEAD
        std::vector<rv_window_frame_spec> general(specs ? size_t{nspecs} + 1 : 0);  // + 1: not NULL when nspecs == 0, which has its own text
        for (uint32_t j = 0; specs && j < nspecs; ++j) general[j] = rv_window_frame_spec{specs[j].op, specs[j].col, specs[j].offset, RV_FRAME_UNBOUNDED, 0};
        window_call("rv_window", RV_WIN_LEAD, ctx, cols, ncols, partition_cols, npart, order_cols, order_flags, norder,
                    specs ? general.data() : nullptr, nspecs, out);
    });
}

}  // extern "C"
