// Window frames on the device: rv_window_frames -- COUNT / SUM / MIN / MAX / AVG over bounded and unbounded ROWS frames, FIRST_VALUE /
// LAST_VALUE and NTILE, next to everything rv_window computes and over the same sequence.  One unit of the backend library behind
// include/rivulus_gpu.h (gfx950 only; compiled with hipcc).  The sequence, the heads, the checks and ops 0 .. 8 are window.hip's
// (window_passes.hpp); the kernels here are window_frame_kernel.hpp's, the case rule window_frame_rule.hpp's.
#include <map>
#include <tuple>

#include "window_frame_kernel.hpp"
#include "window_passes.hpp"

using namespace rvh;
using namespace rvl;

namespace rvl {
namespace {

// the three launches of K12's scan over scan indices (forward or mirrored)
template <uint32_t OP>
void launch_frame_scan(rv_ctx *ctx, const rvk::WfScanParams &p) {
    const dim3 grid(static_cast<uint32_t>(p.ntiles)), block(rvk::kWinThreads);
    hipLaunchKernelGGL(rvk::window_frame_tile_agg<OP>, grid, block, 0, ctx->stream, p);
    RV_HIP(hipGetLastError());
    hipLaunchKernelGGL(rvk::window_carry_scan<OP>, dim3(1), block, 0, ctx->stream, static_cast<const rvk::WinTriple *>(p.tile_agg), p.ntiles, p.carry);
    RV_HIP(hipGetLastError());
    hipLaunchKernelGGL(rvk::window_frame_apply<OP>, grid, block, 0, ctx->stream, p);
    RV_HIP(hipGetLastError());
}

void launch_frame_scan(rv_ctx *ctx, uint32_t op, const rvk::WfScanParams &p) {
    if (op == rvwin::WC_ADD_F64) launch_frame_scan<rvwin::WC_ADD_F64>(ctx, p);
    else if (op == rvwin::WC_MIN_U64) launch_frame_scan<rvwin::WC_MIN_U64>(ctx, p);
    else if (op == rvwin::WC_MAX_U64) launch_frame_scan<rvwin::WC_MAX_U64>(ctx, p);
    else launch_frame_scan<rvwin::WC_ADD_I64>(ctx, p);
}

struct Gathered {  // a value column in sequence order
    rvk::WfCells cells{};
    DevBufRef values, validity;
};
struct Scanned {  // value and non-null count per position
    DevBufRef value, count;
    const uint64_t *d_value() const { return value ? static_cast<const uint64_t *>(value->ptr) : nullptr; }
    const uint32_t *d_count() const { return count ? static_cast<const uint32_t *>(count->ptr) : nullptr; }
};

uint32_t scan_op(uint32_t op, const rv_dcolumn *col) {
    if (op == RV_WINF_MIN) return rvwin::WC_MIN_U64;
    if (op == RV_WINF_MAX) return rvwin::WC_MAX_U64;
    return col->dtype == RV_FLOAT64 ? rvwin::WC_ADD_F64 : rvwin::WC_ADD_I64;  // COUNT over a column that is no number: only the counts are kept
}

}  // namespace

rv_dtype window_frame_dtype(uint32_t op, const rv_dcolumn *col) {
    if (op == RV_WINF_AVG) return RV_FLOAT64;
    if (op == RV_WINF_COUNT || op == RV_WINF_NTILE) return RV_INT64;
    return col->dtype;
}

void window_frame_passes(rv_ctx *ctx, const Sequence &q, const rv_dcolumn *const *cols, const rv_window_frame_spec *specs, uint32_t nspecs,
                         std::vector<std::unique_ptr<rv_dcolumn>> &outs, NullCounts &nulls, std::vector<IndexGather> &gathers, PassTimer &timer) {
    const uint64_t n = q.n;
    const uint64_t nwords = (n + 63) / 64, ntiles = (n + rvk::kWinTileRows - 1) / rvk::kWinTileRows;
    const dim3 lanes(static_cast<uint32_t>((n + rvk::kWinThreads - 1) / rvk::kWinThreads)), block(rvk::kWinThreads);
    const uint64_t *part_heads = static_cast<const uint64_t *>(q.part_heads->ptr);
    DevBufRef tile_agg = pool_alloc(ctx, ntiles * sizeof(rvk::WinTriple) + 16), carry = pool_alloc(ctx, ntiles * sizeof(rvk::WinTriple) + 16);
    rvk::WfScanParams base{};
    base.n = n;
    base.ntiles = ntiles;
    base.tile_agg = static_cast<rvk::WinTriple *>(tile_agg->ptr);
    base.carry = static_cast<rvk::WinTriple *>(carry->ptr);

    // 1. the partition geometry: head_pos and tail_pos of every position (without partition keys there is one partition: 0 and n - 1)
    DevBufRef head_pos, tail_pos;
    if (q.ids) {
        head_pos = pool_alloc(ctx, n * 4 + 16);
        tail_pos = pool_alloc(ctx, n * 4 + 16);
        rvk::WfScanParams g = base;
        g.heads = part_heads;
        g.src = rvk::WFS_HEAD_POS;
        g.out32 = static_cast<uint32_t *>(head_pos->ptr);
        launch_frame_scan<rvwin::WC_MAX_U64>(ctx, g);
        g.src = rvk::WFS_TAIL_POS;
        g.mirrored = 1;
        g.out32 = static_cast<uint32_t *>(tail_pos->ptr);
        launch_frame_scan<rvwin::WC_MIN_U64>(ctx, g);
        timer.launches += 6;
    }

    std::map<uint32_t, Gathered> gathered;                                     // by column index
    std::map<uint32_t, DevBufRef> block_heads;                                 // by width (1 <= width < n)
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, Scanned> scans;  // by (column, scan op, width or 0: the partitions, mirrored)

    auto cells_of = [&](uint32_t ci) -> const Gathered & {  // one gather per distinct value column; in place: the column itself
        auto it = gathered.find(ci);
        if (it != gathered.end()) return it->second;
        const rv_dcolumn *col = cols[ci];
        Gathered g;
        const bool numeric = is_value_type(col->dtype);
        g.cells.all_null = col->dtype == RV_NULL;
        if (g.cells.all_null) {
        } else if (!q.perm) {
            g.cells.values = numeric ? static_cast<const uint64_t *>(col->values->ptr) : nullptr;
            g.cells.validity = col->validity ? static_cast<const uint8_t *>(col->validity->ptr) : nullptr;
            g.cells.offset = col->offset;
        } else {
            rvk::WfGatherParams p{};
            p.perm = q.d_perm();
            p.col = dev_view(col);
            p.n = n;
            if (numeric) {
                g.values = pool_alloc(ctx, n * 8 + 16);
                p.cells = static_cast<uint64_t *>(g.values->ptr);
            }
            if (col->validity) {
                g.validity = pool_alloc(ctx, nwords * 8 + 16);
                p.validity = static_cast<uint64_t *>(g.validity->ptr);
            }
            if (p.cells || p.validity) {
                hipLaunchKernelGGL(rvk::window_frame_gather, lanes, block, 0, ctx->stream, p);
                RV_HIP(hipGetLastError());
                ++timer.launches;
            }
            g.cells.values = p.cells;
            g.cells.validity = reinterpret_cast<const uint8_t *>(p.validity);
        }
        return gathered.emplace(ci, std::move(g)).first->second;
    };
    auto heads_of = [&](uint32_t width) -> const uint64_t * {  // width 0: the partitions
        if (!width) return part_heads;
        auto it = block_heads.find(width);
        if (it == block_heads.end()) {
            it = block_heads.emplace(width, pool_alloc(ctx, nwords * 8 + 16)).first;
            rvk::WfBlockHeadsParams p{};
            p.part_heads = part_heads;
            p.head_pos = head_pos ? static_cast<const uint32_t *>(head_pos->ptr) : nullptr;
            p.n = n;
            p.width = width;
            p.block_heads = static_cast<uint64_t *>(it->second->ptr);
            hipLaunchKernelGGL(rvk::window_frame_block_heads, lanes, block, 0, ctx->stream, p);
            RV_HIP(hipGetLastError());
            ++timer.launches;
        }
        return static_cast<const uint64_t *>(it->second->ptr);
    };
    auto scan_of = [&](uint32_t ci, uint32_t op, uint32_t width, uint32_t mirrored) -> const Scanned & {
        const auto key = std::make_tuple(ci, op, width, mirrored);
        auto it = scans.find(key);
        if (it != scans.end()) return it->second;
        const rv_dcolumn *col = cols[ci];
        const bool numeric = is_value_type(col->dtype);
        Scanned s;
        rvk::WfScanParams p = base;
        p.cells = cells_of(ci).cells;
        p.heads = heads_of(width);
        p.src = numeric ? rvk::WFS_CELL : rvk::WFS_VALID;
        p.mirrored = mirrored;
        p.is_float = col->dtype == RV_FLOAT64;
        p.is_max = op == rvwin::WC_MAX_U64;
        if (numeric) {
            s.value = pool_alloc(ctx, n * 8 + 16);
            p.out_value = static_cast<uint64_t *>(s.value->ptr);
        }
        s.count = pool_alloc(ctx, n * 4 + 16);
        p.out32 = static_cast<uint32_t *>(s.count->ptr);
        launch_frame_scan(ctx, op, p);
        timer.launches += 3;
        return scans.emplace(key, std::move(s)).first->second;
    };

    // 2. the expressions
    for (uint32_t j = 0; j < nspecs; ++j) {
        const uint32_t op = specs[j].op;
        if (!is_window_frame_op(op)) continue;
        const rv_dcolumn *col = cols[specs[j].col];
        rvk::WfCombineParams c{};
        c.perm = q.d_perm();
        c.head_pos = head_pos ? static_cast<const uint32_t *>(head_pos->ptr) : nullptr;
        c.tail_pos = tail_pos ? static_cast<const uint32_t *>(tail_pos->ptr) : nullptr;
        c.n = n;
        c.buckets = specs[j].offset;
        if (op != RV_WINF_NTILE) c.frame = rvframe::frame_of(specs[j].preceding, specs[j].following);
        if (op == RV_WINF_FIRST_VALUE || op == RV_WINF_LAST_VALUE) {
            c.fin = op == RV_WINF_FIRST_VALUE ? rvk::WFO_FIRST : rvk::WFO_LAST;
            gathers.push_back(IndexGather{j, pool_alloc(ctx, n * 8 + 16)});
            c.out = static_cast<uint64_t *>(gathers.back().idx->ptr);
        } else {
            outs[j] = new_value_column(ctx, window_frame_dtype(op, col), n);
            c.out = static_cast<uint64_t *>(outs[j]->values->ptr);
            if (op == RV_WINF_NTILE) c.fin = rvk::WFO_NTILE;
            else {
                c.op = scan_op(op, col);
                c.is_float = col->dtype == RV_FLOAT64;
                c.fin = op == RV_WINF_COUNT ? rvk::WFO_COUNT : op == RV_WINF_SUM ? rvk::WFO_VALUE : op == RV_WINF_AVG ? rvk::WFO_AVG : rvk::WFO_MINMAX;
                // a width of n and more cuts no partition: its blocks are the partitions, as with an unbounded side
                const uint32_t width = c.frame.width && c.frame.width < n ? static_cast<uint32_t>(c.frame.width) : 0;
                if (!c.frame.following_unbounded || c.frame.preceding_unbounded) {
                    const Scanned &s = scan_of(specs[j].col, c.op, width, 0);
                    c.prefix_value = s.d_value();
                    c.prefix_count = s.d_count();
                }
                if (!c.frame.preceding_unbounded) {
                    const Scanned &s = scan_of(specs[j].col, c.op, width, 1);
                    c.suffix_value = s.d_value();
                    c.suffix_count = s.d_count();
                }
                if (c.fin == rvk::WFO_MINMAX || c.fin == rvk::WFO_AVG) {
                    c.nulls = nulls.attach(j, n);
                    c.out_validity = static_cast<uint64_t *>(outs[j]->validity->ptr);
                }
            }
        }
        hipLaunchKernelGGL(rvk::window_frame, lanes, block, 0, ctx->stream, c);
        RV_HIP(hipGetLastError());
        ++timer.launches;
    }
}

}  // namespace rvl

extern "C" {

rv_status rv_window_frames(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const uint32_t *partition_cols, uint32_t npart,
                           const uint32_t *order_cols, const uint32_t *order_flags, uint32_t norder, const rv_window_frame_spec *specs,
                           uint32_t nspecs, rv_dcolumn **out) {
    return guarded([&] {
        window_call("rv_window_frames", RV_WINF_NTILE, ctx, cols, ncols, partition_cols, npart, order_cols, order_flags, norder, specs, nspecs, out);
    });
}

}  // extern "C"
