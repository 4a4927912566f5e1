// Top-k on the device: rv_top_k_indices (the first k rows of rv_sort_indices) and rv_top_k (the first k rows of rv_sort) without sorting
// the column: a radix select over the first key finds a small set of candidate rows that holds the answer, and the existing sort and
// gather settle the rest.  One unit of the backend library behind include/rivulus_gpu.h (gfx950 only; compiled with hipcc).  Shared helpers
// are declared in launch.hpp (namespace rvl), the steps every breaker's unit takes in breaker_steps.hpp; the kernels and the shape of the
// passes are in topk_kernel.hpp, the decisions in topk_rule.hpp.  Both sorts here, of the whole column and of the candidates, are sort_chain.
#include "breaker_steps.hpp"
#include "topk_kernel.hpp"

using namespace rvh;
using namespace rvl;

namespace rvl {
namespace {

static_assert(rvk::TOPK_OUT_WORDS <= 8, "topk_plan's words fit Ctrl::valid_pop");
static_assert(rvk::kTopKTileRows == 256 * rvt::kTopKCollectRowsPerLane, "a tile is one workgroup x rvt::kTopKCollectRowsPerLane rows per lane");

struct Candidates {
    DevBufRef rows;      // ascending row ids, Int64
    uint64_t count = 0;
    uint64_t passes = 0;  // passes over the key column: topk_hist and every topk_refine
    bool selected = false;  // false: the caller sorts the whole column
};

// The select over `key`, 0 < k < n: the candidate rows are the first `count` rows of the sort by this key, as a set -- every row that ties
// with the last of them included.  One read-back per pass over the column; one more for the collect's total.
Candidates select_candidates(rv_ctx *ctx, const rv_dcolumn *key, uint32_t flags, uint64_t k, uint64_t divisor) {
    Candidates res;
    const uint64_t n = key->length;
    const bool nulls_last = (flags & RV_SORT_NULLS_LAST) != 0;
    const uint64_t flip = (flags & RV_SORT_DESCENDING) ? ~0ull : 0ull;
    constexpr size_t kHistBytes = static_cast<size_t>(rvk::kSortPositions) * rvk::kSortDigits * 8;
    DevBufRef hist = pool_alloc(ctx, kHistBytes), pass_hist = pool_alloc(ctx, rvk::kSortDigits * 8), scan_total = pool_alloc(ctx, 16);
    RV_HIP(hipMemsetAsync(hist->ptr, 0, kHistBytes, ctx->stream));
    Ctrl *ctrl = prepare_ctrl(ctx, 0);
    PassTimer timer(ctx);
    timer.start();
    const dim3 grid(grid_for_words(ctx, n, rvk::kTopKThreads)), block(rvk::kTopKThreads);

    rvk::TopKHistParams hp{};
    hp.key = dev_view(key);
    hp.n = n;
    hp.flip = flip;
    hp.hist = static_cast<unsigned long long *>(hist->ptr);
    hipLaunchKernelGGL(rvk::topk_hist, grid, block, 0, ctx->stream, hp);
    RV_HIP(hipGetLastError());
    rvk::TopKPlanParams pp{};
    pp.hist = hp.hist;
    pp.n = n;
    pp.k = k;
    pp.nulls_last = nulls_last ? 1u : 0u;
    pp.out = &ctrl->valid_pop[0];
    hipLaunchKernelGGL(rvk::topk_plan<true>, dim3(1), block, 0, ctx->stream, pp);
    RV_HIP(hipGetLastError());
    timer.launches += 2;
    const Ctrl *h = fetch_ctrl(ctx);
    res.passes = 1;
    const uint64_t valid_rows = h->valid_pop[rvk::TOPK_OUT_VALID], mask = h->valid_pop[rvk::TOPK_OUT_MASK];
    const uint64_t null_rows = n - valid_rows;
    const rvtopk::NullClass nc = rvtopk::null_class(n, valid_rows, k, nulls_last);

    rvk::TopKCollectParams cp{};
    cp.key = hp.key;
    cp.n = n;
    cp.flip = flip;
    uint64_t count = n;
    if (nc.kind == rvtopk::kNullsOnly) {
        cp.take_nulls = 1;
        count = null_rows;
    } else if (nc.kind == rvtopk::kValues) {
        uint64_t prefix = h->valid_pop[rvk::TOPK_OUT_PREFIX], below = h->valid_pop[rvk::TOPK_OUT_BELOW], in_bin = h->valid_pop[rvk::TOPK_OUT_IN_BIN];
        uint32_t pos = static_cast<uint32_t>(h->valid_pop[rvk::TOPK_OUT_POS]);
        uint64_t owed = nc.r - below;  // of the rows of the chosen bin
        const uint64_t nulls_taken = nc.nulls_taken ? null_rows : 0;
        count = nulls_taken + below + in_bin;
        uint64_t remaining = mask & ((1ull << pos) - 1);
        while (rvtopk::refine_more(count, n, divisor, remaining)) {
            const uint32_t next = rvtopk::highest_position(remaining);
            RV_HIP(hipMemsetAsync(pass_hist->ptr, 0, rvk::kSortDigits * 8, ctx->stream));
            rvk::TopKRefineParams rp{};
            rp.key = hp.key;
            rp.n = n;
            rp.flip = flip;
            rp.prefix = prefix;
            rp.pos = next;
            rp.hist = static_cast<unsigned long long *>(pass_hist->ptr);
            hipLaunchKernelGGL(rvk::topk_refine, grid, block, 0, ctx->stream, rp);
            RV_HIP(hipGetLastError());
            rvk::TopKPlanParams qp{};
            qp.hist = rp.hist;
            qp.r = owed;
            qp.prefix = prefix;
            qp.pos = next;
            qp.out = &ctrl->valid_pop[0];
            hipLaunchKernelGGL(rvk::topk_plan<false>, dim3(1), block, 0, ctx->stream, qp);
            RV_HIP(hipGetLastError());
            timer.launches += 2;
            h = fetch_ctrl(ctx);
            ++res.passes;
            prefix = h->valid_pop[rvk::TOPK_OUT_PREFIX];
            const uint64_t shed_below = h->valid_pop[rvk::TOPK_OUT_BELOW];
            count += shed_below + h->valid_pop[rvk::TOPK_OUT_IN_BIN] - in_bin;  // the bin refined into the part below its new bin and that bin
            in_bin = h->valid_pop[rvk::TOPK_OUT_IN_BIN];
            owed -= shed_below;
            pos = next;
            remaining &= ~(1ull << next);
        }
        cp.take_values = 1;
        cp.take_nulls = nulls_taken ? 1u : 0u;
        cp.pos = pos;
        cp.limit = rvtopk::high_from(prefix, pos);
    }
    if (nc.kind == rvtopk::kEveryRow || count >= n || count > n / 2) return res;  // the whole sort is no dearer than this many candidates

    const uint32_t ntiles = static_cast<uint32_t>((n + rvk::kTopKTileRows - 1) / rvk::kTopKTileRows);
    DevBufRef tile_counts = pool_alloc(ctx, static_cast<size_t>(ntiles) * 4 + 16);
    res.rows = pool_alloc(ctx, std::max<size_t>(count * 8, 16));
    cp.tile_counts = static_cast<uint32_t *>(tile_counts->ptr);
    cp.out = static_cast<int64_t *>(res.rows->ptr);
    cp.capacity = count;
    hipLaunchKernelGGL(rvk::topk_tile_count, dim3(ntiles), block, 0, ctx->stream, cp);
    RV_HIP(hipGetLastError());
    DevBufRef bases;
    device_exclusive_scan(ctx, cp.tile_counts, ntiles, bases, false, false, static_cast<unsigned long long *>(scan_total->ptr));
    cp.bases = static_cast<const uint64_t *>(bases->ptr);
    hipLaunchKernelGGL(rvk::topk_collect, dim3(ntiles), block, 0, ctx->stream, cp);
    RV_HIP(hipGetLastError());
    timer.launches += 5;
    timer.stop();
    uint64_t collected = 0;
    RV_HIP(hipMemcpyAsync(&collected, scan_total->ptr, 8, hipMemcpyDeviceToHost, ctx->stream));
    RV_HIP(hipStreamSynchronize(ctx->stream));  // the working buffers go back to the pool
    timer.add();
    require(collected == count, RV_ERR_INTERNAL,
            fmt("top-k: the collect found %llu candidates, the plan %llu", static_cast<unsigned long long>(collected), static_cast<unsigned long long>(count)));
    res.count = count;
    res.selected = true;
    return res;
}

// The first min(k, n) rows of the sort by (keys[0], keys[1], ...) as Int64 row ids in a buffer of at least that many rows.
DevBufRef top_k_rows(rv_ctx *ctx, const rv_dcolumn *const *keys, const uint32_t *flags, uint32_t nkeys, uint64_t k, uint64_t *rows_out) {
    const uint64_t n = keys[0]->length, kk = std::min(k, n);
    *rows_out = kk;
    ctx->top_k_last_passes = 0;
    ctx->top_k_last_candidates = 0;
    if (kk == 0) return pool_alloc(ctx, 16);
    const uint64_t select_from = ctx->opt_top_k_select_from_rows > 0 ? static_cast<uint64_t>(ctx->opt_top_k_select_from_rows) : rvt::kTopKSelectFromRows;
    const uint64_t divisor = ctx->opt_top_k_refine_divisor > 0 ? static_cast<uint64_t>(ctx->opt_top_k_refine_divisor) : rvt::kTopKRefineDivisor;
    Candidates cand;
    if (n >= select_from && kk < n - kk) cand = select_candidates(ctx, keys[0], flags[0], kk, divisor);
    if (!cand.selected) {  // the whole sort; the caller keeps the first kk rows of it
        ctx->top_k_last_candidates = n;
        return sort_chain(ctx, keys, flags, nkeys);
    }
    // every key at the candidates, the chain of stable sorts from the last key to the first over those few rows, and the candidates' row
    // ids through the permutation: ties of the first key that straddle the cut are all candidates, so the later keys decide them
    const uint64_t *d_cand = static_cast<const uint64_t *>(cand.rows->ptr);
    std::vector<rv_dcolumn *> at_cand(nkeys, nullptr);
    std::vector<std::unique_ptr<rv_dcolumn>> gathered(nkeys);
    for (uint32_t j = 0; j < nkeys; ++j) {
        take_on_device(ctx, &keys[j], 1, d_cand, cand.count, &at_cand[j], false);
        gathered[j].reset(at_cand[j]);
    }
    DevBufRef perm = sort_chain(ctx, at_cand.data(), flags, nkeys);
    const rv_dcolumn ids = plain_view(RV_INT64, cand.rows, cand.count);
    const rv_dcolumn *ids_ptr = &ids;
    rv_dcolumn *first = nullptr;
    take_on_device(ctx, &ids_ptr, 1, static_cast<const uint64_t *>(perm->ptr), kk, &first, false);
    std::unique_ptr<rv_dcolumn> owned(first);
    RV_HIP(hipStreamSynchronize(ctx->stream));  // the candidates and the permutation go back to the pool
    ctx->top_k_last_passes = cand.passes;
    ctx->top_k_last_candidates = cand.count;
    ctx->last_kernel = "topk_collect";
    return owned->values;
}

}  // namespace
}  // namespace rvl

extern "C" {

rv_status rv_top_k_indices(rv_ctx *ctx, const rv_dcolumn *key, uint32_t flags, uint64_t k, rv_dcolumn **out_indices) {
    return guarded([&] {
        require(ctx && key && out_indices, RV_ERR_INVALID_ARG, "rv_top_k_indices: NULL argument");
        *out_indices = nullptr;
        check_sort_key(key, flags, "rv_top_k_indices");
        set_device(ctx);
        breaker_call(ctx, out_indices, 1, [&] {
            uint64_t rows = 0;
            DevBufRef idx = top_k_rows(ctx, &key, &flags, 1, k, &rows);
            *out_indices = index_column(idx, rows);
        });
    });
}

rv_status rv_top_k(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const uint32_t *key_cols, const uint32_t *key_flags, uint32_t nkeys,
                   uint64_t k, rv_dcolumn **out) {
    return guarded([&] {
        require(ctx && cols && out && (nkeys == 0 || (key_cols && key_flags)), RV_ERR_INVALID_ARG, "rv_top_k: NULL argument");
        require(nkeys >= 1, RV_ERR_INVALID_ARG, "rv_top_k: no sort keys");
        check_batch(cols, ncols);
        check_key_columns("rv_top_k", "", key_cols, nkeys, ncols);
        for (uint32_t j = 0; j < nkeys; ++j) check_sort_key(cols[key_cols[j]], key_flags[j], "rv_top_k");
        for (uint32_t c = 0; c < ncols; ++c) out[c] = nullptr;
        set_device(ctx);
        breaker_call(ctx, out, ncols, [&] {
            std::vector<const rv_dcolumn *> keys(nkeys);
            for (uint32_t j = 0; j < nkeys; ++j) keys[j] = cols[key_cols[j]];
            uint64_t rows = 0;
            DevBufRef idx = top_k_rows(ctx, keys.data(), key_flags, nkeys, k, &rows);
            const std::string name = ctx->last_kernel;
            take_on_device(ctx, cols, ncols, static_cast<const uint64_t *>(idx->ptr), rows, out, false);
            RV_HIP(hipStreamSynchronize(ctx->stream));  // the index list goes back to the pool
            ctx->last_kernel = name;
        });
    });
}

}  // extern "C"
