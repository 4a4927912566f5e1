// Sort on the device: rv_sort_indices (the stable permutation of a key column) and rv_sort (that permutation, chained over the keys,
// followed by the gather of take_concat.hip).  One unit of the backend library behind include/rivulus_gpu.h (gfx950 only; compiled with
// hipcc).  Shared helpers are declared in launch.hpp (namespace rvl), the steps every breaker's unit takes in breaker_steps.hpp; the
// kernels and the shape of the passes are in sort_kernel.hpp.  sort_chain is the chain for every unit that orders rows by several keys
// (topk.hip, window.hip).
#include <rocprim/device/device_radix_sort.hpp>

#include "breaker_steps.hpp"
#include "sort_kernel.hpp"

using namespace rvh;
using namespace rvl;

namespace rvl {
namespace {

constexpr uint32_t kSortFlagsKnown = RV_SORT_DESCENDING | RV_SORT_NULLS_LAST;
static_assert(rvk::kSortTileRows == 256 * rvt::kSortRowsPerLane, "a tile is one workgroup x rvt::kSortRowsPerLane rows per lane");

}  // namespace

// what every entry point that orders rows by a key column checks of it (rv_sort_indices, rv_sort, rv_top_k_indices, rv_top_k)
void check_sort_key(const rv_dcolumn *key, uint32_t flags, const char *what) {
    require((flags & ~kSortFlagsKnown) == 0, RV_ERR_INVALID_ARG, fmt("%s: unknown flag bits 0x%x", what, flags & ~kSortFlagsKnown));
    require(key->dtype == RV_INT64 || key->dtype == RV_FLOAT64 || key->dtype == RV_NULL, RV_ERR_UNSUPPORTED,
            fmt("%s: only Int64, Float64 (and Null) key columns are supported; Boolean and String sort keys are not built", what));
    require(key->length < (uint64_t{1} << 32), RV_ERR_UNSUPPORTED, fmt("%s: keys of 2^32 rows or more are not supported (32-bit row ids inside)", what));
}

namespace {

template <bool NULLS>
void launch_pass(rv_ctx *ctx, rvk::SortPassParams &p, bool last, DevBufRef &hist_total) {
    const dim3 grid(p.ntiles), block(rvk::kSortThreads);
    hipLaunchKernelGGL(rvk::sort_tile_hist<NULLS>, grid, block, 0, ctx->stream, p);
    RV_HIP(hipGetLastError());
    DevBufRef bases;
    device_exclusive_scan(ctx, p.tile_counts, static_cast<uint64_t>(p.nbins) * p.ntiles, bases, false, false, static_cast<unsigned long long *>(hist_total->ptr));
    p.bases = static_cast<const uint64_t *>(bases->ptr);
    if (last) hipLaunchKernelGGL((rvk::sort_scatter<NULLS, true>), grid, block, 0, ctx->stream, p);
    else if constexpr (!NULLS) hipLaunchKernelGGL((rvk::sort_scatter<false, false>), grid, block, 0, ctx->stream, p);
    RV_HIP(hipGetLastError());
    // (`bases` goes back to the pool; its next user runs behind the scatter on the stream)
}

}  // namespace

// The permutation as n Int64 rows.  `prior`: n device-resident indices, or nullptr.  Two waits: the plan (which passes run; a bad index
// of `prior`) and the end, after which the working buffers go back to the pool.
DevBufRef sort_indices(rv_ctx *ctx, const rv_dcolumn *key, uint32_t flags, const uint64_t *prior) {
    const uint64_t n = key->length;
    DevBufRef out = pool_alloc(ctx, std::max<size_t>(n * 8, 16));
    ctx->sort_last_passes = 0;
    if (n == 0) return out;
    const uint32_t ntiles = static_cast<uint32_t>((n + rvk::kSortTileRows - 1) / rvk::kSortTileRows);
    DevBufRef keys[2] = {pool_alloc(ctx, n * 8 + 16), pool_alloc(ctx, n * 8 + 16)};
    DevBufRef rows[2] = {pool_alloc(ctx, n * 4 + 16), pool_alloc(ctx, n * 4 + 16)};
    constexpr size_t kHistBytes = static_cast<size_t>(rvk::kSortPositions) * rvk::kSortDigits * 8;
    DevBufRef hist = pool_alloc(ctx, kHistBytes), scan_total = pool_alloc(ctx, 16);
    RV_HIP(hipMemsetAsync(hist->ptr, 0, kHistBytes, ctx->stream));
    Ctrl *ctrl = prepare_ctrl(ctx, 0);
    RV_HIP(hipMemsetAsync(&ctrl->pops[0], 0xFF, 8, ctx->stream));
    PassTimer timer(ctx);
    timer.start();

    rvk::SortMapParams m{};
    m.key = dev_view(key);
    m.prior = prior;
    m.n = n;
    m.flip = (flags & RV_SORT_DESCENDING) ? ~0ull : 0ull;
    m.keys = static_cast<uint64_t *>(keys[0]->ptr);
    m.rows = static_cast<uint32_t *>(rows[0]->ptr);
    m.hist = static_cast<unsigned long long *>(hist->ptr);
    m.first_bad = &ctrl->pops[0];
    hipLaunchKernelGGL(rvk::sort_map_hist, dim3(grid_for_words(ctx, n, rvk::kSortThreads)), dim3(rvk::kSortThreads), 0, ctx->stream, m);
    RV_HIP(hipGetLastError());
    hipLaunchKernelGGL(rvk::sort_plan, dim3(1), dim3(rvk::kSortThreads), 0, ctx->stream, static_cast<const unsigned long long *>(hist->ptr), &ctrl->pops[1], &ctrl->pops[2]);
    RV_HIP(hipGetLastError());
    const Ctrl *h = fetch_ctrl(ctx);
    if (h->pops[0] != ~0ull) {  // as take_on_device reports it: the first offending index
        uint64_t bad = 0;
        RV_HIP(hipMemcpyAsync(&bad, prior + h->pops[0], 8, hipMemcpyDeviceToHost, ctx->stream));
        RV_HIP(hipStreamSynchronize(ctx->stream));
        throw Error(RV_ERR_OUT_OF_BOUNDS, fmt("Index %llu out of bounds for %llu rows", static_cast<unsigned long long>(bad), static_cast<unsigned long long>(n)));
    }
    const uint64_t value_passes = h->pops[1], valid_rows = h->pops[2];
    const bool null_pass = valid_rows > 0 && valid_rows < n;

    timer.launches = 2;  // the map and the plan
    uint64_t scatters = 0;
    int cur = 0;
    std::string name;
    rvk::SortPassParams p{};
    p.key = m.key;
    p.n = n;
    p.ntiles = ntiles;
    p.index_out = static_cast<int64_t *>(out->ptr);
    p.null_digit = (flags & RV_SORT_NULLS_LAST) ? 1u : 0u;
    DevBufRef tile_counts = pool_alloc(ctx, static_cast<size_t>(rvk::kSortDigits) * ntiles * 4 + 16);
    p.tile_counts = static_cast<uint32_t *>(tile_counts->ptr);
    auto bind = [&] {
        p.keys_in = static_cast<const uint64_t *>(keys[cur]->ptr);
        p.rows_in = static_cast<const uint32_t *>(rows[cur]->ptr);
        p.keys_out = static_cast<uint64_t *>(keys[cur ^ 1]->ptr);
        p.rows_out = static_cast<uint32_t *>(rows[cur ^ 1]->ptr);
    };
    if (ctx->opt_sort_engine == 1) {  // the yardstick: the pair sort by rocPRIM over all 64 bits, everything around it unchanged
        bind();
        size_t temp_bytes = 0;
        RV_HIP(rocprim::radix_sort_pairs(nullptr, temp_bytes, p.keys_in, p.keys_out, p.rows_in, p.rows_out, static_cast<size_t>(n), 0u, 64u, ctx->stream));
        DevBufRef temp = pool_alloc(ctx, std::max<size_t>(temp_bytes, 16));
        RV_HIP(rocprim::radix_sort_pairs(temp->ptr, temp_bytes, p.keys_in, p.keys_out, p.rows_in, p.rows_out, static_cast<size_t>(n), 0u, 64u, ctx->stream));
        cur ^= 1;
        ++timer.launches;
        name = "rocprim::radix_sort_pairs";
    } else {
        for (uint32_t pos = 0; pos < static_cast<uint32_t>(rvk::kSortPositions); ++pos) {
            if (!((value_passes >> pos) & 1)) continue;
            const bool last = !null_pass && (value_passes >> (pos + 1)) == 0;
            bind();
            p.shift = 8 * pos;
            p.nbins = rvk::kSortDigits;
            launch_pass<false>(ctx, p, last, scan_total);
            cur ^= 1;
            ++scatters;
            name = "sort_scatter";
        }
    }
    if (null_pass) {
        bind();
        p.nbins = 2;
        launch_pass<true>(ctx, p, true, scan_total);
        ++scatters;
        if (name.empty()) name = "sort_scatter";
        else if (name != "sort_scatter") name += "+sort_scatter";
    } else if (scatters == 0) {  // nothing wrote the output yet
        hipLaunchKernelGGL(rvk::sort_widen, dim3(grid_for_words(ctx, n, rvk::kSortThreads)), dim3(rvk::kSortThreads), 0, ctx->stream,
                           static_cast<const uint32_t *>(rows[cur]->ptr), n, static_cast<int64_t *>(out->ptr));
        RV_HIP(hipGetLastError());
        ++timer.launches;
        name += name.empty() ? "sort_widen" : "+sort_widen";
    }
    timer.launches += scatters * 5;  // tile counts, the scan's three, the scatter
    timer.stop();
    RV_HIP(hipStreamSynchronize(ctx->stream));  // the working buffers go back to the pool
    timer.add();
    ctx->sort_last_passes = scatters;
    ctx->last_kernel = name;
    return out;
}

namespace {

// `prior` as rv_take_device takes its index list
const uint64_t *check_prior(rv_ctx *ctx, const rv_dcolumn *key, const rv_dcolumn *prior) {
    if (!prior) return nullptr;
    require(prior->dtype == RV_INT64, RV_ERR_TYPE_MISMATCH, "rv_sort_indices: prior must be an Int64 array");
    require(prior->length == key->length, RV_ERR_LENGTH_MISMATCH,
            fmt("rv_sort_indices: prior has %llu rows, the key %llu", static_cast<unsigned long long>(prior->length), static_cast<unsigned long long>(key->length)));
    uint64_t nulls = 0;
    const rv_status st = rv_null_count(ctx, prior, &nulls);
    if (st != RV_OK) throw Error(st, last_error());
    require(nulls == 0, RV_ERR_INVALID_ARG, "rv_sort_indices: prior must not contain nulls");
    return static_cast<const uint64_t *>(prior->values->ptr) + prior->offset;
}

}  // namespace

// (k0, k1, ...) is the chain from the last key to the first: each stable sort reorders what the keys after it left
DevBufRef sort_chain(rv_ctx *ctx, const rv_dcolumn *const *keys, const uint32_t *flags, uint32_t nkeys, DevBufRef prior) {
    for (uint32_t k = nkeys; k-- > 0;) prior = sort_indices(ctx, keys[k], flags[k], prior ? static_cast<const uint64_t *>(prior->ptr) : nullptr);
    return prior;
}

}  // namespace rvl

extern "C" {

rv_status rv_sort_indices(rv_ctx *ctx, const rv_dcolumn *key, uint32_t flags, const rv_dcolumn *prior, rv_dcolumn **out_indices) {
    return guarded([&] {
        require(ctx && key && out_indices, RV_ERR_INVALID_ARG, "rv_sort_indices: NULL argument");
        *out_indices = nullptr;
        check_sort_key(key, flags, "rv_sort_indices");
        set_device(ctx);
        const uint64_t *d_prior = check_prior(ctx, key, prior);
        breaker_call(ctx, out_indices, 1, [&] { *out_indices = index_column(sort_indices(ctx, key, flags, d_prior), key->length); });
    });
}

rv_status rv_sort(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const uint32_t *key_cols, const uint32_t *key_flags, uint32_t nkeys,
                  rv_dcolumn **out) {
    return guarded([&] {
        require(ctx && cols && out && (nkeys == 0 || (key_cols && key_flags)), RV_ERR_INVALID_ARG, "rv_sort: NULL argument");
        require(nkeys >= 1, RV_ERR_INVALID_ARG, "rv_sort: no sort keys");
        check_batch(cols, ncols);
        check_key_columns("rv_sort", "", key_cols, nkeys, ncols);
        for (uint32_t k = 0; k < nkeys; ++k) check_sort_key(cols[key_cols[k]], key_flags[k], "rv_sort");
        for (uint32_t c = 0; c < ncols; ++c) out[c] = nullptr;
        set_device(ctx);
        breaker_call(ctx, out, ncols, [&] {
            std::vector<const rv_dcolumn *> keys(nkeys);
            for (uint32_t k = 0; k < nkeys; ++k) keys[k] = cols[key_cols[k]];
            DevBufRef idx = sort_chain(ctx, keys.data(), key_flags, nkeys);
            const std::string name = ctx->last_kernel;
            const uint64_t passes = ctx->sort_last_passes;
            take_on_device(ctx, cols, ncols, static_cast<const uint64_t *>(idx->ptr), cols[0]->length, out, false);
            RV_HIP(hipStreamSynchronize(ctx->stream));  // the index list goes back to the pool
            ctx->last_kernel = name;
            ctx->sort_last_passes = passes;
        });
    });
}

}  // extern "C"
