// Hash join on the device (reference PhysicalPlan::HashJoin, plan.rs:174-284): build table, probe, gather; the inner join and the
// outer, semi and anti joins (rv_join_kind).
// One unit of the backend library behind include/rivulus_gpu.h (gfx950 only; compiled with hipcc).  Shared helpers and the
// functions the units call across each other are declared in launch.hpp (namespace rvl); the kernels are in join_kernel.hpp.
#include <rocprim/device/device_radix_sort.hpp>

#include "breaker_steps.hpp"
#include "join_kernel.hpp"

using namespace rvh;
using namespace rvl;

// A build side hashed on the device (join_kernel.hpp has the layout).  Probed by any number of key columns.
struct rv_join_table {
    rv_dtype key_dtype = RV_NULL;
    uint64_t n_build = 0;
    uint64_t n_keyed = 0;   // rows in key groups (non-null, non-NaN)
    uint64_t n_null = 0;    // null rows, behind them in `rows`
    uint64_t max_group = 0; // longest key group
    uint64_t nslots = 0;
    uint64_t hash_mask = ~0ull;
    DevBufRef slots, rows;
    std::shared_ptr<rvh::Pool> pool;  // keeps the blocks' pool alive with the table
};

namespace rvl {
namespace {

rvk::JoinTableView table_view(const rv_join_table *t, rv_dtype probe_dtype) {
    rvk::JoinTableView v{};
    v.slots = static_cast<unsigned long long *>(t->slots->ptr);
    v.rows = static_cast<const uint32_t *>(t->rows->ptr);
    v.slot_mask = t->nslots - 1;
    v.hash_mask = t->hash_mask;
    v.null_start = static_cast<uint32_t>(t->n_keyed);
    v.null_count = static_cast<uint32_t>(t->n_null);
    // AnyValue's PartialEq (series.rs:85-97): values of different variants never compare equal; only Null meets Null
    v.match_values = t->key_dtype == probe_dtype && t->key_dtype != RV_NULL;
    return v;
}

void check_key(const rv_dcolumn *key, const char *what) {
    require(key != nullptr, RV_ERR_INVALID_ARG, fmt("%s: NULL key column", what));
    require(key->dtype != RV_STRING, RV_ERR_UNSUPPORTED,
            fmt("%s: String join keys are not supported on the device (String payload columns are)", what));
    require(key->dtype == RV_NULL || key->dtype == RV_BOOLEAN || is_value_type(key->dtype), RV_ERR_UNSUPPORTED,
            fmt("%s: unsupported key dtype", what));
}

// a bitmap of n rows at offset 0 as the BooleanArray selection_prefix / selection_to_indices read
DevBufRef ascending_rows(rv_ctx *ctx, const DevBufRef &bitmap, uint64_t n, uint64_t count) {
    const rv_dcolumn sel = plain_view(RV_BOOLEAN, bitmap, n);
    DevBufRef excl = selection_prefix(ctx, &sel, count);
    return selection_to_indices(ctx, &sel, count, excl);
}

std::unique_ptr<rv_join_table> build_table(rv_ctx *ctx, const rv_dcolumn *key) {
    check_key(key, "rv_join_build");
    const uint64_t n = key->length;
    require(n < (uint64_t{1} << 32), RV_ERR_UNSUPPORTED, "rv_join_build: build sides of 2^32 rows or more are not supported (32-bit build row ids)");
    auto t = std::make_unique<rv_join_table>();
    t->key_dtype = key->dtype;
    t->n_build = n;
    t->pool = ctx->pool;
    if (ctx->opt_join_hash_bits > 0 && ctx->opt_join_hash_bits < 64) t->hash_mask = (uint64_t{1} << ctx->opt_join_hash_bits) - 1;
    const rvk::DevCol kv = dev_view(key);

    // 1. which rows go into key groups, which into the null group
    const uint64_t nwords = (n + 63) / 64;
    DevBufRef keep = pool_alloc(ctx, nwords * 8 + 16), nulls = pool_alloc(ctx, nwords * 8 + 16);
    if (n) {
        Ctrl *ctrl = prepare_ctrl(ctx, 0);
        const uint64_t waves = (nwords + rvk::kJoinClassWords - 1) / rvk::kJoinClassWords;
        hipLaunchKernelGGL(rvk::join_classify, dim3(static_cast<uint32_t>((waves + 3) / 4)), dim3(256), 0, ctx->stream, kv, n,
                           static_cast<uint64_t *>(keep->ptr), static_cast<uint64_t *>(nulls->ptr), &ctrl->pops[0]);
        RV_HIP(hipGetLastError());
        const Ctrl *h = fetch_ctrl(ctx);
        t->n_keyed = h->pops[0];
        t->n_null = h->pops[1];
    }
    uint64_t nslots = 16;
    while (nslots < 2 * t->n_keyed) nslots *= 2;
    t->nslots = nslots;
    t->slots = pool_alloc(ctx, nslots * 16);
    RV_HIP(hipMemsetAsync(t->slots->ptr, 0, nslots * 16, ctx->stream));
    t->rows = pool_alloc(ctx, std::max<size_t>((t->n_keyed + t->n_null) * 4, 16));
    uint32_t *rows = static_cast<uint32_t *>(t->rows->ptr);

    // 2. key groups: (key bits, row) of the kept rows in row order, a stable radix sort, then one slot per distinct key
    if (t->n_keyed) {
        const uint64_t m = t->n_keyed;
        DevBufRef idx = ascending_rows(ctx, keep, n, m);
        DevBufRef keys_in = pool_alloc(ctx, m * 8), keys_out = pool_alloc(ctx, m * 8), rows_in = pool_alloc(ctx, m * 4 + 16);
        const int grid = grid_for_words(ctx, m, 256);
        hipLaunchKernelGGL(rvk::join_gather_keys, dim3(grid), dim3(256), 0, ctx->stream, kv, static_cast<const uint64_t *>(idx->ptr), m,
                           static_cast<uint64_t *>(keys_in->ptr), static_cast<uint32_t *>(rows_in->ptr));
        RV_HIP(hipGetLastError());
        const unsigned end_bit = key->dtype == RV_BOOLEAN ? 1 : 64;
        size_t temp_bytes = 0;
        RV_HIP(rocprim::radix_sort_pairs(nullptr, temp_bytes, static_cast<const uint64_t *>(keys_in->ptr), static_cast<uint64_t *>(keys_out->ptr),
                                         static_cast<const uint32_t *>(rows_in->ptr), rows, static_cast<size_t>(m), 0u, end_bit, ctx->stream));
        DevBufRef temp = pool_alloc(ctx, std::max<size_t>(temp_bytes, 16));
        RV_HIP(rocprim::radix_sort_pairs(temp->ptr, temp_bytes, static_cast<const uint64_t *>(keys_in->ptr), static_cast<uint64_t *>(keys_out->ptr),
                                         static_cast<const uint32_t *>(rows_in->ptr), rows, static_cast<size_t>(m), 0u, end_bit, ctx->stream));
        rvk::JoinTableView v = table_view(t.get(), key->dtype);
        Ctrl *ctrl = prepare_ctrl(ctx, 0);
        hipLaunchKernelGGL(rvk::join_insert_heads, dim3(grid), dim3(256), 0, ctx->stream, v, static_cast<const uint64_t *>(keys_out->ptr), m);
        hipLaunchKernelGGL(rvk::join_insert_tails, dim3(grid), dim3(256), 0, ctx->stream, v, static_cast<const uint64_t *>(keys_out->ptr), m,
                           &ctrl->pops[2]);
        RV_HIP(hipGetLastError());
        t->max_group = fetch_ctrl(ctx)->pops[2];  // (also: the scratch blocks above go back to the pool after their last reader)
    }
    // 3. the null group, ascending, behind the key groups
    if (t->n_null) {
        DevBufRef idx = ascending_rows(ctx, nulls, n, t->n_null);
        hipLaunchKernelGGL(rvk::join_null_rows, dim3(grid_for_words(ctx, t->n_null, 256)), dim3(256), 0, ctx->stream,
                           static_cast<const uint64_t *>(idx->ptr), t->n_null, rows + t->n_keyed);
        RV_HIP(hipGetLastError());
    }
    RV_HIP(hipStreamSynchronize(ctx->stream));
    return t;
}

// JoinProbeParams of `key` against `t`, without the tile counts and the outputs; longest = the longest list a probe row of this key
// column can meet
rvk::JoinProbeParams probe_params(const rv_join_table *t, const rv_dcolumn *key, uint64_t &longest) {
    rvk::JoinProbeParams p{};
    p.table = table_view(t, key->dtype);
    p.key = dev_view(key);
    p.n = key->length;
    p.lane_most = rvt::kJoinLaneListMost;
    longest = std::max<uint64_t>(p.table.match_values ? t->max_group : 0, t->n_null);
    return p;
}

// pairs the device can hold: two 8-byte indices each
uint64_t device_pair_cap(const rv_ctx *ctx) { return static_cast<uint64_t>(ctx->props.totalGlobalMem) / 16; }

bool kind_has_pairs(rv_join_kind kind) { return kind != RV_JOIN_PROBE_SEMI && kind != RV_JOIN_PROBE_ANTI; }
const char *kind_name(rv_join_kind kind) {
    switch (kind) {
        case RV_JOIN_PROBE_OUTER: return "outer";
        case RV_JOIN_FULL_OUTER: return "full";
        case RV_JOIN_PROBE_SEMI: return "semi";
        case RV_JOIN_PROBE_ANTI: return "anti";
        default: return "inner";
    }
}
void check_kind(const char *what, int kind) {
    require(kind >= RV_JOIN_INNER && kind <= RV_JOIN_PROBE_ANTI, RV_ERR_INVALID_ARG, fmt("%s: unknown join kind %d", what, kind));
}
// f(std::integral_constant<int, KIND>) for the kernel kind of a join kind: the one place a run-time kind becomes a template argument
template <class F>
void with_kind(rv_join_kind kind, F f) {
    switch (kind) {
        case RV_JOIN_INNER: return f(std::integral_constant<int, rvk::JOIN_INNER>{});
        case RV_JOIN_PROBE_OUTER: return f(std::integral_constant<int, rvk::JOIN_OUTER>{});
        case RV_JOIN_FULL_OUTER: return f(std::integral_constant<int, rvk::JOIN_FULL>{});
        case RV_JOIN_PROBE_SEMI: return f(std::integral_constant<int, rvk::JOIN_SEMI>{});
        case RV_JOIN_PROBE_ANTI: return f(std::integral_constant<int, rvk::JOIN_ANTI>{});
        default: throw Error(RV_ERR_INTERNAL, "join: no kernel kind for this join kind");
    }
}
// the emit pass over the first p.n rows, into fresh index buffers: by lists of at most one row, of at most a lane's share, or longer, in
// the kind's instantiation (named with the kind appended, but for the inner join).  `pairs` are the rows the emit pass writes, `room` >=
// pairs the rows the buffers hold (the full outer join's tail goes behind); semi and anti joins get no build buffer.
void emit_pairs(rv_ctx *ctx, rvk::JoinProbeParams &p, uint64_t longest, uint64_t pairs, DevBufRef &out_probe, DevBufRef &out_build,
                rv_join_kind kind = RV_JOIN_INNER, uint64_t room = 0) {
    room = std::max(room, pairs);
    out_probe = pool_alloc(ctx, std::max<size_t>(room * 8, 16));
    if (kind_has_pairs(kind)) out_build = pool_alloc(ctx, std::max<size_t>(room * 8, 16));
    if (!pairs) return;
    p.out_probe = static_cast<int64_t *>(out_probe->ptr);
    p.out_build = out_build ? static_cast<int64_t *>(out_build->ptr) : nullptr;
    const dim3 grid(static_cast<uint32_t>((p.n + rvk::kJoinTileRows - 1) / rvk::kJoinTileRows)), block(rvk::kJoinThreads);
    const int mode = !kind_has_pairs(kind) || longest <= 1 ? 0 : longest <= rvt::kJoinLaneListMost ? 1 : 2;
    with_kind(kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        if constexpr (K == rvk::JOIN_SEMI || K == rvk::JOIN_ANTI) {
            hipLaunchKernelGGL((rvk::join_probe_emit<0, K>), grid, block, 0, ctx->stream, p);
        } else {
            if (mode == 0) hipLaunchKernelGGL((rvk::join_probe_emit<0, K>), grid, block, 0, ctx->stream, p);
            else if (mode == 1) hipLaunchKernelGGL((rvk::join_probe_emit<1, K>), grid, block, 0, ctx->stream, p);
            else hipLaunchKernelGGL((rvk::join_probe_emit<2, K>), grid, block, 0, ctx->stream, p);
        }
    });
    RV_HIP(hipGetLastError());
    ctx->last_kernel = kind == RV_JOIN_INNER ? fmt("join_probe_emit<%d>", mode) : fmt("join_probe_emit<%d,%s>", mode, kind_name(kind));
}

// result_pairs of plan.rs:196-204 as two Int64 index buffers, for every kind (rv_join_probe: RV_JOIN_INNER; rv_join_probe_kind): the count
// pass with the kind's row rule, the scan of the tile counts, one read-back of the total, the size check, then the emit pass.  A cell
// without a partner is kJoinNone in the buffers.
//   RV_JOIN_INNER: a probe without rows, or against a table without a single list, has nothing to count: no count pass, no read-back.
//   The other kinds count every probe row -- against such a table every one of them is unmatched -- and always read the block back.
//   RV_JOIN_FULL_OUTER: the count pass marks the groups it meets; the build rows of the unmarked groups and of no group are counted before
//   the size check and written behind the probe rows, ascending.  That check comes before any OUTPUT is allocated; the marks and the two
//   build-row bitmaps -- a bit per slot and two bits per build row -- are scratch of the count pass and are there before it.
// The inner join reports under rv_join_probe's name whichever entry point it came through.
uint64_t probe_table(rv_ctx *ctx, const rv_join_table *t, const rv_dcolumn *key, rv_join_kind kind, DevBufRef &out_probe, DevBufRef &out_build) {
    const bool inner = kind == RV_JOIN_INNER, full = kind == RV_JOIN_FULL_OUTER;
    check_key(key, inner ? "rv_join_probe" : "rv_join_probe_kind");
    uint64_t longest = 0;
    rvk::JoinProbeParams p = probe_params(t, key, longest);
    const uint64_t ntiles = (p.n + rvk::kJoinTileRows - 1) / rvk::kJoinTileRows;
    const bool counted = p.n && (longest || !inner), fetched = counted || !inner;
    uint64_t total = 0, tail = 0;
    DevBufRef tiles, marks, matched, unmatched, tail_rows;
    Ctrl *ctrl = fetched ? prepare_ctrl(ctx, 0) : nullptr;
    if (full) {
        const size_t mark_bytes = ((t->nslots + 1 + 31) / 32) * 4, row_bytes = ((t->n_build + 63) / 64) * 8;
        marks = pool_alloc(ctx, mark_bytes + 16);
        matched = pool_alloc(ctx, row_bytes + 16);
        unmatched = pool_alloc(ctx, row_bytes + 16);
        RV_HIP(hipMemsetAsync(marks->ptr, 0, mark_bytes, ctx->stream));
        RV_HIP(hipMemsetAsync(matched->ptr, 0, row_bytes + 16, ctx->stream));
    }
    if (counted) {
        tiles = pool_alloc(ctx, ntiles * 8 + 16);
        p.tile_counts = static_cast<uint64_t *>(tiles->ptr);
        const dim3 grid(static_cast<uint32_t>(ntiles)), block(rvk::kJoinThreads);
        uint32_t *m = full ? static_cast<uint32_t *>(marks->ptr) : nullptr;
        with_kind(kind, [&](auto k) { hipLaunchKernelGGL(rvk::join_probe_count<decltype(k)::value>, grid, block, 0, ctx->stream, p, m); });
        hipLaunchKernelGGL(rvk::scan_sums_inplace, dim3(1), dim3(1024), 0, ctx->stream, p.tile_counts, ntiles, &ctrl->pops[0]);
        RV_HIP(hipGetLastError());
    }
    if (full && t->n_build) {
        const rvk::JoinTableView v = table_view(t, key->dtype);
        if (p.n)
            hipLaunchKernelGGL(rvk::join_mark_rows, dim3(static_cast<uint32_t>((t->nslots + 1 + 255) / 256)), dim3(256), 0, ctx->stream, v,
                               static_cast<const uint32_t *>(marks->ptr), static_cast<unsigned long long *>(matched->ptr));
        hipLaunchKernelGGL(rvk::join_unmatched_words, dim3(grid_for_words(ctx, (t->n_build + 63) / 64, 256)), dim3(256), 0, ctx->stream,
                           static_cast<const unsigned long long *>(matched->ptr), t->n_build, static_cast<uint64_t *>(unmatched->ptr), &ctrl->pops[1]);
        RV_HIP(hipGetLastError());
    }
    if (fetched) {
        ctx->last_kernel = "join_probe_count";
        const Ctrl *h = fetch_ctrl(ctx);
        total = counted ? h->pops[0] : 0;
        tail = h->pops[1];
    }
    // refuse what the device cannot hold before anything is allocated (n_probe x n_build pairs can exceed 2^64 bytes)
    require(total <= device_pair_cap(ctx) && tail <= device_pair_cap(ctx) - total, RV_ERR_OOM,
            fmt(inner ? "rv_join_probe: %llu pairs need %llu x 16 bytes of output, more than the device's %llu bytes"
                      : "rv_join_probe_kind: %llu rows need %llu x 16 bytes of output, more than the device's %llu bytes",
                static_cast<unsigned long long>(total + tail), static_cast<unsigned long long>(total + tail),
                static_cast<unsigned long long>(ctx->props.totalGlobalMem)));
    if (tail) {
        tail_rows = ascending_rows(ctx, unmatched, t->n_build, tail);  // before the outputs: its scratch is freed first
        ctx->last_kernel = "join_probe_count";
    }
    emit_pairs(ctx, p, longest, total, out_probe, out_build, kind, total + tail);
    if (tail) {
        hipLaunchKernelGGL(rvk::join_unmatched_tail, dim3(grid_for_words(ctx, tail, 256)), dim3(256), 0, ctx->stream, static_cast<const uint64_t *>(tail_rows->ptr),
                           tail, static_cast<int64_t *>(out_probe->ptr) + total, static_cast<int64_t *>(out_build->ptr) + total);
        RV_HIP(hipGetLastError());
    }
    RV_HIP(hipStreamSynchronize(ctx->stream));  // the scratch goes back to the pool
    return total + tail;
}

// An index buffer of the probe as a public Int64 column: kJoinNone cells become null cells (value 0, validity attached only when
// there is one, null_count known).
rv_dcolumn *nullable_index_column(rv_ctx *ctx, const DevBufRef &buf, uint64_t rows) {
    std::unique_ptr<rv_dcolumn> o(index_column(buf, rows));
    if (!rows) return o.release();
    DevBufRef validity = pool_alloc(ctx, std::max<size_t>(bitmap_words_bytes(rows), 16));
    Ctrl *ctrl = prepare_ctrl(ctx, 0);
    hipLaunchKernelGGL(rvk::join_index_nulls, dim3(grid_for_words(ctx, rows, 256)), dim3(256), 0, ctx->stream, static_cast<int64_t *>(buf->ptr), rows,
                       static_cast<uint64_t *>(validity->ptr), &ctrl->pops[0]);
    RV_HIP(hipGetLastError());
    o->null_count = static_cast<int64_t>(rows - fetch_ctrl(ctx)->pops[0]);
    if (o->null_count) o->validity = validity;
    return o.release();
}

static_assert(rvt::kJoinFastBatchRows * 4 == static_cast<uint64_t>(rvk::kJoinTileRows), "the fast count pass takes four batches per tile");

// The probe of a window cut into batches of chunk_rows rows (rv_hash_join_chunked): ONE count pass that also counts every batch,
// the tile scan, ONE read-back of the total and the K batch counts (into batch_rows[K]), the size check, then the emit pass over
// the longest prefix of batches whose pairs fit `max_pairs` (0: no cap of the caller's) and the device -- at least one batch.
// Returns the pairs of the prefix; *taken = its batches.
// `kind`: RV_JOIN_INNER or a probe-preserving kind; the batch counts then follow the kind's row rule.  `what` names the entry point.
uint64_t probe_table_batched(rv_ctx *ctx, const char *what, rv_join_kind kind, const rv_join_table *t, const rv_dcolumn *key, uint64_t chunk_rows,
                             uint64_t max_pairs, uint64_t *batch_rows, uint64_t &taken, DevBufRef &out_probe, DevBufRef &out_build) {
    check_key(key, what);
    const uint64_t n = key->length;
    const uint64_t nb = (n + chunk_rows - 1) / chunk_rows;
    uint64_t longest = 0;
    rvk::JoinProbeParams p = probe_params(t, key, longest);
    uint64_t total = 0;
    DevBufRef tiles;
    ctx->last_kernel = "join_probe_count_batched";
    if (n) {
        const uint64_t ntiles = (n + rvk::kJoinTileRows - 1) / rvk::kJoinTileRows;
        tiles = pool_alloc(ctx, ntiles * 8 + 16);
        DevBufRef counts = pool_alloc(ctx, nb * 8 + 16);
        p.tile_counts = static_cast<uint64_t *>(tiles->ptr);
        rvk::JoinBatchParams b{chunk_rows, nb, static_cast<unsigned long long *>(counts->ptr)};
        const bool fast = chunk_rows == rvt::kJoinFastBatchRows;
        if (!fast) RV_HIP(hipMemsetAsync(counts->ptr, 0, nb * 8, ctx->stream));
        Ctrl *ctrl = prepare_ctrl(ctx, 0);
        const dim3 grid(static_cast<uint32_t>(ntiles)), block(rvk::kJoinThreads);
        with_kind(kind, [&](auto k) {
            constexpr int K = decltype(k)::value;
            if constexpr (K != rvk::JOIN_FULL) {  // a full outer join has no batched form: refused by the entry point
                if (fast) hipLaunchKernelGGL((rvk::join_probe_count_batched<true, K>), grid, block, 0, ctx->stream, p, b);
                else hipLaunchKernelGGL((rvk::join_probe_count_batched<false, K>), grid, block, 0, ctx->stream, p, b);
            }
        });
        hipLaunchKernelGGL(rvk::scan_sums_inplace, dim3(1), dim3(1024), 0, ctx->stream, p.tile_counts, ntiles, &ctrl->pops[0]);
        RV_HIP(hipGetLastError());
        void *hs = ctx->stage(nb * 8);
        RV_HIP(hipMemcpyAsync(hs, counts->ptr, nb * 8, hipMemcpyDeviceToHost, ctx->stream));
        total = fetch_ctrl(ctx)->pops[0];  // the one wait: the total and the batch counts together
        std::memcpy(batch_rows, hs, nb * 8);
        uint64_t sum = 0;
        for (uint64_t k = 0; k < nb; ++k) sum += batch_rows[k];
        require(sum == total, RV_ERR_INTERNAL, fmt("%s: per-batch pair counts do not add up", what));
    }
    // the longest prefix that fits; one batch the device cannot hold on its own is RV_ERR_OOM before anything is allocated
    const uint64_t device_most = device_pair_cap(ctx);
    const uint64_t cap = max_pairs ? std::min(max_pairs, device_most) : device_most;
    require(nb == 0 || batch_rows[0] <= device_most, RV_ERR_OOM,
            fmt("%s: batch 0 has %llu pairs, more than the device's %llu bytes hold at 16 bytes each", what,
                static_cast<unsigned long long>(nb ? batch_rows[0] : 0), static_cast<unsigned long long>(ctx->props.totalGlobalMem)));
    uint64_t pairs = 0;
    taken = 0;
    while (taken < nb && (taken == 0 || (pairs <= cap && batch_rows[taken] <= cap - pairs))) pairs += batch_rows[taken++];
    p.n = std::min(n, taken * chunk_rows);  // the prefix's rows: its tiles' prefixes are those of the whole window
    emit_pairs(ctx, p, longest, pairs, out_probe, out_build, kind);
    // no wait here: `tiles` goes back to the pool, and its next user runs behind the emit pass on the stream
    return pairs;
}

// the checks of rv_hash_join, shared by the chunked form
void check_join_sides(const char *what, const rv_dcolumn *const *build_cols, uint32_t n_build, uint32_t build_key, const rv_dcolumn *const *probe_cols,
                      uint32_t n_probe, uint32_t probe_key) {
    require(build_key < n_build, RV_ERR_INVALID_ARG, fmt("%s: build key %u out of range for %u build columns", what, build_key, n_build));
    require(probe_key < n_probe, RV_ERR_INVALID_ARG, fmt("%s: probe key %u out of range for %u probe columns", what, probe_key, n_probe));
    check_batch(build_cols, n_build);
    check_batch(probe_cols, n_probe);
    for (const auto &[cols, n] : {std::pair{build_cols, n_build}, std::pair{probe_cols, n_probe}})
        for (uint32_t c = 0; c < n; ++c) {
            const rv_dtype d = cols[c]->dtype;
            require(is_value_type(d) || d == RV_BOOLEAN || d == RV_STRING || d == RV_NULL, RV_ERR_UNSUPPORTED, fmt("%s: unsupported dtype", what));
        }
    check_key(build_cols[build_key], what);
    check_key(probe_cols[probe_key], what);
}

// materialize_join_result (plan.rs:212-255): every probe column by probe_idx, then every build column but the key by build_idx.
// The indices come from the tables themselves: no bounds pre-pass.  The outputs are freed on an error.
// Other kinds (rv_hash_join_kind): the side that can lack a partner goes through the nullable gather, kJoinNone being the null index;
// RV_JOIN_FULL_OUTER keeps the build key at its place; semi and anti joins gather the probe columns only.
uint32_t join_output_columns(rv_join_kind kind, uint32_t n_probe, uint32_t n_build) {
    return !kind_has_pairs(kind) ? n_probe : kind == RV_JOIN_FULL_OUTER ? n_probe + n_build : n_probe + n_build - 1;
}
void gather_pairs(rv_ctx *ctx, const rv_dcolumn *const *build_cols, uint32_t n_build, uint32_t build_key, const rv_dcolumn *const *probe_cols,
                  uint32_t n_probe, const DevBufRef &pi, const DevBufRef &bi, uint64_t rows, rv_dcolumn **out, rv_join_kind kind = RV_JOIN_INNER) {
    const uint32_t nout = join_output_columns(kind, n_probe, n_build);
    std::vector<const rv_dcolumn *> build_rest;
    for (uint32_t c = 0; c < n_build; ++c)
        if (c != build_key || kind == RV_JOIN_FULL_OUTER) build_rest.push_back(build_cols[c]);
    const IndexNulls none{};  // kJoinNone is the null index
    const uint64_t *p_idx = static_cast<const uint64_t *>(pi->ptr), *b_idx = bi ? static_cast<const uint64_t *>(bi->ptr) : nullptr;
    const uint32_t n_rest = static_cast<uint32_t>(build_rest.size());
    breaker_call(ctx, out, nout, [&] {
        if (kind == RV_JOIN_FULL_OUTER) take_nullable_on_device(ctx, probe_cols, n_probe, p_idx, rows, out, false, none);
        else take_on_device(ctx, probe_cols, n_probe, p_idx, rows, out, false);
        if (kind == RV_JOIN_FULL_OUTER || kind == RV_JOIN_PROBE_OUTER) take_nullable_on_device(ctx, build_rest.data(), n_rest, b_idx, rows, out + n_probe, false, none);
        else if (kind_has_pairs(kind)) take_on_device(ctx, build_rest.data(), n_rest, b_idx, rows, out + n_probe, false);
        RV_HIP(hipStreamSynchronize(ctx->stream));  // the index buffers go back to the pool
    });
}

}  // namespace
}  // namespace rvl

extern "C" {

rv_status rv_join_build(rv_ctx *ctx, const rv_dcolumn *build_key, rv_join_table **out) {
    return guarded([&] {
        require(ctx && build_key && out, RV_ERR_INVALID_ARG, "rv_join_build: NULL argument");
        *out = nullptr;
        set_device(ctx);
        *out = build_table(ctx, build_key).release();
    });
}

rv_status rv_join_probe(rv_ctx *ctx, const rv_join_table *table, const rv_dcolumn *probe_key, rv_dcolumn **out_probe_idx,
                        rv_dcolumn **out_build_idx, uint64_t *out_rows) {
    return guarded([&] {
        require(ctx && table && probe_key && out_probe_idx && out_build_idx, RV_ERR_INVALID_ARG, "rv_join_probe: NULL argument");
        *out_probe_idx = *out_build_idx = nullptr;
        set_device(ctx);
        DevBufRef pi, bi;
        const uint64_t rows = probe_table(ctx, table, probe_key, RV_JOIN_INNER, pi, bi);
        std::unique_ptr<rv_dcolumn> a(index_column(pi, rows)), b(index_column(bi, rows));
        *out_probe_idx = a.release();
        *out_build_idx = b.release();
        if (out_rows) *out_rows = rows;
    });
}

rv_status rv_join_probe_kind(rv_ctx *ctx, const rv_join_table *table, const rv_dcolumn *probe_key, int kind_arg, rv_dcolumn **out_probe_idx,
                             rv_dcolumn **out_build_idx, uint64_t *out_rows) {
    return guarded([&] {
        require(ctx && table && probe_key && out_probe_idx && out_build_idx, RV_ERR_INVALID_ARG, "rv_join_probe_kind: NULL argument");
        check_kind("rv_join_probe_kind", kind_arg);
        const rv_join_kind kind = static_cast<rv_join_kind>(kind_arg);
        *out_probe_idx = *out_build_idx = nullptr;
        set_device(ctx);
        DevBufRef pi, bi;
        const uint64_t rows = probe_table(ctx, table, probe_key, kind, pi, bi);
        std::unique_ptr<rv_dcolumn> a, b;
        a.reset(kind == RV_JOIN_FULL_OUTER ? nullable_index_column(ctx, pi, rows) : index_column(pi, rows));
        if (kind == RV_JOIN_FULL_OUTER || kind == RV_JOIN_PROBE_OUTER) b.reset(nullable_index_column(ctx, bi, rows));
        else if (kind == RV_JOIN_INNER) b.reset(index_column(bi, rows));
        RV_HIP(hipStreamSynchronize(ctx->stream));
        *out_probe_idx = a.release();
        *out_build_idx = b.release();
        if (out_rows) *out_rows = rows;
    });
}

rv_status rv_join_table_free(rv_ctx *ctx, rv_join_table *table) {
    return guarded([&] {
        require(ctx, RV_ERR_INVALID_ARG, "rv_join_table_free: NULL context");
        if (table) {
            RV_HIP(hipStreamSynchronize(ctx->stream));
            delete table;
        }
    });
}

rv_status rv_join_table_info(const rv_join_table *table, uint64_t *build_rows, uint64_t *slots, uint64_t *longest_list) {
    return guarded([&] {
        require(table, RV_ERR_INVALID_ARG, "rv_join_table_info: NULL table");
        if (build_rows) *build_rows = table->n_build;
        if (slots) *slots = table->nslots;
        if (longest_list) *longest_list = std::max(table->max_group, table->n_null);
    });
}

rv_status rv_hash_join(rv_ctx *ctx, const rv_dcolumn *const *build_cols, uint32_t n_build, uint32_t build_key,
                       const rv_dcolumn *const *probe_cols, uint32_t n_probe, uint32_t probe_key, rv_dcolumn **out, uint64_t *out_rows) {
    return guarded([&] {
        require(ctx && build_cols && probe_cols && out, RV_ERR_INVALID_ARG, "rv_hash_join: NULL argument");
        check_join_sides("rv_hash_join", build_cols, n_build, build_key, probe_cols, n_probe, probe_key);
        set_device(ctx);
        const uint32_t nout = n_probe + n_build - 1;
        for (uint32_t c = 0; c < nout; ++c) out[c] = nullptr;
        std::unique_ptr<rv_join_table> t = build_table(ctx, build_cols[build_key]);
        DevBufRef pi, bi;
        const uint64_t rows = probe_table(ctx, t.get(), probe_cols[probe_key], RV_JOIN_INNER, pi, bi);
        gather_pairs(ctx, build_cols, n_build, build_key, probe_cols, n_probe, pi, bi, rows, out);
        if (out_rows) *out_rows = rows;
    });
}

rv_status rv_hash_join_kind(rv_ctx *ctx, const rv_dcolumn *const *build_cols, uint32_t n_build, uint32_t build_key, const rv_dcolumn *const *probe_cols,
                            uint32_t n_probe, uint32_t probe_key, int kind_arg, rv_dcolumn **out, uint64_t *out_rows) {
    return guarded([&] {
        require(ctx && build_cols && probe_cols && out, RV_ERR_INVALID_ARG, "rv_hash_join_kind: NULL argument");
        check_kind("rv_hash_join_kind", kind_arg);
        const rv_join_kind kind = static_cast<rv_join_kind>(kind_arg);
        check_join_sides("rv_hash_join_kind", build_cols, n_build, build_key, probe_cols, n_probe, probe_key);
        set_device(ctx);
        const uint32_t nout = join_output_columns(kind, n_probe, n_build);
        for (uint32_t c = 0; c < nout; ++c) out[c] = nullptr;
        std::unique_ptr<rv_join_table> t = build_table(ctx, build_cols[build_key]);
        DevBufRef pi, bi;
        const uint64_t rows = probe_table(ctx, t.get(), probe_cols[probe_key], kind, pi, bi);
        gather_pairs(ctx, build_cols, n_build, build_key, probe_cols, n_probe, pi, bi, rows, out, kind);
        if (out_rows) *out_rows = rows;
    });
}

// rv_hash_join_chunked and rv_hash_join_chunked_kind, `what` the entry point's name
static void hash_join_chunked(rv_ctx *ctx, const char *what, rv_join_kind kind, const rv_join_table *table, const rv_dcolumn *const *build_cols, uint32_t n_build,
                       uint32_t build_key, const rv_dcolumn *const *probe_cols, uint32_t n_probe, uint32_t probe_key, uint64_t chunk_rows, uint64_t max_pairs,
                       rv_dcolumn **out, uint64_t *out_rows, uint64_t nchunks, int64_t *out_nulls, uint64_t *out_total, uint64_t *out_batches) {
    {
        require(ctx && table && build_cols && probe_cols && out && out_batches, RV_ERR_INVALID_ARG, fmt("%s: NULL argument", what));
        require(chunk_rows >= 1, RV_ERR_INVALID_ARG, fmt("%s: chunk_rows is 0", what));
        check_join_sides(what, build_cols, n_build, build_key, probe_cols, n_probe, probe_key);
        require(build_cols[build_key]->length == table->n_build, RV_ERR_LENGTH_MISMATCH,
                fmt("%s: build columns of %llu rows, the table was built from %llu", what, static_cast<unsigned long long>(build_cols[build_key]->length),
                    static_cast<unsigned long long>(table->n_build)));
        const uint64_t n = probe_cols[0]->length;
        // dataframe_to_batches: ceil(n / chunk_rows) batches, none for an empty frame (streaming.rs:135-233)
        const uint64_t nb = (n + chunk_rows - 1) / chunk_rows;
        require(nb <= nchunks && (out_rows || nb == 0), RV_ERR_INVALID_ARG,
                fmt("%s: %llu batches, room for %llu", what, static_cast<unsigned long long>(nb), static_cast<unsigned long long>(nchunks)));
        set_device(ctx);
        const uint32_t nout = join_output_columns(kind, n_probe, n_build);
        for (uint32_t c = 0; c < nout; ++c) out[c] = nullptr;
        *out_batches = 0;
        std::vector<uint64_t> counts(nb);
        uint64_t taken = 0;
        DevBufRef pi, bi;
        const uint64_t rows = probe_table_batched(ctx, what, kind, table, probe_cols[probe_key], chunk_rows, max_pairs, counts.data(), taken, pi, bi);
        gather_pairs(ctx, build_cols, n_build, build_key, probe_cols, n_probe, pi, bi, rows, out, kind);
        breaker_call(ctx, out, nout, [&] {
            if (out_nulls) batch_null_counts(ctx, what, out, nout, counts.data(), taken, out_nulls);
        });
        if (nb) std::memcpy(out_rows, counts.data(), nb * 8);
        if (out_total) *out_total = rows;
        *out_batches = taken;
    }
}

rv_status rv_hash_join_chunked(rv_ctx *ctx, const rv_join_table *table, const rv_dcolumn *const *build_cols, uint32_t n_build, uint32_t build_key,
                               const rv_dcolumn *const *probe_cols, uint32_t n_probe, uint32_t probe_key, uint64_t chunk_rows, uint64_t max_pairs,
                               rv_dcolumn **out, uint64_t *out_rows, uint64_t nchunks, int64_t *out_nulls, uint64_t *out_total, uint64_t *out_batches) {
    return guarded([&] {
        hash_join_chunked(ctx, "rv_hash_join_chunked", RV_JOIN_INNER, table, build_cols, n_build, build_key, probe_cols, n_probe, probe_key, chunk_rows, max_pairs,
                          out, out_rows, nchunks, out_nulls, out_total, out_batches);
    });
}

rv_status rv_hash_join_chunked_kind(rv_ctx *ctx, const rv_join_table *table, const rv_dcolumn *const *build_cols, uint32_t n_build, uint32_t build_key,
                                    const rv_dcolumn *const *probe_cols, uint32_t n_probe, uint32_t probe_key, int kind_arg, uint64_t chunk_rows,
                                    uint64_t max_pairs, rv_dcolumn **out, uint64_t *out_rows, uint64_t nchunks, int64_t *out_nulls, uint64_t *out_total,
                                    uint64_t *out_batches) {
    return guarded([&] {
        check_kind("rv_hash_join_chunked_kind", kind_arg);
        const rv_join_kind kind = static_cast<rv_join_kind>(kind_arg);
        require(kind != RV_JOIN_FULL_OUTER, RV_ERR_UNSUPPORTED,
                "rv_hash_join_chunked_kind: RV_JOIN_FULL_OUTER has no batched form (its unmatched build rows belong to no probe batch); use rv_hash_join_kind");
        hash_join_chunked(ctx, "rv_hash_join_chunked_kind", kind, table, build_cols, n_build, build_key, probe_cols, n_probe, probe_key, chunk_rows, max_pairs,
                          out, out_rows, nchunks, out_nulls, out_total, out_batches);
    });
}

}  // extern "C"
