// Grouped aggregation on the device: group_by(key).agg(count / sum / min / max) -- rv_group_ids and rv_hash_aggregate over one key
// column, rv_group_ids_keys and rv_hash_aggregate_keys over a tuple of them.
// One unit of the backend library behind include/rivulus_gpu.h (gfx950 only; compiled with hipcc).  Shared helpers are declared in
// launch.hpp (namespace rvl), the steps every breaker's unit takes in breaker_steps.hpp; the kernels and the layout of the group table
// are in group_agg_kernel.hpp, the passes over tuples in group_keys_kernel.hpp.
#include <rocprim/device/device_radix_sort.hpp>

#include "group_agg_kernel.hpp"
#include "group_keys_kernel.hpp"
#include "breaker_steps.hpp"

using namespace rvh;
using namespace rvl;

namespace rvl {
namespace {

// the dense group ids of a key column: what both entry points start from
struct GroupIds {
    uint64_t groups = 0;
    DevBufRef gids;       // [n] uint32, or int64 when asked for the ABI's column
    DevBufRef first_row;  // [groups] uint64, ascending
};

void check_group_key(const rv_dcolumn *key, const char *what) {
    require(key->dtype == RV_INT64 || key->dtype == RV_NULL, RV_ERR_UNSUPPORTED,
            fmt("%s: only Int64 (and Null) key columns are supported on the device; String keys go through rv_string_dict_build ids", what));
    require(key->length < (uint64_t{1} << 32), RV_ERR_UNSUPPORTED, fmt("%s: keys of 2^32 rows or more are not supported (32-bit row ids, as the join)", what));
}

dim3 row_grid(uint64_t n) { return dim3(static_cast<uint32_t>((n + rvk::kGroupAggThreads - 1) / rvk::kGroupAggThreads)); }

// the key columns of one call.  tuple = false: ONE Int64 (or Null) column through the single-key passes of group_agg_kernel.hpp, all its
// null keys one group; tuple = true: the passes of group_keys_kernel.hpp over nkeys columns
struct KeyCols {
    const rv_dcolumn *const *cols;
    uint32_t nkeys;
    bool tuple;
    uint64_t rows() const { return cols[0]->length; }
};

// the three passes over tuples, one instantiation per number of key columns
template <int NK>
void launch_insert_keys(rv_ctx *ctx, uint64_t n, const rvk::GroupKeysInsertParams &q) {
    hipLaunchKernelGGL(rvk::group_insert_keys<NK>, row_grid(n), dim3(rvk::kGroupAggThreads), 0, ctx->stream, q);
}
template <int NK>
void launch_ids_keys(rv_ctx *ctx, const rvk::GroupKeysView &t, const uint64_t *marks, const uint64_t *excl, void *gids, bool wide, uint32_t *error) {
    if (wide)
        hipLaunchKernelGGL((rvk::group_ids_keys<NK, int64_t>), row_grid(t.n), dim3(rvk::kGroupAggThreads), 0, ctx->stream, t, marks, excl, static_cast<int64_t *>(gids), error);
    else
        hipLaunchKernelGGL((rvk::group_ids_keys<NK, uint32_t>), row_grid(t.n), dim3(rvk::kGroupAggThreads), 0, ctx->stream, t, marks, excl, static_cast<uint32_t *>(gids), error);
}
#define RV_KEYS_DISPATCH(nkeys, fn, ...)                                        \
    switch (nkeys) {                                                            \
        case 1: fn<1>(__VA_ARGS__); break;                                      \
        case 2: fn<2>(__VA_ARGS__); break;                                      \
        case 3: fn<3>(__VA_ARGS__); break;                                      \
        case 4: fn<4>(__VA_ARGS__); break;                                      \
        case 5: fn<5>(__VA_ARGS__); break;                                      \
        case 6: fn<6>(__VA_ARGS__); break;                                      \
        case 7: fn<7>(__VA_ARGS__); break;                                      \
        case 8: fn<8>(__VA_ARGS__); break;                                      \
        default: require(false, RV_ERR_INTERNAL, "group keys: no kernel for this many key columns"); \
    }
static_assert(rvk::kGroupKeysMost == 8, "RV_KEYS_DISPATCH lists the instantiations");

// insert, rank, ids.  One read-back here: the group count after the insert (everything behind it is sized by it).  The id pass is
// left QUEUED with a freshly prepared control block whose `err` is its flag: the caller reads it with its own last read-back.
GroupIds group_ids_of(rv_ctx *ctx, const KeyCols &keys, const char *what, bool wide) {
    GroupIds r;
    const uint64_t n = keys.rows();
    r.gids = pool_alloc(ctx, std::max<size_t>(n * (wide ? 8 : 4), 16));
    if (n == 0) {
        r.first_row = pool_alloc(ctx, 16);
        (void)prepare_ctrl(ctx, 0);
        return r;
    }
    const uint64_t max_groups = ctx->opt_agg_max_groups > 0 ? static_cast<uint64_t>(ctx->opt_agg_max_groups) : rvt::kGroupAggGroupsMostDefault;
    bool keyed = false;  // a column with a word in it: without one there is one group and a table of 16 slots will do
    for (uint32_t k = 0; k < keys.nkeys; ++k) keyed = keyed || keys.cols[k]->dtype != RV_NULL;
    uint64_t nslots = 16;
    if (keyed)
        while (nslots < 2 * std::min(n, max_groups)) nslots *= 2;
    DevBufRef slots = pool_alloc(ctx, nslots * 8), null_first = pool_alloc(ctx, 16);
    RV_HIP(hipMemsetAsync(slots->ptr, 0, nslots * 8, ctx->stream));
    RV_HIP(hipMemsetAsync(null_first->ptr, 0xFF, 16, ctx->stream));
    // the single-key view; over tuples what the passes behind the ids read of it: the slots, and a null word that stays ~0 (no null group)
    rvk::GroupTableView t{};
    t.slots = static_cast<unsigned long long *>(slots->ptr);
    t.null_first = static_cast<unsigned long long *>(null_first->ptr);
    t.slot_mask = nslots - 1;
    t.hash_mask = ctx->opt_agg_hash_bits > 0 && ctx->opt_agg_hash_bits < 64 ? (uint64_t{1} << ctx->opt_agg_hash_bits) - 1 : ~0ull;
    t.n = n;
    rvk::GroupKeysView tk{};
    if (keys.tuple) {
        tk.slots = t.slots;
        tk.slot_mask = t.slot_mask;
        tk.hash_mask = t.hash_mask;
        tk.n = n;
        tk.nkeys = keys.nkeys;
        for (uint32_t k = 0; k < keys.nkeys; ++k) tk.key[k] = dev_view(keys.cols[k]);
    }
    else t.key = dev_view(keys.cols[0]);

    // 1. insert: every distinct key's slot ends up holding the key's first row
    Ctrl *ctrl = prepare_ctrl(ctx, 0);
    unsigned long long *distinct = striped(ctx, &ctrl->pops[0]);
    unsigned long long *claimed = n > max_groups ? &ctrl->pops[1] : nullptr;
    if (keys.tuple) {
        rvk::GroupKeysInsertParams q{};
        q.t = tk;
        q.distinct = distinct;
        q.claimed = claimed;
        q.max_groups = max_groups;
        q.error = &ctrl->err;
        RV_KEYS_DISPATCH(keys.nkeys, launch_insert_keys, ctx, n, q)
    }
    else {
        rvk::GroupInsertParams q{};
        q.t = t;
        q.distinct = distinct;
        q.claimed = claimed;
        q.max_groups = max_groups;
        q.error = &ctrl->err;
        hipLaunchKernelGGL(rvk::group_insert, row_grid(n), dim3(rvk::kGroupAggThreads), 0, ctx->stream, q);
    }
    RV_HIP(hipGetLastError());
    RV_HIP(hipMemcpyAsync(&ctrl->pops[2], null_first->ptr, 8, hipMemcpyDeviceToDevice, ctx->stream));
    const Ctrl *h = fetch_ctrl(ctx);
    const uint64_t found = h->pops[0] + (h->pops[2] != ~0ull ? 1 : 0);
    require(!(h->err & 2u) && found <= max_groups, RV_ERR_UNSUPPORTED,
            fmt("%s: at least %llu distinct keys, more than option agg_max_groups = %llu allows", what, static_cast<unsigned long long>(found),
                static_cast<unsigned long long>(max_groups)));
    require(h->err == 0, RV_ERR_INTERNAL, fmt("%s: a chain walk exhausted the group table", what));
    r.groups = found;

    // 2. rank: bit `first row` per group, the selection scan, the ascending first rows
    const uint64_t nwords = (n + 63) / 64;
    DevBufRef marks = pool_alloc(ctx, nwords * 8 + 16);
    RV_HIP(hipMemsetAsync(marks->ptr, 0, nwords * 8 + 16, ctx->stream));
    hipLaunchKernelGGL(rvk::group_mark_first, dim3(grid_for_words(ctx, nslots + 1, rvk::kGroupAggThreads)), dim3(rvk::kGroupAggThreads), 0, ctx->stream, t, nslots,
                       static_cast<unsigned long long *>(marks->ptr));
    RV_HIP(hipGetLastError());
    const rv_dcolumn sel = plain_view(RV_BOOLEAN, marks, n);
    DevBufRef excl = selection_prefix(ctx, &sel, r.groups);
    r.first_row = selection_to_indices(ctx, &sel, r.groups, excl);

    // 3. ids: every row's group position
    ctrl = prepare_ctrl(ctx, 0);
    if (keys.tuple) {
        RV_KEYS_DISPATCH(keys.nkeys, launch_ids_keys, ctx, tk, static_cast<const uint64_t *>(marks->ptr), static_cast<const uint64_t *>(excl->ptr), r.gids->ptr, wide,
                         &ctrl->err)
    }
    else if (wide)
        hipLaunchKernelGGL(rvk::group_ids<int64_t>, row_grid(n), dim3(rvk::kGroupAggThreads), 0, ctx->stream, t, static_cast<const uint64_t *>(marks->ptr),
                           static_cast<const uint64_t *>(excl->ptr), static_cast<int64_t *>(r.gids->ptr), &ctrl->err);
    else
        hipLaunchKernelGGL(rvk::group_ids<uint32_t>, row_grid(n), dim3(rvk::kGroupAggThreads), 0, ctx->stream, t, static_cast<const uint64_t *>(marks->ptr),
                           static_cast<const uint64_t *>(excl->ptr), static_cast<uint32_t *>(r.gids->ptr), &ctrl->err);
    RV_HIP(hipGetLastError());
    ctx->last_kernel = keys.tuple ? "group_ids<keys>" : "group_ids";
    return r;  // (the table, the marks and the scan go back to the pool; their next user runs behind these kernels on the stream)
}

// one accumulator of the integer pass
struct Acc {
    uint32_t kind;
    const rv_dcolumn *col;  // nullptr: AK_COUNT_ROWS
    DevBufRef buf;
};

DevBufRef new_acc(rv_ctx *ctx, uint64_t groups, bool ones) {
    const size_t bytes = std::max<size_t>(groups * 8, 16);
    DevBufRef b = pool_alloc(ctx, bytes);
    RV_HIP(hipMemsetAsync(b->ptr, ones ? 0xFF : 0, bytes, ctx->stream));
    return b;
}

// the accumulators, at most kAggOpsMost per launch -- in the LDS form as many as fit the LDS of one accumulator at the most groups
// (kGroupAggLdsGroupsMost x 8 bytes: 4 up to a quarter of that many groups, 1 from half on); returns the launches and names the form
uint64_t launch_accumulate(rv_ctx *ctx, const std::vector<Acc> &accs, const GroupIds &ids, uint64_t n, std::string &name) {
    const bool lds = ids.groups <= rvt::kGroupAggLdsGroupsMost;
    const size_t per_launch = lds ? std::min<size_t>(rvk::kAggOpsMost, rvt::kGroupAggLdsGroupsMost / ids.groups) : rvk::kAggOpsMost;
    const uint64_t ntiles = (n + rvk::kGroupAggTileRows - 1) / rvk::kGroupAggTileRows;
    // as many workgroups as are resident at once (8 per CU, fewer when their LDS fills the CU's 160 KiB first): each strides over the
    // tiles and, in the LDS form, flushes its accumulators once
    const size_t lds_bytes = lds ? std::min(per_launch, accs.size()) * ids.groups * 8 : 0;
    const uint64_t per_cu = lds_bytes ? std::clamp<uint64_t>((uint64_t{160} << 10) / lds_bytes, 1, 8) : 8;
    const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(ntiles, static_cast<uint64_t>(ctx->props.multiProcessorCount) * per_cu)));
    uint64_t launches = 0;
    for (size_t at = 0; at < accs.size(); at += per_launch, ++launches) {
        rvk::GroupAccParams p{};
        p.gids = static_cast<const uint32_t *>(ids.gids->ptr);
        p.n = n;
        p.groups = static_cast<uint32_t>(ids.groups);
        std::vector<const rv_dcolumn *> cols;
        for (size_t k = at; k < std::min(accs.size(), at + per_launch); ++k) {
            rvk::AggAcc &a = p.acc[p.nacc++];
            a.acc = static_cast<unsigned long long *>(accs[k].buf->ptr);
            a.kind = accs[k].kind;
            if (!accs[k].col) continue;
            size_t c = 0;
            while (c < cols.size() && cols[c] != accs[k].col) ++c;
            if (c == cols.size()) {
                cols.push_back(accs[k].col);
                p.cols[c] = dev_view(accs[k].col);
            }
            a.col = static_cast<uint32_t>(c);
        }
        if (lds) {
            const size_t bytes = static_cast<size_t>(p.nacc) * p.groups * 8;  // past 64 KiB a kernel's dynamic LDS has to be enabled, once
            const void *fn = reinterpret_cast<const void *>(&rvk::group_accumulate<true>);
            size_t &enabled = ctx->lds_enabled[fn];
            if (bytes > (size_t{64} << 10) && bytes > enabled) {
                RV_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(rvt::kGroupAggLdsGroupsMost * 8)));
                enabled = rvt::kGroupAggLdsGroupsMost * 8;
            }
            hipLaunchKernelGGL(rvk::group_accumulate<true>, grid, dim3(rvk::kGroupAggThreads), bytes, ctx->stream, p);
        }
        else hipLaunchKernelGGL(rvk::group_accumulate<false>, grid, dim3(rvk::kGroupAggThreads), 0, ctx->stream, p);
        RV_HIP(hipGetLastError());
    }
    if (launches) name = lds ? "group_accumulate<lds>" : "group_accumulate<global>";
    return launches;
}

// rows grouped by id, each group ascending: a stable radix sort of (gid, row) over the bits the ids take
struct GroupLists {
    DevBufRef rows, starts;
};
GroupLists group_lists(rv_ctx *ctx, const GroupIds &ids, uint64_t n) {
    GroupLists L;
    L.rows = pool_alloc(ctx, n * 4 + 16);
    L.starts = pool_alloc(ctx, (ids.groups + 1) * 8 + 16);
    DevBufRef rows_in = pool_alloc(ctx, n * 4 + 16), gids_out = pool_alloc(ctx, n * 4 + 16);
    const int grid = grid_for_words(ctx, n, rvk::kGroupAggThreads);
    hipLaunchKernelGGL(rvk::group_iota_rows, dim3(grid), dim3(rvk::kGroupAggThreads), 0, ctx->stream, n, static_cast<uint32_t *>(rows_in->ptr));
    RV_HIP(hipGetLastError());
    unsigned end_bit = 1;
    while (end_bit < 32 && (uint64_t{1} << end_bit) < ids.groups) ++end_bit;
    const uint32_t *gids = static_cast<const uint32_t *>(ids.gids->ptr);
    size_t temp_bytes = 0;
    RV_HIP(rocprim::radix_sort_pairs(nullptr, temp_bytes, gids, static_cast<uint32_t *>(gids_out->ptr), static_cast<const uint32_t *>(rows_in->ptr),
                                     static_cast<uint32_t *>(L.rows->ptr), static_cast<size_t>(n), 0u, end_bit, ctx->stream));
    DevBufRef temp = pool_alloc(ctx, std::max<size_t>(temp_bytes, 16));
    RV_HIP(rocprim::radix_sort_pairs(temp->ptr, temp_bytes, gids, static_cast<uint32_t *>(gids_out->ptr), static_cast<const uint32_t *>(rows_in->ptr),
                                     static_cast<uint32_t *>(L.rows->ptr), static_cast<size_t>(n), 0u, end_bit, ctx->stream));
    hipLaunchKernelGGL(rvk::group_list_starts, dim3(grid), dim3(rvk::kGroupAggThreads), 0, ctx->stream, static_cast<const uint32_t *>(gids_out->ptr), n,
                       static_cast<uint32_t>(ids.groups), static_cast<uint64_t *>(L.starts->ptr));
    RV_HIP(hipGetLastError());
    return L;
}

void check_specs(const char *what, uint64_t rows, const rv_dcolumn *const *value_cols, uint32_t n_values, const rv_agg_spec *specs, uint32_t n_specs) {
    require(n_specs >= 1, RV_ERR_INVALID_ARG, fmt("%s: no aggregates", what));
    for (uint32_t c = 0; c < n_values; ++c) require(value_cols[c] != nullptr, RV_ERR_INVALID_ARG, fmt("%s: value column %u is NULL", what, c));
    for (uint32_t j = 0; j < n_specs; ++j) {
        require(specs[j].op <= static_cast<uint32_t>(RV_AGG_MAX), RV_ERR_INVALID_ARG, fmt("%s: aggregate %u has the unknown op %u", what, j, specs[j].op));
        require(specs[j].op == RV_AGG_COUNT_ROWS || specs[j].col < n_values, RV_ERR_INVALID_ARG,
                fmt("%s: aggregate %u reads value column %u of %u", what, j, specs[j].col, n_values));
    }
    for (uint32_t c = 0; c < n_values; ++c)
        require(value_cols[c]->length == rows, RV_ERR_LENGTH_MISMATCH,
                fmt("%s: value column %u has %llu rows, the key %llu", what, c, static_cast<unsigned long long>(value_cols[c]->length),
                    static_cast<unsigned long long>(rows)));
    for (uint32_t j = 0; j < n_specs; ++j) {
        if (specs[j].op == RV_AGG_COUNT_ROWS) continue;
        const rv_dtype d = value_cols[specs[j].col]->dtype;
        if (specs[j].op == RV_AGG_COUNT)
            require(is_value_type(d) || d == RV_BOOLEAN || d == RV_STRING || d == RV_NULL, RV_ERR_UNSUPPORTED, fmt("%s: aggregate %u: unsupported dtype", what, j));
        else
            require(is_value_type(d), RV_ERR_TYPE_MISMATCH, fmt("%s: aggregate %u: SUM / MIN / MAX take an Int64 or Float64 column", what, j));
    }
}

// the key list of the _keys entry points: one to kGroupKeysMost columns of one length, none of them String
void check_group_keys(const rv_dcolumn *const *keys, uint32_t nkeys, const char *what) {
    require(nkeys >= 1 && nkeys <= static_cast<uint32_t>(rvk::kGroupKeysMost), RV_ERR_INVALID_ARG,
            fmt("%s: %u key columns; one to %d are taken", what, nkeys, rvk::kGroupKeysMost));
    for (uint32_t k = 0; k < nkeys; ++k) require(keys[k] != nullptr, RV_ERR_INVALID_ARG, fmt("%s: key column %u is NULL", what, k));
    for (uint32_t k = 1; k < nkeys; ++k)
        require(keys[k]->length == keys[0]->length, RV_ERR_LENGTH_MISMATCH,
                fmt("%s: key column %u has %llu rows, key column 0 %llu", what, k, static_cast<unsigned long long>(keys[k]->length),
                    static_cast<unsigned long long>(keys[0]->length)));
    for (uint32_t k = 0; k < nkeys; ++k)
        require(keys[k]->dtype == RV_INT64 || keys[k]->dtype == RV_FLOAT64 || keys[k]->dtype == RV_BOOLEAN || keys[k]->dtype == RV_NULL, RV_ERR_UNSUPPORTED,
                fmt("%s: key column %u: Int64, Float64, Boolean (and Null) key columns are supported on the device; String keys go through rv_string_dict_build ids",
                    what, k));
    require(keys[0]->length < (uint64_t{1} << 32), RV_ERR_UNSUPPORTED, fmt("%s: keys of 2^32 rows or more are not supported (32-bit row ids, as the join)", what));
}

// one Int64 or Null key is what the single-key passes take: same groups by definition, one hash and one cell per probe
KeyCols key_cols(const rv_dcolumn *const *keys, uint32_t nkeys) {
    return KeyCols{keys, nkeys, !(nkeys == 1 && (keys[0]->dtype == RV_INT64 || keys[0]->dtype == RV_NULL))};
}

// everything behind the group ids; out: the key cells of every key column, then the aggregates
void hash_aggregate(rv_ctx *ctx, const KeyCols &keys, const char *what, const rv_dcolumn *const *value_cols, const rv_agg_spec *specs, uint32_t n_specs,
                    rv_dcolumn **out, rv_dcolumn **out_first_row, uint64_t *out_groups) {
    const uint64_t n = keys.rows();
    GroupIds ids = group_ids_of(ctx, keys, what, false);
    const uint64_t G = ids.groups;
    std::vector<std::unique_ptr<rv_dcolumn>> outs(n_specs);
    std::vector<Acc> accs;
    std::vector<std::pair<uint32_t, DevBufRef>> minmax;  // (output, its non-null counts)
    std::vector<uint32_t> fsums;
    for (uint32_t j = 0; j < n_specs; ++j) {
        const uint32_t op = specs[j].op;
        const rv_dcolumn *col = op == RV_AGG_COUNT_ROWS ? nullptr : value_cols[specs[j].col];
        auto o = std::make_unique<rv_dcolumn>();
        o->dtype = op <= static_cast<uint32_t>(RV_AGG_COUNT) ? RV_INT64 : col->dtype;
        o->length = G;
        o->null_count = 0;
        o->values = new_acc(ctx, G, op == RV_AGG_MIN);
        if (op == RV_AGG_SUM && col->dtype == RV_FLOAT64) fsums.push_back(j);
        else {
            accs.push_back(Acc{op, col, o->values});  // rv_agg_op and the AK_ kinds share their values
            if (op == RV_AGG_MIN || op == RV_AGG_MAX) {
                minmax.emplace_back(j, new_acc(ctx, G, false));
                accs.push_back(Acc{rvk::AK_COUNT, col, minmax.back().second});
            }
        }
        outs[j] = std::move(o);
    }
    static_assert(int(RV_AGG_COUNT_ROWS) == int(rvk::AK_COUNT_ROWS) && int(RV_AGG_COUNT) == int(rvk::AK_COUNT) && int(RV_AGG_SUM) == int(rvk::AK_SUM_I64) &&
                      int(RV_AGG_MIN) == int(rvk::AK_MIN) && int(RV_AGG_MAX) == int(rvk::AK_MAX), "rv_agg_op and the accumulator kinds");
    if (G) {
        // group_ids_of left its id pass queued with a fresh control block: ctrl->err is that pass's flag, read with the first read-back
        NullCounts nulls(ctx, outs, static_cast<Ctrl *>(ctx->d_ctrl));
        bool ids_checked = false;
        auto settle = [&] {
            const Ctrl *h = nulls.settle();
            if (ids_checked) return;
            if (!h) h = fetch_ctrl(ctx);  // no MIN / MAX: the read-back is the flag's alone
            require(h->err == 0, RV_ERR_INTERNAL, fmt("%s: a row's key was not found in the group table", what));
            ids_checked = true;
        };
        PassTimer timer(ctx);
        std::string name;
        if (!accs.empty()) {
            timer.start();
            timer.launches += launch_accumulate(ctx, accs, ids, n, name);
        }
        if (!fsums.empty()) {
            timer.start();
            GroupLists L = group_lists(ctx, ids, n);
            for (uint32_t j : fsums) {
                hipLaunchKernelGGL(rvk::group_f64_sum, dim3(static_cast<uint32_t>((G + 3) / 4)), dim3(rvk::kGroupAggThreads), 0, ctx->stream,
                                   dev_view(value_cols[specs[j].col]), static_cast<const uint32_t *>(L.rows->ptr), static_cast<const uint64_t *>(L.starts->ptr),
                                   static_cast<uint32_t>(G), rvt::kGroupAggWaveListMost, static_cast<double *>(outs[j]->values->ptr));
                RV_HIP(hipGetLastError());
                ++timer.launches;
            }
            name += name.empty() ? "group_f64_sum" : "+group_f64_sum";
        }
        timer.stop();
        ctx->last_kernel = name;
        // MIN / MAX: the winning bits in place, the validity, the nulls
        for (const auto &[j, counts] : minmax) {
            if (nulls.pending.size() == 8) settle();
            rv_dcolumn *o = outs[j].get();
            unsigned long long *null_cells = nulls.attach(j, G);
            hipLaunchKernelGGL(rvk::group_minmax_finish, row_grid(G), dim3(rvk::kGroupAggThreads), 0, ctx->stream, static_cast<unsigned long long *>(o->values->ptr),
                               static_cast<const unsigned long long *>(counts->ptr), G, o->dtype == RV_FLOAT64 ? 1 : 0, static_cast<uint64_t *>(o->validity->ptr),
                               null_cells);
            RV_HIP(hipGetLastError());
        }
        settle();
        timer.add();
    }
    // out[0 .. nkeys): the key cells at the first rows (a gather with read-backs of its own: after this call's control block has been read)
    rv_dcolumn *key_cells[rvk::kGroupKeysMost] = {};
    take_on_device(ctx, keys.cols, keys.nkeys, static_cast<const uint64_t *>(ids.first_row->ptr), G, key_cells, false);
    std::vector<std::unique_ptr<rv_dcolumn>> cells(keys.nkeys);
    for (uint32_t k = 0; k < keys.nkeys; ++k) cells[k].reset(key_cells[k]);
    RV_HIP(hipStreamSynchronize(ctx->stream));  // the ids, the lists and the count accumulators go back to the pool
    if (out_first_row) *out_first_row = index_column(ids.first_row, G);  // (the last step that can fail: before the outputs are handed over)
    for (uint32_t k = 0; k < keys.nkeys; ++k) out[k] = cells[k].release();
    for (uint32_t j = 0; j < n_specs; ++j) out[keys.nkeys + j] = outs[j].release();
    if (out_groups) *out_groups = G;
}

// rv_group_ids and rv_group_ids_keys behind their checks
void group_ids_call(rv_ctx *ctx, const KeyCols &keys, const char *what, rv_dcolumn **out_gids, rv_dcolumn **out_first_row, uint64_t *out_groups) {
    set_device(ctx);
    breaker_call(ctx, nullptr, 0, [&] {  // both outputs are handed over by the last step, which cannot fail
        GroupIds ids = group_ids_of(ctx, keys, what, true);
        require(fetch_ctrl(ctx)->err == 0, RV_ERR_INTERNAL, fmt("%s: a row's key was not found in the group table", what));
        std::unique_ptr<rv_dcolumn> a(index_column(ids.gids, keys.rows())), b(index_column(ids.first_row, ids.groups));
        *out_gids = a.release();
        *out_first_row = b.release();
        if (out_groups) *out_groups = ids.groups;
    });
}

// rv_hash_aggregate and rv_hash_aggregate_keys behind their checks
void hash_aggregate_call(rv_ctx *ctx, const KeyCols &keys, const char *what, const rv_dcolumn *const *value_cols, const rv_agg_spec *specs, uint32_t n_specs,
                         rv_dcolumn **out, rv_dcolumn **out_first_row, uint64_t *out_groups) {
    for (uint32_t j = 0; j < keys.nkeys + n_specs; ++j) out[j] = nullptr;
    if (out_first_row) *out_first_row = nullptr;
    set_device(ctx);
    breaker_call(ctx, out, keys.nkeys + n_specs, [&] { hash_aggregate(ctx, keys, what, value_cols, specs, n_specs, out, out_first_row, out_groups); });
}

}  // namespace

// ---- the window operator's way in (window.hip): rv_group_ids_keys' checks and its dense Int64 ids, without the handles
void check_partition_keys(const rv_dcolumn *const *keys, uint32_t nkeys, const char *what) { check_group_keys(keys, nkeys, what); }
DevBufRef partition_ids(rv_ctx *ctx, const rv_dcolumn *const *keys, uint32_t nkeys, const char *what) {
    GroupIds ids = group_ids_of(ctx, key_cols(keys, nkeys), what, true);
    require(fetch_ctrl(ctx)->err == 0, RV_ERR_INTERNAL, fmt("%s: a row's key was not found in the group table", what));
    return ids.gids;
}
}  // namespace rvl

extern "C" {

rv_status rv_group_ids(rv_ctx *ctx, const rv_dcolumn *key, rv_dcolumn **out_gids, rv_dcolumn **out_first_row, uint64_t *out_groups) {
    return guarded([&] {
        require(ctx && key && out_gids && out_first_row, RV_ERR_INVALID_ARG, "rv_group_ids: NULL argument");
        *out_gids = *out_first_row = nullptr;
        check_group_key(key, "rv_group_ids");
        group_ids_call(ctx, KeyCols{&key, 1, false}, "rv_group_ids", out_gids, out_first_row, out_groups);
    });
}

rv_status rv_hash_aggregate(rv_ctx *ctx, const rv_dcolumn *key, const rv_dcolumn *const *value_cols, uint32_t n_values, const rv_agg_spec *specs,
                            uint32_t n_specs, rv_dcolumn **out, rv_dcolumn **out_first_row, uint64_t *out_groups) {
    return guarded([&] {
        require(ctx && key && specs && out && (value_cols || n_values == 0), RV_ERR_INVALID_ARG, "rv_hash_aggregate: NULL argument");
        check_specs("rv_hash_aggregate", key->length, value_cols, n_values, specs, n_specs);
        check_group_key(key, "rv_hash_aggregate");
        hash_aggregate_call(ctx, KeyCols{&key, 1, false}, "rv_hash_aggregate", value_cols, specs, n_specs, out, out_first_row, out_groups);
    });
}

rv_status rv_group_ids_keys(rv_ctx *ctx, const rv_dcolumn *const *keys, uint32_t nkeys, rv_dcolumn **out_gids, rv_dcolumn **out_first_row, uint64_t *out_groups) {
    return guarded([&] {
        require(ctx && keys && out_gids && out_first_row, RV_ERR_INVALID_ARG, "rv_group_ids_keys: NULL argument");
        *out_gids = *out_first_row = nullptr;
        check_group_keys(keys, nkeys, "rv_group_ids_keys");
        group_ids_call(ctx, key_cols(keys, nkeys), "rv_group_ids_keys", out_gids, out_first_row, out_groups);
    });
}

rv_status rv_hash_aggregate_keys(rv_ctx *ctx, const rv_dcolumn *const *keys, uint32_t nkeys, const rv_dcolumn *const *value_cols, uint32_t n_values,
                                 const rv_agg_spec *specs, uint32_t n_specs, rv_dcolumn **out, rv_dcolumn **out_first_row, uint64_t *out_groups) {
    return guarded([&] {
        require(ctx && keys && specs && out && (value_cols || n_values == 0), RV_ERR_INVALID_ARG, "rv_hash_aggregate_keys: NULL argument");
        check_group_keys(keys, nkeys, "rv_hash_aggregate_keys");
        check_specs("rv_hash_aggregate_keys", keys[0]->length, value_cols, n_values, specs, n_specs);
        hash_aggregate_call(ctx, key_cols(keys, nkeys), "rv_hash_aggregate_keys", value_cols, specs, n_specs, out, out_first_row, out_groups);
    });
}

}  // extern "C"
