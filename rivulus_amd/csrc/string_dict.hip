// Device string dictionary: a String column reduced to Int64 ids, once, so that String join keys run through the Int64 join.
// One unit of the backend library behind include/rivulus_gpu.h (gfx950 only; compiled with hipcc).  Shared helpers are declared in
// launch.hpp (namespace rvl); the kernels are in string_dict_kernel.hpp, the hash in string_hash.hpp.
#include "string_dict_kernel.hpp"
#include "breaker_steps.hpp"

using namespace rvh;
using namespace rvl;

// The distinct non-null strings of `source` (string_dict_kernel.hpp has the layout).  Encodes any number of String columns.
struct rv_string_dict {
    rv_dcolumn source;  // a view that shares the column's buffers, as rv_slice does: the bytes behind every slot
    uint64_t rows = 0, distinct = 0, nslots = 0;
    uint64_t hash_mask = ~0ull;
    DevBufRef slots;
    std::shared_ptr<rvh::Pool> pool;  // keeps the blocks' pool alive with the dictionary
};

namespace rvl {
namespace {

rvk::StrColView str_view(const rv_dcolumn *c) {
    rvk::StrColView v{};
    if (c->dtype != RV_STRING) return v;
    v.offsets = static_cast<const int32_t *>(c->offsets->ptr);
    v.data = static_cast<const uint8_t *>(c->values->ptr);
    v.validity = c->validity ? static_cast<const uint8_t *>(c->validity->ptr) : nullptr;
    v.offset = c->offset;
    return v;
}

void check_column(const rv_dcolumn *col, const char *what) {
    require(col->dtype == RV_STRING || col->dtype == RV_NULL, RV_ERR_TYPE_MISMATCH, fmt("%s: not a String column", what));
    require(col->length < (uint64_t{1} << 32), RV_ERR_UNSUPPORTED, fmt("%s: columns of 2^32 rows or more are not supported (32-bit row ids, as the join)", what));
}

rvk::StrDictParams dict_params(const rv_string_dict *d, const rv_dcolumn *col, Ctrl *ctrl) {
    rvk::StrDictParams q{};
    q.slots = static_cast<unsigned long long *>(d->slots->ptr);
    q.slot_mask = d->nslots - 1;
    q.hash_mask = d->hash_mask;
    q.source = str_view(&d->source);
    q.col = str_view(col);
    q.n = col->length;
    q.error = &ctrl->err;
    return q;
}

dim3 dict_grid(uint64_t n) { return dim3(static_cast<uint32_t>((n + rvk::kStrDictThreads - 1) / rvk::kStrDictThreads)); }

// the ids column of `col`, queued behind whatever the stream holds; finish_ids completes it from the call's read-back
struct IdsLaunch {
    std::unique_ptr<rv_dcolumn> ids;
    bool counted = false;  // the kernel counts the non-null rows (ctrl->pops[1])
};

IdsLaunch queue_encode(rv_ctx *ctx, const rv_string_dict *d, const rv_dcolumn *col, Ctrl *ctrl) {
    IdsLaunch L;
    const uint64_t n = col->length;
    L.ids = std::make_unique<rv_dcolumn>();
    L.ids->dtype = RV_INT64;
    L.ids->length = n;
    L.ids->null_count = 0;
    L.ids->values = pool_alloc(ctx, std::max<size_t>(n * 8, 16));
    if (n == 0) return L;
    if (col->dtype == RV_NULL) {  // all nulls: placeholder values under an all-zero bitmap
        const size_t vb = std::max<size_t>(bitmap_words_bytes(n), 16);
        L.ids->validity = pool_alloc(ctx, vb);
        RV_HIP(hipMemsetAsync(L.ids->values->ptr, 0, n * 8, ctx->stream));
        RV_HIP(hipMemsetAsync(L.ids->validity->ptr, 0, vb, ctx->stream));
        L.ids->null_count = static_cast<int64_t>(n);
        return L;
    }
    rvk::StrDictParams q = dict_params(d, col, ctrl);
    q.ids = static_cast<int64_t *>(L.ids->values->ptr);
    if (col->validity) {  // re-based to bit 0
        L.ids->validity = pool_alloc(ctx, std::max<size_t>(bitmap_words_bytes(n), 16));
        hipLaunchKernelGGL(rvk::copy_bits_kernel, dim3(grid_for_words(ctx, (n + 63) / 64, 256)), dim3(256), 0, ctx->stream,
                           static_cast<const uint8_t *>(col->validity->ptr), static_cast<uint64_t>(col->validity->bytes), col->offset, n,
                           static_cast<uint64_t *>(L.ids->validity->ptr));
        q.valid_count = striped(ctx, &ctrl->pops[1]);
        L.counted = true;
    }
    hipLaunchKernelGGL(rvk::str_dict_encode, dict_grid(n), dim3(rvk::kStrDictThreads), 0, ctx->stream, q);
    RV_HIP(hipGetLastError());
    ctx->last_kernel = "str_dict_encode";
    return L;
}

rv_dcolumn *finish_ids(IdsLaunch &L, const Ctrl *fetched) {
    if (L.counted) {
        L.ids->null_count = static_cast<int64_t>(L.ids->length - fetched->pops[1]);
        if (L.ids->null_count == 0) L.ids->validity.reset();  // absent without nulls, as every builder leaves it
    }
    return L.ids.release();
}

}  // namespace
}  // namespace rvl

extern "C" {

rv_status rv_string_dict_build(rv_ctx *ctx, const rv_dcolumn *col, rv_string_dict **out, rv_dcolumn **out_ids) {
    return guarded([&] {
        require(ctx && col && out, RV_ERR_INVALID_ARG, "rv_string_dict_build: NULL argument");
        *out = nullptr;
        if (out_ids) *out_ids = nullptr;
        check_column(col, "rv_string_dict_build");
        set_device(ctx);
        const uint64_t n = col->length;
        auto d = std::make_unique<rv_string_dict>();
        d->source = *col;
        d->rows = n;
        d->pool = ctx->pool;
        if (ctx->opt_string_hash_bits > 0 && ctx->opt_string_hash_bits < 64) d->hash_mask = (uint64_t{1} << ctx->opt_string_hash_bits) - 1;
        // at most half full: sized by the non-null rows where the column knows them, by all its rows where it does not
        const uint64_t keyed_most = col->dtype == RV_NULL ? 0 : col->null_count >= 0 ? n - static_cast<uint64_t>(col->null_count) : n;
        uint64_t nslots = 16;
        while (nslots < rvt::kStrDictSlotsPerRow * keyed_most) nslots *= 2;
        d->nslots = nslots;
        d->slots = pool_alloc(ctx, nslots * 8);
        RV_HIP(hipMemsetAsync(d->slots->ptr, 0, nslots * 8, ctx->stream));
        Ctrl *ctrl = prepare_ctrl(ctx, 0);
        PassTimer timer(ctx);
        timer.start();
        const bool insert = n && col->dtype == RV_STRING;
        if (insert) {
            rvk::StrDictParams q = dict_params(d.get(), col, ctrl);
            q.distinct = striped(ctx, &ctrl->pops[0]);
            hipLaunchKernelGGL(rvk::str_dict_insert, dict_grid(n), dim3(rvk::kStrDictThreads), 0, ctx->stream, q);
            RV_HIP(hipGetLastError());
            ctx->last_kernel = "str_dict_insert";
        }
        IdsLaunch L;
        if (out_ids) L = queue_encode(ctx, d.get(), col, ctrl);
        timer.stop();
        const Ctrl *h = fetch_ctrl(ctx);  // the call's one read-back: distinct strings, non-null rows, the error flag
        timer.launches = (insert ? 1 : 0) + (out_ids && insert ? 1 : 0);
        timer.add();
        require(h->err == 0, RV_ERR_INTERNAL, "rv_string_dict_build: a chain walk exhausted the table");
        d->distinct = h->pops[0];
        if (out_ids) *out_ids = finish_ids(L, h);
        *out = d.release();
    });
}

rv_status rv_string_dict_encode(rv_ctx *ctx, const rv_string_dict *dict, const rv_dcolumn *col, rv_dcolumn **out_ids) {
    return guarded([&] {
        require(ctx && dict && col && out_ids, RV_ERR_INVALID_ARG, "rv_string_dict_encode: NULL argument");
        *out_ids = nullptr;
        check_column(col, "rv_string_dict_encode");
        set_device(ctx);
        Ctrl *ctrl = prepare_ctrl(ctx, 0);
        PassTimer timer(ctx);
        timer.start();
        IdsLaunch L = queue_encode(ctx, dict, col, ctrl);
        timer.stop();
        const Ctrl *h = fetch_ctrl(ctx);
        timer.launches = col->length && col->dtype == RV_STRING ? 1 : 0;
        timer.add();
        require(h->err == 0, RV_ERR_INTERNAL, "rv_string_dict_encode: a chain walk exhausted the table");
        *out_ids = finish_ids(L, h);
    });
}

rv_status rv_string_dict_info(const rv_string_dict *dict, uint64_t *rows, uint64_t *distinct, uint64_t *slots) {
    return guarded([&] {
        require(dict, RV_ERR_INVALID_ARG, "rv_string_dict_info: NULL dictionary");
        if (rows) *rows = dict->rows;
        if (distinct) *distinct = dict->distinct;
        if (slots) *slots = dict->nslots;
    });
}

rv_status rv_string_dict_free(rv_ctx *ctx, rv_string_dict *dict) {
    return guarded([&] {
        require(ctx, RV_ERR_INVALID_ARG, "rv_string_dict_free: NULL context");
        if (dict) {
            RV_HIP(hipStreamSynchronize(ctx->stream));
            delete dict;
        }
    });
}

}  // extern "C"
