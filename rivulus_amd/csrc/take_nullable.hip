// RecordBatch::take over a NULLABLE index list on the device: rv_take_device_nullable and the outer joins' gathers.
// One unit of the backend library behind include/rivulus_gpu.h (gfx950 only; compiled with hipcc).  Shared helpers and the
// functions the units call across each other are declared in launch.hpp (namespace rvl); the kernels are in take_nullable_kernel.hpp.
// A unit of its own: take_concat.hip and strings.hip, which hold the gathers of every other operator, are not touched by it.
#include "launch.hpp"
#include "take_nullable_kernel.hpp"

using namespace rvh;
using namespace rvl;

namespace rvl {
namespace {

// gather_strings (strings.hip) with a null index giving a null element: length 0, validity bit clear
rv_dcolumn *gather_strings_nullable(rv_ctx *ctx, const rv_dcolumn *src, const uint64_t *d_indices, uint64_t n, const rvk::TakeNulls &z) {
    auto o = empty_string_gather(ctx, n);
    if (n == 0) return o.release();
    DevBufRef lengths = pool_alloc(ctx, n * 4 + 16), starts = pool_alloc(ctx, n * 4 + 16);
    o->validity = pool_alloc(ctx, std::max<size_t>(bitmap_words_bytes(n), 16));
    Ctrl *ctrl = prepare_ctrl(ctx, 0);
    rvk::StrGather g{};
    g.offsets = static_cast<const int32_t *>(src->offsets->ptr);
    g.data = static_cast<const uint8_t *>(src->values->ptr);
    g.validity = src->validity ? static_cast<const uint8_t *>(src->validity->ptr) : nullptr;
    g.validity_bytes = src->validity ? src->validity->bytes : 0;
    g.offset = src->offset;
    g.src_length = src->length;
    g.indices = d_indices;
    g.n = n;
    g.lengths = static_cast<uint32_t *>(lengths->ptr);
    g.starts = static_cast<int32_t *>(starts->ptr);
    g.out_validity = static_cast<uint64_t *>(o->validity->ptr);
    g.valid_pop = striped(ctx, &ctrl->valid_pop[0]);
    g.err = &ctrl->err;
    hipLaunchKernelGGL(rvk::str_gather_lengths_nullable, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, ctx->stream, g, z);
    RV_HIP(hipGetLastError());
    finish_string_gather(ctx, o.get(), g, n, ctrl);
    return o.release();
}

}  // namespace

// take_on_device (take_concat.hip) over a nullable index list: the bounds pre-pass skips null indices, every output gets a bitmap,
// dropped again when no null cell came out.
void take_nullable_on_device(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const uint64_t *d_idx, uint64_t n_indices, rv_dcolumn **out,
                             bool check_bounds, const IndexNulls &nulls) {
    const rvk::TakeNulls z{nulls.validity, nulls.offset};
    const uint64_t rows = ncols ? cols[0]->length : 0;
    for (uint32_t c = 0; c < ncols; ++c) {
        require(is_value_type(cols[c]->dtype) || cols[c]->dtype == RV_BOOLEAN || cols[c]->dtype == RV_STRING || cols[c]->dtype == RV_NULL,
                RV_ERR_UNSUPPORTED, "rv_take: unsupported dtype");
        out[c] = nullptr;
    }
    if (n_indices && check_bounds) {  // the FIRST non-null index that is out of bounds, with rv_take_device's text
        Ctrl *ctrl = prepare_ctrl(ctx, 0);
        RV_HIP(hipMemsetAsync(&ctrl->pops[0], 0xFF, 8, ctx->stream));
        hipLaunchKernelGGL(rvk::take_bounds_nullable_kernel, dim3(grid_for_words(ctx, n_indices, 256)), dim3(256), 0, ctx->stream, d_idx, z, n_indices, rows,
                           &ctrl->pops[0]);
        RV_HIP(hipGetLastError());
        const Ctrl *h = fetch_ctrl(ctx);
        if (h->pops[0] != ~0ull) {
            uint64_t bad = 0;
            RV_HIP(hipMemcpyAsync(&bad, d_idx + h->pops[0], 8, hipMemcpyDeviceToHost, ctx->stream));
            RV_HIP(hipStreamSynchronize(ctx->stream));
            throw Error(RV_ERR_OUT_OF_BOUNDS, fmt("Index %llu out of bounds for %llu rows", static_cast<unsigned long long>(bad), static_cast<unsigned long long>(rows)));
        }
    }
    try {
        for (uint32_t c = 0; c < ncols; ++c) {
            if (cols[c]->dtype == RV_STRING) {
                out[c] = gather_strings_nullable(ctx, cols[c], d_idx, n_indices, z);
                continue;
            }
            if (cols[c]->dtype == RV_NULL) {  // a NullArray stays a NullArray
                auto o = std::make_unique<rv_dcolumn>();
                o->dtype = RV_NULL;
                o->length = n_indices;
                o->null_count = static_cast<int64_t>(n_indices);
                out[c] = o.release();
                continue;
            }
            auto o = std::make_unique<rv_dcolumn>();
            o->dtype = cols[c]->dtype;
            o->length = n_indices;
            o->values = pool_alloc(ctx, std::max<size_t>(elem_bytes(cols[c]->dtype, n_indices), 16));
            o->validity = pool_alloc(ctx, std::max<size_t>(bitmap_words_bytes(n_indices), 16));
            Ctrl *ctrl = prepare_ctrl(ctx, 0);
            rvk::TakeParams p{};
            p.col = dev_view(cols[c]);
            p.indices = d_idx;
            p.out_values = static_cast<uint64_t *>(o->values->ptr);
            p.out_validity = static_cast<uint64_t *>(o->validity->ptr);
            p.out_valid_pop = striped(ctx, &ctrl->valid_pop[0]);
            p.n = n_indices;
            if (n_indices) {
                hipLaunchKernelGGL(rvk::take_nullable_kernel, dim3(grid_for_words(ctx, n_indices, 256)), dim3(256), 0, ctx->stream, p, z);
                RV_HIP(hipGetLastError());
            }
            const Ctrl *h = fetch_ctrl(ctx);
            o->null_count = static_cast<int64_t>(n_indices - h->valid_pop[0]);
            if (o->null_count == 0) o->validity.reset();
            out[c] = o.release();
        }
    } catch (...) {
        (void)hipStreamSynchronize(ctx->stream);
        drop_outputs(out, ncols);
        throw;
    }
}
}  // namespace rvl

extern "C" {

rv_status rv_take_device_nullable(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const rv_dcolumn *indices, rv_dcolumn **out) {
    return guarded([&] {
        require(ctx && indices && (out || ncols == 0), RV_ERR_INVALID_ARG, "rv_take_device_nullable: NULL argument");
        require(indices->dtype == RV_INT64, RV_ERR_TYPE_MISMATCH, "rv_take_device_nullable: the index list must be an Int64 array");
        check_batch(cols, ncols);
        set_device(ctx);
        const uint64_t *d_idx = static_cast<const uint64_t *>(indices->values->ptr) + indices->offset;
        if (indices->validity) {
            const IndexNulls nulls{static_cast<const uint8_t *>(indices->validity->ptr), indices->offset};
            take_nullable_on_device(ctx, cols, ncols, d_idx, indices->length, out, true, nulls);
        } else {
            take_on_device(ctx, cols, ncols, d_idx, indices->length, out);  // no bitmap, no null index: rv_take_device
        }
        RV_HIP(hipStreamSynchronize(ctx->stream));
    });
}

}  // extern "C"
