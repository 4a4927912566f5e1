// Narrow companions of resident Int64 columns (runtime.hpp, NarrowCodes): which views may read one, what the lean passes have read of
// a buffer so far, and the build -- a min/max pass, the width chosen from the range, the pack pass -- queued on the context's stream
// behind the pass that completed the buffer's last whole scan.  One unit of the backend library behind include/rivulus_gpu.h.
#include "launch.hpp"
#include "narrow_kernel.hpp"

using namespace rvh;

namespace rvl {

// a view of a buffer that could ever have a companion
static bool eligible(rv_ctx *ctx, const rv_dcolumn *col) {
    return col && col->values && col->values->pool == ctx->pool &&
           rvn::buffer_eligible(col->values->id, col->dtype == RV_INT64, col->validity != nullptr);
}

// A view was made of `col` (rv_slice) or handed to a pass: the buffer's columns span at least this many elements.
void narrow_note_extent(rv_ctx *ctx, const rv_dcolumn *col) {
    if (eligible(ctx, col)) col->values->scan.note_extent(col->offset + col->length);
}

// The companion a lean pass over `col` may read instead of the 8-byte values, or nullptr: built, covering the view, and the view's
// first element aligned for the pair loads (an odd offset runs the plain kernel: same result).
const NarrowCodes *narrow_codes_for(rv_ctx *ctx, const rv_dcolumn *col) {
    if (ctx->opt_narrow_codes < 0 || !eligible(ctx, col)) return nullptr;
    const NarrowCodes *nc = col->values->narrow.get();
    if (!nc || !rvn::slice_aligned(col->offset) || !rvn::view_covered(col->offset, col->length, nc->count)) return nullptr;
    return nc;
}

// min / max, width, codes.  No companion (and no second try) when the range needs more than 32 bits or the pool has no memory for
// the codes: the query that triggered the build never fails because of it.
static void build(rv_ctx *ctx, DevBuf &buf) {
    const uint64_t count = buf.scan.extent;
    buf.narrow_refused = true;  // until the codes are queued
    if (count == 0 || count * 8 > buf.bytes) return;
    try {
        const int blocks = std::max(1, ctx->props.multiProcessorCount) * 8;
        DevBufRef mm = pool_alloc(ctx, 256);
        long long h[2] = {0x7FFFFFFFFFFFFFFFll, -0x7FFFFFFFFFFFFFFFll - 1};
        RV_HIP(hipMemcpyAsync(mm->ptr, h, sizeof h, hipMemcpyHostToDevice, ctx->stream));
        RV_HIP(hipStreamSynchronize(ctx->stream));  // (h is on the stack)
        const uint64_t pairs = std::max<uint64_t>(1, count / 2);
        const dim3 grid_mm(static_cast<uint32_t>(std::min<uint64_t>((pairs + 255) / 256, static_cast<uint64_t>(blocks))));
        hipLaunchKernelGGL(rvk::narrow_minmax_kernel, grid_mm, dim3(256), 0, ctx->stream, static_cast<const long long *>(buf.ptr), count, static_cast<long long *>(mm->ptr));
        RV_HIP(hipGetLastError());
        RV_HIP(hipMemcpyAsync(h, mm->ptr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        RV_HIP(hipStreamSynchronize(ctx->stream));
        const int width = rvn::code_bytes(rvn::value_range(h[0], h[1]));
        if (!width) return;
        auto nc = std::make_shared<NarrowCodes>();
        nc->codes = pool_alloc(ctx, static_cast<size_t>(count) * width + 16);
        nc->code_bytes = width;
        nc->base = h[0];
        nc->count = count;
        const uint64_t quads = std::max<uint64_t>(1, count / 4);
        const dim3 grid_pk(static_cast<uint32_t>(std::min<uint64_t>((quads + 255) / 256, static_cast<uint64_t>(blocks))));
        if (width == 2)
            hipLaunchKernelGGL(rvk::narrow_pack_kernel<2>, grid_pk, dim3(256), 0, ctx->stream, static_cast<const long long *>(buf.ptr), count, static_cast<long long>(nc->base), nc->codes->ptr);
        else
            hipLaunchKernelGGL(rvk::narrow_pack_kernel<4>, grid_pk, dim3(256), 0, ctx->stream, static_cast<const long long *>(buf.ptr), count, static_cast<long long>(nc->base), nc->codes->ptr);
        RV_HIP(hipGetLastError());
        // queued: every later pass of this context runs behind it on the same stream
        ctx->narrow_builds += 1;
        ctx->narrow_bytes += static_cast<uint64_t>(count) * width;
        buf.narrow = std::move(nc);
        buf.narrow_refused = false;
    } catch (const Error &e) {
        if (e.status != RV_ERR_OOM) throw;
        (void)hipGetLastError();
    }
}

// A lean one-column pass over elements [offset, offset + rows) of `buf` has finished (the host has waited for it): count it towards
// the buffer's whole scans, and build the companion when the rule says the buffer is worth it.
void narrow_after_pass(rv_ctx *ctx, DevBuf &buf, uint64_t offset, uint64_t rows) {
    if (ctx->opt_narrow_codes < 0 || buf.pool != ctx->pool || buf.id == 0) return;
    buf.scan.note_pass(offset, rows);
    if (buf.narrow || buf.narrow_refused) return;
    if (rvn::worth_building(ctx->opt_narrow_codes, buf.scan, rvt::kNarrowAfterWholeScans, rvt::kNarrowFromRows)) build(ctx, buf);
}

}  // namespace rvl
