// Narrow companions of resident Int64 columns (runtime.hpp, NarrowCodes): which views may read one, what the lean passes have read of
// a buffer so far, and the build -- a min/max pass, the width and layout chosen from the range and the triggering launch, the pack pass
// -- queued on the context's stream behind the pass that completed the buffer's last whole scan.  One unit of the backend library
// behind include/rivulus_gpu.h.
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
// first element aligned for its layout's loads -- even for the pair loads of 2- and 4-byte codes, a multiple of 384 and no per-batch
// counts for packed codes (narrow_rule.hpp, layout_to_read; any other launch runs the plain kernel: same result).
const NarrowCodes *narrow_codes_for(rv_ctx *ctx, const rv_dcolumn *col, bool batch_counts) {
    if (ctx->opt_narrow_codes < 0 || !eligible(ctx, col)) return nullptr;
    const DevBuf &buf = *col->values;
    bool found = false;
    const rvn::Layout layout = rvn::layout_to_read(rvn::LaunchKind{col->offset, batch_counts}, buf.narrow != nullptr, buf.narrow_packed != nullptr, &found);
    if (!found) return nullptr;
    const NarrowCodes *nc = layout == rvn::Layout::kPacked ? buf.narrow_packed.get() : buf.narrow.get();
    if (!rvn::slice_aligned(col->offset) || !rvn::view_covered(col->offset, col->length, nc->count)) return nullptr;
    return nc;
}

// min / max, width and layout, codes.  `second`: the buffer has one companion already and the launches that cannot read it have
// completed their own whole scans -- the other layout is built beside it.  No companion (and no second try) when the range needs more
// than 32 bits or the pool has no memory for the codes: the query that triggered the build never fails because of it.
static void build(rv_ctx *ctx, DevBuf &buf, const rvn::LaunchKind &kind, bool second) {
    const NarrowCodes *have = second ? (buf.narrow ? buf.narrow.get() : buf.narrow_packed.get()) : nullptr;
    const uint64_t count = have ? have->count : buf.scan.extent;  // (the second companion covers what the first does: its base and range are those elements')
    bool &refused = second ? buf.other_refused : buf.narrow_refused;
    refused = true;  // until the codes are queued
    if (count == 0 || count * 8 > buf.bytes) return;
    try {
        const int blocks = std::max(1, ctx->props.multiProcessorCount) * 8;
        int64_t base = have ? have->base : 0;
        uint64_t range = have ? have->range : 0;
        if (!have) {
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
            base = h[0];
            range = rvn::value_range(h[0], h[1]);
        }
        bool wanted = true;
        const rvn::Layout layout = second ? rvn::second_layout(ctx->opt_narrow_codes, range, kind, buf.narrow_packed != nullptr, &wanted)
                                          : rvn::layout_to_build(ctx->opt_narrow_codes, range, kind);
        const int width = layout == rvn::Layout::kPacked ? 2 : rvn::code_bytes(range);
        if (!width || !wanted) return;
        auto nc = std::make_shared<NarrowCodes>();
        const uint64_t bytes = layout == rvn::Layout::kPacked ? rvn::packed_bytes(count) : count * static_cast<uint64_t>(width);
        nc->codes = pool_alloc(ctx, static_cast<size_t>(bytes) + 16);
        nc->layout = layout;
        nc->code_bytes = width;
        nc->base = base;
        nc->range = range;
        nc->count = count;
        if (layout == rvn::Layout::kPacked) {
            const uint64_t words = bytes / 8;
            const dim3 grid_pk(static_cast<uint32_t>(std::min<uint64_t>((words + 255) / 256, static_cast<uint64_t>(blocks))));
            hipLaunchKernelGGL(rvk::narrow_pack10_kernel, grid_pk, dim3(256), 0, ctx->stream, static_cast<const long long *>(buf.ptr), count, static_cast<long long>(nc->base), words,
                               static_cast<rvk::rv_u32x2 *>(nc->codes->ptr));
        } else {
            const uint64_t quads = std::max<uint64_t>(1, count / 4);
            const dim3 grid_pk(static_cast<uint32_t>(std::min<uint64_t>((quads + 255) / 256, static_cast<uint64_t>(blocks))));
            if (width == 2)
                hipLaunchKernelGGL(rvk::narrow_pack_kernel<2>, grid_pk, dim3(256), 0, ctx->stream, static_cast<const long long *>(buf.ptr), count, static_cast<long long>(nc->base), nc->codes->ptr);
            else
                hipLaunchKernelGGL(rvk::narrow_pack_kernel<4>, grid_pk, dim3(256), 0, ctx->stream, static_cast<const long long *>(buf.ptr), count, static_cast<long long>(nc->base), nc->codes->ptr);
        }
        RV_HIP(hipGetLastError());
        // queued: every later pass of this context runs behind it on the same stream
        ctx->narrow_builds += 1;
        ctx->narrow_bytes += bytes;
        (layout == rvn::Layout::kPacked ? buf.narrow_packed : buf.narrow) = std::move(nc);
        refused = false;
    } catch (const Error &e) {
        if (e.status != RV_ERR_OOM) throw;
        (void)hipGetLastError();
    }
}

// A lean one-column pass over elements [offset, offset + rows) of `buf` has finished (the host has waited for it): count it towards
// the buffer's whole scans -- in the first cover while the buffer has no companion, in the second when it has one this launch could
// not read (narrow_rule.hpp, count_pass_in) -- and build the companion the rule says the buffer is worth.
void narrow_after_pass(rv_ctx *ctx, DevBuf &buf, uint64_t offset, uint64_t rows, bool batch_counts) {
    if (ctx->opt_narrow_codes < 0 || buf.pool != ctx->pool || buf.id == 0) return;
    const rvn::LaunchKind kind{offset, batch_counts};
    buf.scan.note_pass(offset, rows);
    switch (rvn::count_pass_in(kind, buf.narrow != nullptr, buf.narrow_packed != nullptr)) {
        case rvn::CountIn::kFirst:
            if (!buf.narrow_refused && rvn::worth_building(ctx->opt_narrow_codes, buf.scan, rvt::kNarrowAfterWholeScans, rvt::kNarrowFromRows)) build(ctx, buf, kind, false);
            break;
        case rvn::CountIn::kSecond:
            if (buf.other_refused) break;
            buf.scan_other.note_extent(buf.scan.extent);
            buf.scan_other.note_pass(offset, rows);
            if (rvn::worth_building(ctx->opt_narrow_codes, buf.scan_other, rvt::kNarrowAfterWholeScans, rvt::kNarrowFromRows)) build(ctx, buf, kind, true);
            break;
        case rvn::CountIn::kNowhere: break;
    }
}

}  // namespace rvl
