// The fused filter + compact launch: shape -> instantiation, LDS and output sizing, launch, read-back, redo and overflow re-run.
// One unit of the backend library behind include/rivulus_gpu.h (gfx950 only; compiled with hipcc).  Shared helpers and the
// functions the units call across each other are declared in launch.hpp (namespace rvl).
#include "fused_rule.hpp"
#include "launch.hpp"
#include "narrow_sides.hpp"
#include "narrow_term.hpp"
#include "tile_addr.hpp"

#include <cmath>

using namespace rvh;
using namespace rvl;

namespace rvk {
// first match wins among equals, so the preferred default geometry is listed first in each table
const FusedEntry *fused_entries(size_t *n) {
    static const std::vector<FusedEntry> all = [] {
        std::vector<FusedEntry> v;
        for (auto *source : {fused_entries_lean1, fused_entries_valid1, fused_entries_multi, fused_entries_bool, fused_entries_full, fused_entries_expr,
                             fused_entries_roomy, fused_entries_narrow}) {
            size_t k = 0;
            const FusedEntry *t = source(&k);
            v.insert(v.end(), t, t + k);
        }
        return v;
    }();
    *n = all.size();
    return all.data();
}
}  // namespace rvk

namespace rvl {

// ---------------------------------------------------------------------------------------
// fused launch
// ---------------------------------------------------------------------------------------
// The staged instantiation of a launch and the geometries it walks down through are chosen by fused_rule.hpp, over every staged entry in
// one array; for one-column lean/validity launches the geometry can be steered with rv_ctx_set_option("rows_per_lane", R | waves << 8).
constexpr int kNarrowFlags = rvk::FF_NARROW16 | rvk::FF_NARROW32 | rvk::FF_PACK10;
constexpr rvf::Flags kRuleFlags = {rvk::FF_ONE_I64 | rvk::FF_ONE_F64 | rvk::FF_STAMP | rvk::FF_PROJALL | rvk::FF_NONULL | rvk::FF_EXPR | kNarrowFlags,
                                   rvk::FF_ONE_I64 | rvk::FF_ONE_F64, rvk::FF_PROJALL, rvk::FF_NONULL, rvk::FF_SEL, kNarrowFlags, rvk::FF_PACK10};
static rvf::Table<rvk::FusedEntry> staged_table() {
    size_t n = 0;
    const rvk::FusedEntry *t = rvk::fused_entries(&n);
    return {t, n};
}
// (costs several microseconds: once per (kernel, LDS size) and context)
static void enable_lds(rv_ctx *ctx, const void *fn, size_t lds) {
    size_t &enabled = ctx->lds_enabled[fn];
    if (lds > enabled) {
        RV_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
        enabled = lds;
    }
}

// Selectivity of the lowered predicate `in` over a strided sample of its rows; -1 when the sample could not be taken.
double sample_selectivity(rv_ctx *ctx, const rvk::ScanInputs &in, int nvals) {
    constexpr uint32_t kBlocks = 1024, kBlockRows = 1024;
    const rvk::SampleFn fn = rvk::sample_kernel(nvals);
    if (!fn || in.n < static_cast<uint64_t>(kBlocks) * kBlockRows) return -1.0;
    if (!ctx->d_sample) {
        void *d = nullptr, *h = nullptr;
        constexpr size_t kBytes = rvk::kSampleWords * 8;
        if (hipMalloc(&d, kBytes) != hipSuccess || hipHostMalloc(&h, kBytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            if (d) (void)hipFree(d);
            return -1.0;
        }
        RV_HIP(hipMemset(d, 0, kBytes));
        std::memset(h, 0, kBytes);
        ctx->d_sample = static_cast<unsigned long long *>(d);
        ctx->h_sample = static_cast<volatile unsigned long long *>(h);
    }
    rvk::SampleParams sp{};
    sp.in = in;
    sp.stride = (in.n / kBlocks) & ~uint64_t(63);
    sp.dev_words = ctx->d_sample;
    sp.host_words = ctx->h_sample;
    sp.sequence = ++ctx->sample_seq;
    hipLaunchKernelGGL(fn, dim3(kBlocks), dim3(256), 0, ctx->stream, sp);
    RV_HIP(hipGetLastError());
    // the last workgroup writes {survivors, sequence} into pinned memory: spin on it; after 2 ms fall back to draining the stream
    const auto t0 = std::chrono::steady_clock::now();
    while (ctx->h_sample[1] != sp.sequence) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
            RV_HIP(hipStreamSynchronize(ctx->stream));
            break;
        }
    }
    if (ctx->h_sample[1] != sp.sequence) return -1.0;
    ctx->samples_taken += 1;
    for (int b = 0; b < rvk::kSampleBuckets; ++b)
        ctx->last_sample_hist[b] = static_cast<float>((ctx->h_sample[2 + b / 4] >> (16 * (b % 4))) & 0xFFFF) / static_cast<float>(kBlocks);
    static_assert(kBlocks == rvk::kSampleBlocks, "sample geometry");
    for (uint32_t b = 0; b < kBlocks; ++b)
        ctx->last_sample_profile[b] = static_cast<uint16_t>((ctx->h_sample[2 + rvk::kSampleHistWords + b / 4] >> (16 * (b % 4))) & 0xFFFF);
    ctx->last_sample_stride = sp.stride;
    ctx->last_sample_rows = in.n;
    uint64_t sampled = 0;  // rows the blocks covered (the last ones may be cut by the table's end)
    for (uint32_t b = 0; b < kBlocks; ++b) {
        const uint64_t first = static_cast<uint64_t>(b) * sp.stride;
        sampled += first >= in.n ? 0 : std::min<uint64_t>(kBlockRows, in.n - first);
    }
    return sampled ? static_cast<double>(ctx->h_sample[0]) / static_cast<double>(sampled) : -1.0;
}

// the last sample's histogram and profile travel with the predicate's memory
static void keep_sample(rv_ctx *ctx, rv_ctx::SeenPredicate *q) {
    std::copy(ctx->last_sample_hist, ctx->last_sample_hist + 16, q->hist);
    q->have_hist = true;
    std::copy(ctx->last_sample_profile, ctx->last_sample_profile + 1024, q->profile);
    q->profile_stride = ctx->last_sample_stride;
    q->profile_rows = ctx->last_sample_rows;
}

// rows the outputs of a pass over n rows are sized for (option "out_sizing")
// `expected`: the selectivity this predicate is known to have over these buffers (its last pass, or the strided sample of a first
// call); < 0: unknown
uint64_t output_capacity(rv_ctx *ctx, uint64_t n, double expected) {
    if (ctx->opt_out_sizing == 1 && ctx->last_selectivity >= 0.0)
        return std::min<uint64_t>(n, static_cast<uint64_t>(static_cast<double>(n) * (ctx->last_selectivity * 1.5 + 0.01)) + 1024);
    if (ctx->opt_out_sizing >= 2)
        return std::min<uint64_t>(n, static_cast<uint64_t>(static_cast<double>(n) * static_cast<double>(ctx->opt_out_sizing) * 1e-6) + 1024);
    // Default: big tables (the ones whose first call is sampled: 2^25 rows, 256 MiB per output column) get outputs for what the predicate
    // is known to keep x 1.2 + 2 % of the rows (the sample's 1024 blocks of a table whose survivors come in runs of 1e5 rows are off by
    // 1 % of the rows, one sigma) -- BASELINE configs[1] then holds 8 + 1.3 GB instead of 8 + 8, configs[3] at G = 1 fits one GPU without
    // an option.  A pass that keeps more counts exactly and is re-run once with outputs of that size (fused_finish).  Small tables and
    // predicates nobody has seen keep outputs for every row: nothing to save, nothing to re-run.
    if (ctx->opt_out_sizing == 0 && expected >= 0.0 && n >= rvt::kOutSizingFromRows)
        return std::min<uint64_t>(n, static_cast<uint64_t>(static_cast<double>(n) * (expected * rvt::kOutSizingFactor + rvt::kOutSizingSlack)) + 4096);
    return n;
}

// Signature of a predicate: the key of the selectivity a launch is sized from (FNV-1a over what decides a row's fate).
uint64_t predicate_signature(const rv_dcolumn *const *cols, uint32_t ncols, const rv_term *terms, uint32_t nterms, rv_null_policy policy, const ExprInfo *ex) {
    uint64_t signature = 0xcbf29ce484222325ull;
    auto mix = [&](uint64_t v) {
        for (int b = 0; b < 8; ++b) signature = (signature ^ ((v >> (8 * b)) & 0xFF)) * 0x100000001b3ull;
    };
    mix(nterms);
    mix(static_cast<uint64_t>(policy));
    for (uint32_t t = 0; t < nterms; ++t) {
        const rv_dcolumn *tc = terms[t].column < ncols ? cols[terms[t].column] : nullptr;
        mix(tc ? static_cast<uint64_t>(tc->dtype) : ~0ull);
        mix(terms[t].column);
        mix(static_cast<uint64_t>(terms[t].op));
        mix(static_cast<uint64_t>(terms[t].lit_type));
        // WHICH data the term reads: the column's buffer (a stream's windows are slices of one table: offset and length stay out of
        // it), or, for a term rewritten to `mask is true`, what the mask stood for (predicate.hip, term_identity) -- so the same
        // predicate text over another table, or another String literal over the same one, is another predicate
        if (terms[t].op == RV_IS_TRUE && terms[t].lit.i != 0) mix(static_cast<uint64_t>(terms[t].lit.i));
        else {
            mix(tc && tc->values ? (tc->values->id ? tc->values->id : reinterpret_cast<uint64_t>(tc->values->ptr)) : 0ull);
            mix(terms[t].lit_type == RV_STRING || terms[t].lit_type == RV_NULL ? 0ull : static_cast<uint64_t>(terms[t].lit.i));
        }
    }
    if (ex) {
        mix(ex->negate_result ? 3 : 2);
        for (size_t t = 0; t < ex->negate.size(); ++t) mix(static_cast<uint64_t>(ex->negate[t]) | (static_cast<uint64_t>(ex->group_end[t]) << 8));
    }
    return signature;
}

// Wave ranges whose survivors outgrew their LDS slot (runs of survivors: clustered or sorted data): re-read, range by range, by
// the generic kernel at their reserved output offsets -- one wave per listed range, nothing shared (fused_kernel.hpp).
static void launch_redo(rv_ctx *ctx, FusedLaunch &L) {
    const int rr = L.nvals ? rvk::redo_rows_per_lane(L.nvals, L.range_rows) : 4;
    const rvk::RedoFn redo = rvk::redo_kernel(L.nvals, rr);
    require(redo != nullptr && L.nranges > 0, RV_ERR_INTERNAL, "no redo kernel variant");
    const size_t redo_lds = rvk::kLdsHeader + static_cast<size_t>(rvk::kRedoWaves) * (std::max(L.nvals, 1) + rvk::kMaxBitStreams) * 64 * rr;
    const uint64_t want = (L.nranges + rvk::kRedoWaves - 1) / rvk::kRedoWaves;
    const uint32_t rgrid = static_cast<uint32_t>(std::min<uint64_t>(want, static_cast<uint64_t>(ctx->props.multiProcessorCount) * 8));
    hipLaunchKernelGGL(redo, dim3(rgrid), dim3(rvk::kRedoWaves * 64), redo_lds, ctx->stream, L.p, L.range_rows, L.nranges);
    RV_HIP(hipGetLastError());
}

struct Bound {
    const rv_dcolumn *const *cols;
    rvk::ScanInputs *in;
    std::vector<int> value_slot, bool_slot;  // per batch column: its slot, or -1
    std::vector<char> never_null;            // per batch column: no null among the survivors (its output needs no bitmap)
    int nvals = 0, nbools = 0, npred = 0;  // value slots [0, npred): the 8-byte columns the terms read (the direct kernel loads them first)

    int add_value(const rv_dcolumn *col) {  // a slot of its own
        require(nvals < rvk::kMaxValueCols, RV_ERR_UNSUPPORTED, "too many 8-byte columns for one pass");
        in->cols[nvals] = dev_view(col);
        return nvals++;
    }
    int value_of(uint32_t c) {
        if (value_slot[c] < 0) value_slot[c] = add_value(cols[c]);
        return value_slot[c];
    }
    int bool_of(uint32_t c) {
        if (bool_slot[c] < 0) {
            require(nbools < rvk::kMaxBoolCols, RV_ERR_UNSUPPORTED, "too many Boolean predicate columns for one pass");
            bool_slot[c] = nbools;
            in->bcols[nbools++] = dev_view(cols[c]);
        }
        return bool_slot[c];
    }
};

// The predicate's columns bound to slots of `in` and its terms lowered there.
static Bound bind_inputs(const rv_dcolumn *const *cols, uint32_t ncols, const rv_term *terms, uint32_t nterms, rv_null_policy policy,
                         const ExprInfo *ex, rvk::ScanInputs &in) {
    require(nterms >= 1 && nterms <= static_cast<uint32_t>(rvk::kMaxTerms), RV_ERR_UNSUPPORTED,
            fmt("predicate needs 1..%d terms, got %u", rvk::kMaxTerms, nterms));
    Bound b{cols, &in, std::vector<int>(ncols, -1), std::vector<int>(ncols, -1), std::vector<char>(ncols, 0)};
    in.n = ncols ? cols[0]->length : 0;
    in.nterms = static_cast<int32_t>(nterms);
    for (uint32_t t = 0; t < nterms; ++t) {
        const uint32_t c = terms[t].column;
        require(c < ncols, RV_ERR_INVALID_ARG, fmt("term %u references column %u of %u", t, c, ncols));
        const rv_dtype ct = cols[c]->dtype;
        require(is_value_type(ct) || ct == RV_BOOLEAN, RV_ERR_UNSUPPORTED,
                "predicate columns must be Int64, Float64 or Boolean on the device path");
        const int slot = ct == RV_BOOLEAN ? b.bool_of(c) : b.value_of(c);
        in.terms[t] = lower_term(terms[t], ct, policy, static_cast<uint32_t>(slot));
        if (ex) in.terms[t].set_literal(ex->negate[t] != 0, ex->group_end[t] != 0);
    }
    b.npred = b.nvals;

    // a nullable column tested by a term that drops its null rows has no null among the survivors: its output
    // needs no bitmap (and the builder would drop it anyway, primitive.rs:179-185)
    if (!ex) {
        for (uint32_t t = 0; t < nterms; ++t)
            if (is_value_type(cols[terms[t].column]->dtype) && !in.terms[t].null_v()) b.never_null[terms[t].column] = 1;
    } else {
        // OR / NOT: only strict propagation (RV_NULL_DROPS) guarantees it, and then for every column the expression reads
        in.expr_mode = 1;
        in.negate_result = ex->negate_result ? 1 : 0;
        if (ex->strict) {
            for (uint32_t c : ex->strict_cols) {
                require(c < ncols, RV_ERR_INTERNAL, "strict column out of range");
                if (is_value_type(cols[c]->dtype)) {
                    b.never_null[c] = 1;
                    if (cols[c]->validity) in.strict_values |= 1u << b.value_of(c);
                } else if (cols[c]->dtype == RV_BOOLEAN && cols[c]->validity) {
                    in.strict_bools |= 1u << b.bool_of(c);  // (its literals may have been simplified away: still read for its nulls)
                }
            }
        }
    }
    return b;
}

// A predicate this context has not run over this data: its selectivity from a strided sample (agg_kernel.hpp,
// sample_count_kernel; ~10 us of device time, one launch, the host spins on a pinned word), so that the FIRST launch is already
// sized for it -- the reference's operators have no warm-up call (stream.rs:136-158), and a one-shot collect() is always
// the first call.  Not for small tables: below 2^25 rows a pass is a few tens of microseconds, and a mis-sized one costs less
// than the sample.  The sample's histogram and profile travel with the predicate's memory (the pass will store its true selectivity).
// < 0: no sample taken.
static double first_call_sample(rv_ctx *ctx, const rvk::ScanInputs &in, int nvals, uint64_t signature) {
    if (ctx->opt_sample < 0 || in.n < (ctx->opt_sample > 0 ? static_cast<uint64_t>(ctx->opt_sample) : rvt::kSampleFromRows)) return -1.0;
    const double s = sample_selectivity(ctx, in, nvals);
    if (s >= 0.0) keep_sample(ctx, ctx->remember_selectivity(signature, s));
    return s;
}

// Every projected column bound to a value slot or to bit streams, its output handle created (in out[] at once: the callers free it on
// an error); alloc_outputs gives it buffers.  Returns the bytes a row of the outputs takes in an LDS slot.
static size_t bind_outputs(Bound &b, uint32_t ncols, const uint32_t *proj, uint32_t nproj, rv_dcolumn **out, FusedLaunch &L) {
    rvk::FusedParams &p = L.p;
    L.outs.assign(nproj, OutCol{});
    size_t row_bytes = 0;
    uint32_t projected = 0;  // value slots an output already writes
    int nxs = 0;
    for (uint32_t j = 0; j < nproj; ++j) {
        const uint32_t c = proj[j];
        require(c < ncols, RV_ERR_INVALID_ARG, fmt("projection %u references column %u of %u", j, c, ncols));
        const rv_dcolumn *src = b.cols[c];
        OutCol &o = L.outs[j];
        o.col = out[j] = new rv_dcolumn();
        o.col->dtype = src->dtype;
        if (is_value_type(src->dtype)) {
            // the same source column projected twice shares nothing: give it its own slot view
            const int slot = b.value_slot[c];
            o.value_slot = slot >= 0 && (projected >> slot & 1u) ? b.add_value(src) : b.value_of(c);
            projected |= 1u << o.value_slot;
            o.validity = src->validity && !b.never_null[c];
            row_bytes += o.validity ? 9 : 8;
        } else if (src->dtype == RV_BOOLEAN) {
            require(nxs + (src->validity ? 2 : 1) <= rvk::kMaxBitStreams, RV_ERR_UNSUPPORTED,
                    "too many Boolean columns for one pass");
            rvk::BitStream &bs = p.xs[nxs];
            bs.src = static_cast<const uint8_t *>(src->values->ptr);
            bs.src_bytes = src->values->bytes;
            bs.mask = src->validity ? static_cast<const uint8_t *>(src->validity->ptr) : nullptr;
            bs.mask_bytes = src->validity ? src->validity->bytes : 0;
            bs.offset = src->offset;
            o.xs_values = nxs++;
            row_bytes += src->validity ? 2 : 1;
            if (src->validity) {
                rvk::BitStream &vs = p.xs[nxs];
                vs.src = static_cast<const uint8_t *>(src->validity->ptr);
                vs.src_bytes = src->validity->bytes;
                vs.offset = src->offset;
                o.xs_valid = nxs++;
            }
        } else {
            throw Error(RV_ERR_UNSUPPORTED, "only Int64, Float64 and Boolean columns are compacted on the device path");
        }
    }
    p.nxs = nxs;
    return row_bytes;
}

// Buffers of every output of L for `cap` rows, bitmaps zeroed on the stream (kernels OR their edge words into them).  A stretch's
// values land in the caller's buffers from row place_base on (out_bias rows before it: the pointers are rounded down to a 128-byte line).
// The pass's outputs (fused_begin) and those of its re-run after an output overflow (fused_finish).
static void alloc_outputs(rv_ctx *ctx, FusedLaunch &L, uint64_t cap) {
    rvk::FusedParams &p = L.p;
    p.out_capacity = cap;
    const size_t wb = zeroed_bitmap_bytes(cap);
    auto zeroed_bitmap = [&](DevBufRef &buf) {
        buf = pool_alloc(ctx, wb);
        RV_HIP(hipMemsetAsync(buf->ptr, 0, wb, ctx->stream));
        return static_cast<uint64_t *>(buf->ptr);
    };
    for (size_t j = 0; j < L.outs.size(); ++j) {
        const OutCol &o = L.outs[j];
        if (o.value_slot >= 0) {
            if (L.place) {
                o.col->values = (*L.place)[j];
                p.out_values[o.value_slot] = static_cast<uint64_t *>(o.col->values->ptr) + (L.place_base - L.out_bias);
            } else {
                o.col->values = pool_alloc(ctx, std::max<size_t>(elem_bytes(o.col->dtype, cap), 8));
                p.out_values[o.value_slot] = static_cast<uint64_t *>(o.col->values->ptr);
            }
            if (o.validity) p.out_validity[o.value_slot] = zeroed_bitmap(o.col->validity);
        } else {
            p.xs[o.xs_values].out = zeroed_bitmap(o.col->values);
            if (o.xs_valid >= 0) p.xs[o.xs_valid].out = zeroed_bitmap(o.col->validity);
        }
    }
}

// The selection bitmap of L's pass, in *sel_out at once.
static void make_selection(rv_ctx *ctx, FusedLaunch &L, rv_dcolumn **sel_out) {
    auto *sel = new rv_dcolumn();
    *sel_out = sel;
    sel->dtype = RV_BOOLEAN;
    sel->length = L.p.in.n;
    sel->null_count = 0;
    sel->values = pool_alloc(ctx, std::max<size_t>(bitmap_words_bytes(L.p.in.n), 8));
    L.p.out_selection = static_cast<uint64_t *>(sel->values->ptr);
}

// What the launch will be.  Decided before anything is allocated or queued for it.
struct LaunchChoice {
    const rvk::FusedEntry *staged = nullptr;   // the staged pass's instantiation, last tried
    const rvk::DirectEntry *direct = nullptr;  // the direct kernel's (runs instead when set)
    int r = 0, vec = 1, waves = 0, flags = 0;  // of the kernel that runs
    void (*fn)(const rvk::FusedParams) = nullptr;
    int need = 0;
    size_t stages = 3, lds = 0, stage_row_bytes = 0;
    size_t lds_plain = 0;  // a pass over codes: what its plain twin needs for the same slots (the re-run after an output overflow)
    size_t stages_plain = 3;  // ... and the stages it runs them with (two behind a three-stage pass over packed codes: size_staged)
    uint32_t cap = 0, ntiles = 0;
    uint64_t tile_rows = 0;
    bool make_selection = false;  // the selection bitmap deferred for per-batch counts is wanted after all (the pass cannot count them)
    const NarrowCodes *narrow = nullptr;  // the pass reads these codes instead of the column's 8-byte values (FF_NARROW16 / FF_NARROW32)
    double redo_expected = 0.0;   // share of the staged pass's wave ranges expected to outgrow their slots
};

// per-batch counts out of the pass: a batch must be a whole number of the geometry's wave ranges (64 x rows per lane)
static bool counts_in_pass(const BatchReq *req, int r) { return req && req->counts && rvf::whole_ranges(req->chunk_rows, r); }
// The direct kernel's LDS bytes: one slot per wave, its rows of every loaded column (+ a validity byte per row for each of the nv_out
// columns with an output bitmap).
static size_t direct_lds(const rvk::DirectEntry &g, int nvals, int nv_out) { return static_cast<size_t>(g.waves) * 64 * g.r * (8 * static_cast<size_t>(nvals) + nv_out); }

// The direct instantiation for this launch's columns and features, or none.
static const rvk::DirectEntry *find_direct(rv_ctx *ctx, const Bound &b, int nv_out, double seen, const BatchReq *req, const RangeOffsets *ranges) {
    const rvk::DirectEntry *found = nullptr;
    const int npred = b.npred, nvals = b.nvals;
    int dflags = b.nbools ? (rvk::FF_VALIDITY | rvk::FF_BOOL) : 0;
    if (ctx->opt_stamp) dflags |= rvk::FF_STAMP;  // diagnostic instantiations (phase cycle sums), a few geometries only
    for (int s = 0; s < npred; ++s)
        if (b.in->cols[s].validity) dflags |= rvk::FF_VALIDITY;
    if (nv_out) dflags |= rvk::FF_VALIDITY | rvk::FF_OUTVALID;
    // the first listed instantiation that covers the inputs' features (listed leanest first) -- among those whose wave
    // ranges serve the caller's side outputs, when it asks for any: wave offsets need a range that tiles 4096 rows, per-batch
    // counts a batch that is a whole number of ranges
    const rvk::DirectEntry *fallback = nullptr;
    bool tall_tried = false;
    constexpr size_t kDirectLdsBudget = (160 * 1024) / 2 - 512;
    for (int t = 0; t < 2 && !found; ++t) {
        size_t cnt = 0;
        const rvk::DirectEntry *tab = t ? rvk::direct_entries_b(&cnt) : rvk::direct_entries_a(&cnt);
        for (size_t i = 0; i < cnt && !found; ++i) {
            const rvk::DirectEntry &g = tab[i];
            if (g.np != npred || g.nq != nvals - npred || (g.flags & dflags) != dflags || ((g.flags ^ dflags) & rvk::FF_STAMP) != 0) continue;
            if (ctx->opt_direct_r > 0 || ctx->opt_direct_waves > 0) {  // diagnostic: a named geometry or none
                if ((ctx->opt_direct_r <= 0 || g.r == ctx->opt_direct_r) && (ctx->opt_direct_waves <= 0 || g.waves == ctx->opt_direct_waves)) found = &g;
                continue;
            }
            if (g.waves != 8 || direct_lds(g, nvals, nv_out) > kDirectLdsBudget) continue;  // two workgroups per CU have to fit
            const bool serves = (!ranges || 4096u % (64u * static_cast<uint32_t>(g.r)) == 0) && (!(req && req->counts) || counts_in_pass(req, g.r));
            // one loaded column while fewer than kDirectTallBelow survive (a table of runs at 30-50 %, a selection just past
            // kDirectFromOneColumn): the 16-row geometry -- what the launch keeps in registers and LDS behind a tile's aggregate
            // covers the chain's latency only at the rate that storage / latency gives, and below ~70 % that, not HBM, is the bound
            if (serves && npred == 1 && nvals == 1 && !nv_out && seen >= 0.0 && seen < rvt::kDirectTallBelow && g.r != 16 && !tall_tried) {
                tall_tried = true;
                for (size_t k = i + 1; k < cnt; ++k)
                    if (tab[k].np == 1 && tab[k].nq == 0 && tab[k].r == 16 && tab[k].waves == 8 && tab[k].flags == g.flags && direct_lds(tab[k], nvals, nv_out) <= kDirectLdsBudget &&
                        (!(req && req->counts) || counts_in_pass(req, 16))) {
                        found = &tab[k];
                        break;
                    }
                if (found) break;
            }
            if (serves) found = &g;
            else if (!fallback) fallback = &g;
        }
    }
    if (!found && ctx->opt_direct_r <= 0 && ctx->opt_direct_waves <= 0) found = fallback;
    return found;
}

// The direct kernel for the launch, when an instantiation serves it (find_direct), with its tiles and LDS (direct_lds).  A staged
// geometry's cap and stage_row_bytes stay.
static bool use_direct(rv_ctx *ctx, LaunchChoice &c, const Bound &b, int nv_out, double seen, const BatchReq *req, const RangeOffsets *ranges,
                       bool sel_deferred) {
    const rvk::DirectEntry *d = find_direct(ctx, b, nv_out, seen, req, ranges);
    if (!d) return false;
    c.direct = d;
    // per-batch counts out of the pass need a batch to be a whole number of the geometry's wave ranges: else the caller counts
    // the selection bitmap, which the kernel writes on the way
    if (sel_deferred && !counts_in_pass(req, d->r)) c.make_selection = true;
    c.tile_rows = static_cast<uint64_t>(d->waves) * 64 * d->r;
    const uint64_t ntiles64 = (b.in->n + c.tile_rows - 1) / c.tile_rows;
    require(ntiles64 < (1ull << 31) - 1, RV_ERR_UNSUPPORTED, "batch too large for one launch");
    c.ntiles = static_cast<uint32_t>(ntiles64);
    c.stages = 2;
    c.lds = direct_lds(*d, b.nvals, nv_out);
    return true;
}

// The staged instantiation e's tiles, stages, LDS slot capacity and LDS bytes.  `row_bytes`: what a row of the outputs takes in a slot.
static void size_staged(rv_ctx *ctx, LaunchChoice &c, const rvk::FusedEntry &e, uint64_t n, int nvals, int nxs, size_t row_bytes, bool dense_sizing) {
    c.stage_row_bytes = row_bytes;
    if (e.flags & rvk::FF_PROJALL)  // the kernel stages a validity byte for every column when any has a bitmap
        c.stage_row_bytes = static_cast<size_t>(nvals) * (((e.flags & rvk::FF_VALIDITY) && !(e.flags & rvk::FF_NONULL)) ? 9 : 8) + static_cast<size_t>(nxs);
    c.tile_rows = static_cast<uint64_t>(e.waves) * 64 * e.r;
    const uint64_t ntiles64 = (n + c.tile_rows - 1) / c.tile_rows;
    require(ntiles64 < (1ull << 31), RV_ERR_UNSUPPORTED, "batch too large for one launch");
    c.ntiles = static_cast<uint32_t>(ntiles64);

    // LDS: every wave owns two slots (double buffered for the deferred look-back) of cap rows.
    // One 1024-thread workgroup per CU may use most of the 160 KiB; 512-thread variants keep to
    // half so that two workgroups fit.
    const uint32_t rows_per_wave = 64u * static_cast<uint32_t>(e.r);
    // 16 waves x 4 per SIMD is one workgroup per CU (128 VGPRs each): it may use most of the LDS; smaller workgroups run
    // two per CU -- unless sized for a dense selection: one workgroup per CU whatever its size, two stages
    const bool roomy = dense_sizing || ctx->opt_roomy != 0;
    const size_t budget = (roomy || e.waves >= 16) ? 144 * 1024 : 72 * 1024;
    // Three stages (write-out two iterations after the aggregate went out, so the scanner's prefix is
    // there when it is needed) when a slot still holds 3/16 of a wave's rows; two otherwise.
    // (a pass over PACKED codes sizes its three stages of slots as the plain form sizes TWO: its re-run after an output overflow, the
    // plain instantiation of its geometry over the 8-byte values, then runs two-staged in the same slots -- the rare second pass pays the
    // exposed look-back, and the pass itself keeps three stages at 48 rows per lane, where a slot sized for three plain stages holds
    // 384 of a wave's 3072 rows, less than the 3/16 below; with two stages it took 0.57 ms against 0.47 ms of the pass over 2-byte
    // codes, profiles/narrow4_steps.txt)
    const bool packed = (e.flags & rvk::FF_PACK10) != 0;
    auto cap_for = [&](size_t st) -> uint32_t {
        if (!c.stage_row_bytes) return rows_per_wave;
        if (packed && st == 3) st = 2;
        return static_cast<uint32_t>(std::min<uint64_t>(rows_per_wave, (budget / (st * e.waves * c.stage_row_bytes)) & ~size_t(63)));
    };
    c.stages = 3;
    if (ctx->opt_depth == 1 || (ctx->opt_depth == 0 && (roomy || cap_for(3) * 16 < rows_per_wave * 3))) c.stages = 2;
    c.cap = cap_for(c.stages);
    if (ctx->opt_cap_rows > 0) c.cap = static_cast<uint32_t>(std::min<int64_t>(c.cap, std::max<int64_t>(64, ctx->opt_cap_rows & ~int64_t(63))));
    c.cap = std::max<uint32_t>(c.cap, 64u * static_cast<uint32_t>(e.vec));  // a slot holds at least one chunk
    require(c.cap >= 64, RV_ERR_INTERNAL, "LDS stage too small");
    // bit streams of a lane-form launch are staged as R + 1 words of bits, whatever the slot's row capacity
    // (a pass over codes stages the survivors' codes: `cap` is sized above from the 8 bytes of a row's value, like the plain form's
    // -- the redo rule, its memory and the walk through the geometries see the same slots -- and only the bytes of the launch shrink)
    const size_t code_bytes = (e.flags & rvk::FF_NARROW16) ? 2 : ((e.flags & rvk::FF_NARROW32) ? 4 : 0);
    auto lds_at = [&](size_t st, uint32_t rows, size_t row_bytes_staged) {
        const size_t xs_words = (e.vec == 1 && rows < (static_cast<uint32_t>(e.r) + 2) * 8u) ? static_cast<size_t>(nxs) * ((e.r + 2) * 8 - rows) : 0;
        const size_t slot = (static_cast<size_t>(rows) * row_bytes_staged + xs_words + 15) & ~size_t(15);
        return rvk::kLdsHeader + st * e.waves * slot + static_cast<size_t>(e.waves) * rvk::kLdsDumpBytes;
    };
    auto lds_for = [&](size_t st, uint32_t rows) { return lds_at(st, rows, c.stage_row_bytes); };
    // the minimum slot of a wide row (several columns with validity bytes) times three stages can pass the CU's 160 KiB
    // (a forced "depth" = 2 on such a shape): two stages then
    constexpr size_t kLdsPerCu = 160 * 1024;
    // (the plain twin of a pass over packed codes never runs three stages: see cap_for)
    auto plain_stages = [&](size_t st) { return (packed && st == 3) ? size_t(2) : st; };
    if (c.stages == 3 && lds_for(plain_stages(3), c.cap) > kLdsPerCu) c.stages = 2;
    require(lds_for(plain_stages(c.stages), c.cap) <= kLdsPerCu, RV_ERR_UNSUPPORTED,
            fmt("fused pass: %zu bytes of LDS for %d columns at %u rows per slot", lds_for(plain_stages(c.stages), c.cap), nvals, c.cap));
    c.stages_plain = plain_stages(c.stages);
    c.lds = c.lds_plain = lds_for(c.stages_plain, c.cap);
    if (code_bytes && c.stage_row_bytes == 8) c.lds = lds_at(c.stages, c.cap, code_bytes);
    // (a pass over packed codes: one spare 2-byte cell behind every slot's `cap`, rvk::kPackedSpareBytes, 16 bytes after rounding -- what
    //  its whole-tile staging's one clamp per pair may write in a wave that outgrew its slot, fused_kernel.hpp.  `cap`, the plain twin's
    //  slots and lds_plain stay)
    if (packed && code_bytes && c.stage_row_bytes == 8)
        c.lds = rvk::kLdsHeader + c.stages * e.waves * ((static_cast<size_t>(c.cap) * code_bytes + rvk::kPackedSpareBytes + 15) & ~size_t(15)) + static_cast<size_t>(e.waves) * rvk::kLdsDumpBytes;
}

// Survivors that come in RUNS (a table sorted or clustered on the predicate's column: ids, timestamps): a wave of the staged
// pass whose 64 R rows hold more of them than its LDS slot leaves its range to the redo kernel (fused_kernel.hpp,
// fused_redo_waves) -- cheap while few ranges do, but past a point the direct kernel, whose rows wait in registers whatever
// survives, is ahead.  The share of ranges to expect: what the last staged pass of this predicate over these buffers left
// to the redo kernel, or -- on a first call -- the share of the sample's 1024-row blocks denser than the slot.
static double redo_estimate(rv_ctx *ctx, const FusedLaunch &L, double seen, bool sampled_now, uint32_t cap_rows, uint32_t rows_per_wave) {
    const rv_ctx::SeenPredicate *q = L.place ? nullptr : ctx->seen_entry(L.signature);
    if (cap_rows >= rows_per_wave) return 0.0;
    const double ratio = static_cast<double>(cap_rows) / rows_per_wave, width = 1.0 / rvk::kSampleBuckets;
    // measured by a staged pass whose slots held at least this share of a wave's rows (roomier slots than it had: unknown -- independent
    // rows stop outgrowing them, runs do not)
    if (q && q->redo_fraction >= 0.0 && std::fabs(q->redo_at - seen) < rvt::kRedoMemorySelectivityBand && ratio <= q->redo_ratio + rvt::kRedoMemorySlotBand) return q->redo_fraction;
    const float *hist = sampled_now ? ctx->last_sample_hist : ((q && q->have_hist) ? q->hist : nullptr);
    if (!hist) return 0.0;
    double f = 0.0;
    for (int b = 0; b < rvk::kSampleBuckets; ++b) {
        const double lo = b * width, hi = lo + width;
        if (lo >= ratio) f += hist[b];
        else if (hi > ratio) f += hist[b] * (hi - ratio) / width;
    }
    return f;
}

// The kernel and geometry of L's pass: the project's policy, read from the bound shape, the selectivity the pass is sized by (`seen`;
// `sampled_now`: out of a sample this call took), the caller's side outputs and the context's options and predicate memory.  Allocates
// nothing, queues nothing, writes nothing of the context.  `row_bytes`: what a row of the outputs takes in an LDS slot (bind_outputs).
static LaunchChoice choose_launch(rv_ctx *ctx, const FusedLaunch &L, const Bound &b, size_t row_bytes, bool expr, bool sel_deferred, double seen,
                                  bool sampled_now, const BatchReq *req, const RangeOffsets *ranges, const NarrowCodes *narrow) {
    const rvk::FusedParams &p = L.p;
    const int nvals = b.nvals, npred = b.npred, nxs = p.nxs;
    const uint64_t n = p.in.n;
    LaunchChoice c;
    // 16-byte loads need every loaded 8-byte column to start 16-byte aligned
    int vec = ctx->opt_vec == 1 ? 1 : (ctx->opt_vec == 2 ? 2 : (nvals <= 3 ? 2 : 1));
    for (int s = 0; s < nvals; ++s) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p.in.cols[s].values) + p.in.cols[s].offset * 8;
        if (a & 15) vec = 1;
    }
    for (int s = 0; s < nvals; ++s)
        if (p.in.cols[s].validity) c.need |= rvk::FF_VALIDITY;
    if (b.nbools) c.need |= rvk::FF_BOOL;
    // shapes that read bit buffers (null bitmaps, Boolean columns) or evaluate an expression run in lane form with 8-byte
    // loads: measured faster than 16-byte loads + per-slot mask arrays on every such shape (profiles/README.md)
    if (ctx->opt_vec == 0 && (c.need || expr)) vec = 1;
    if (nxs) c.need |= rvk::FF_XS;
    if (p.out_selection) c.need |= rvk::FF_SEL;
    if (expr) c.need |= rvk::FF_EXPR;
    // predicate shape: one compare term on the only loaded column, no nulls -> single-pass fast path
    if (!expr && (c.need & ~rvk::FF_SEL) == 0 && nvals == 1 && p.in.nterms == 1 && !p.in.terms[0].is_bool() && p.in.terms[0].code() != rvk::TC_CONST)
        c.need |= p.in.terms[0].is_float() ? rvk::FF_ONE_F64 : rvk::FF_ONE_I64;
    // the lean Int64 form over a column whose buffer has a narrow companion (narrow.hip: built, covering this view, first element even)
    // reads the codes: the default row mapping only (16-byte loads).  A forced geometry ("rows_per_lane") or a diagnostic ("stamp",
    // "debug") takes the codes only in a context that packs on request ("narrow_codes" = 1: tools/narrow_stamp.py; the older tools
    // keep measuring the plain kernel) AND where the narrow table holds EXACTLY that instantiation -- the geometry asked for, with
    // FF_STAMP for a diagnostic (2-byte codes at 32 and 16 rows per lane, packed ones at 48 and 24, fused_narrow.hip).  Otherwise the
    // launch reads the 8-byte values as it always did: a forced geometry is never swapped for another one (include/rivulus_gpu.h,
    // "narrow_codes").  A packed companion (narrow.hip hands one out only to a launch without per-batch counts whose view starts on a
    // super-group) sets FF_PACK10 beside FF_NARROW16: the cells the pass stages are 2-byte codes whatever their layout in memory
    const bool diag = ctx->opt_stamp || ctx->opt_debug;
    if (narrow && c.need == rvk::FF_ONE_I64 && vec == 2 && !L.place && ((ctx->opt_rows_per_lane <= 0 && !diag) || ctx->opt_narrow_codes > 0)) {
        const int codes = narrow->layout == rvn::Layout::kPacked ? (rvk::FF_NARROW16 | rvk::FF_PACK10) : (narrow->code_bytes == 2 ? rvk::FF_NARROW16 : rvk::FF_NARROW32);
        if (rvf::holds_exactly(staged_table(), c.need | codes | (diag ? rvk::FF_STAMP : 0), ctx->opt_rows_per_lane)) c.need |= codes;
    }
    // diagnostics (per-phase stamps, ablations) exist in the FF_STAMP instantiations only; "debug" implies them
    if (diag && ((c.need & ~kNarrowFlags) == rvk::FF_ONE_I64 || (nvals == 2 && c.need == rvk::FF_VALIDITY))) c.need |= rvk::FF_STAMP;
    // every loaded column projected, output bitmap exactly where there is an input bitmap?
    // ... or no output bitmap at all (FF_NONULL: every nullable column is tested by a null-dropping term)
    int projected = 0, nv_out = 0;  // loaded columns projected; ... whose output keeps a bitmap
    for (int s = 0; s < nvals; ++s) {
        projected += p.out_values[s] != nullptr;
        nv_out += p.out_validity[s] != nullptr;
    }
    const bool all_proj = nvals > 0 && !(c.need & (rvk::FF_ONE_I64 | rvk::FF_ONE_F64)) && projected == nvals;
    bool mirror = all_proj;
    for (int s = 0; s < nvals; ++s) mirror = mirror && ((p.out_validity[s] != nullptr) == (p.in.cols[s].validity != nullptr));
    const bool none = all_proj && nv_out == 0;
    // not every loaded column projected, but no output bitmap anywhere: the staging needs no validity select either
    const bool no_out_validity = nvals > 0 && (c.need & rvk::FF_VALIDITY) && !(c.need & (rvk::FF_ONE_I64 | rvk::FF_ONE_F64)) && nv_out == 0;
    const int prefer = mirror ? rvk::FF_PROJALL
                              : ((none && (c.need & rvk::FF_VALIDITY)) ? (rvk::FF_PROJALL | rvk::FF_NONULL) : ((no_out_validity && !all_proj) ? rvk::FF_NONULL : 0));
    c.stage_row_bytes = row_bytes;

    // Most rows survive and the outputs are plain value columns: the direct kernel (direct_kernel.hpp), which keeps a tile's rows
    // in registers until its output offset is known
    bool plain = nvals >= 1 && nxs == 0 && ctx->opt_rows_per_lane <= 0 &&
                 ctx->opt_cap_rows == 0 && (ctx->opt_debug & ~int64_t(4)) == 0 && (p.in.strict_values >> npred) == 0;
    for (int s = npred; s < nvals; ++s) plain = plain && p.out_values[s] != nullptr;
    // measured crossovers against the staged geometries (tools/dense_sweep.py, profiles/r04_dense_sweep.txt): one loaded column
    // from 55 %; one column projected of several loaded from 60 % (the staged pass holds every survivor in its slots there);
    // two projected columns from 22 %, three or four from 15 % (their staged rows crowd the LDS slots early)
    // (columns that keep nulls carry a validity byte per row through the LDS slot: later, tools/dense_nullable.py -- two projected
    // columns from 35 %, three from 22 %)
    double dense_from = nvals == 1 ? rvt::kDirectFromOneColumn
                                   : (projected <= 1 ? rvt::kDirectFromOneProjectedOfSeveral : (projected == 2 ? rvt::kDirectFromTwoProjected : rvt::kDirectFromThreeProjected));
    if (nv_out && nvals > 1) dense_from = std::max(dense_from, projected <= 2 ? rvt::kDirectFromTwoProjectedNullable : rvt::kDirectFromThreeProjectedNullable);
    if (plain && (ctx->opt_direct > 0 || (ctx->opt_direct == 0 && seen >= dense_from))) use_direct(ctx, c, b, nv_out, seen, req, ranges, sel_deferred);

    // Geometry: the instantiation, then the LDS slots (rows a wave can stage per tile).  A wave with more survivors than its
    // slot holds leaves its range to the redo kernel, which re-reads it -- so a selectivity the default geometry's slots would
    // not hold (the context's last pass WITH THIS PREDICATE says so) walks down:
    //   1. the 16-wave instantiations with fewer rows per lane (their three-stage slots hold a larger share of a wave's rows);
    //   2. the same list sized for a dense selection (one workgroup per CU, two stages: a two-stage launch pays for the exposed
    //      look-back, 0.4-0.7 ms per 1e9 rows, so it comes second);
    //   3. the instantiation with the fewest waves (fused_roomy.hip), whose slots hold EVERY row of a wave.
    // Decided from the selectivity, which does not depend on the geometry, so the choice does not flip from call to call (a rule
    // on the share of redone tiles did: the dense geometry redoes none).  x > lit -> [x, y, fn], 5e8 rows, ms per call at
    // 10 / 20 / 30 / 50 / 90 %: default geometry + redo kernel 2.4 / 8.1 / 8.7 / 9.8 / 12.4; walked down 2.4 / 3.7 / 3.8 / 6.5 / 6.9
    // (tools/roomy_ab.py; one column: tools/dense_one.py).
    // (a pass over packed codes goes on with the plain lean class from its top instead of 3.)  The candidates and their order are the
    // rule's (fused_rule.hpp, Walk); here each one is sized, and the walk ends at the first whose slots are not crowded.
    rvf::Walk<rvk::FusedEntry> walk{staged_table(), kRuleFlags, {rvk::kNarrowTallRows, rvk::kPackedTallRows}, nvals, vec, c.need, prefer, ctx->opt_rows_per_lane, req && req->counts};
    for (c.staged = c.direct ? nullptr : walk.first(); !c.direct; c.staged = walk.next()) {
        // the caller will count the selection bitmap instead (a batch is no whole number of this candidate's wave ranges): the class that
        // writes it, at this step of the walk (the forms that write the selection bitmap read the 8-byte values)
        if (c.staged && sel_deferred && !c.make_selection && !counts_in_pass(req, c.staged->r)) {
            c.make_selection = true;
            c.staged = walk.reclass((walk.need | rvk::FF_SEL) & ~kNarrowFlags);
        }
        require(c.staged != nullptr, RV_ERR_INTERNAL, fmt("no fused kernel variant for %d columns, flags %d", nvals, walk.need));
        c.need = walk.need;
        size_staged(ctx, c, *c.staged, n, nvals, nxs, row_bytes, walk.dense_sizing());
        // expected survivors of a wave (+ 10 % and three standard deviations of a binomial) against the slot
        const uint32_t rows_per_wave = 64u * static_cast<uint32_t>(c.staged->r);
        const double expect = seen * rows_per_wave;
        const bool crowded = c.stage_row_bytes && c.cap < rows_per_wave && seen > 0.0 &&
                             expect * rvt::kCrowdedMargin + rvt::kCrowdedSigmas * std::sqrt(expect) > static_cast<double>(c.cap);
        if (!crowded || walk.last()) break;
    }
    if (!c.direct && seen >= 0.0 && c.stage_row_bytes) {
        c.redo_expected = redo_estimate(ctx, L, seen, sampled_now, c.cap, 64u * static_cast<uint32_t>(c.staged->r));
        // Per 1e9 rows of one column the redo kernel costs ~3.5 ms x the share of ranges it re-reads (tools/skew_sweep.py: sorted
        // 10 % 1.37 -> 1.68 ms, sorted 50 % 1.98 -> 3.95 ms); the direct kernel costs 0.8 ms more than the staged pass at 10 %
        // selectivity, 0.4 at 30 %, 0.25 at 50 % (profiles/r04_dense_sweep.txt).
        if (plain && ctx->opt_direct == 0 && ctx->opt_skew >= 0 &&
            c.redo_expected * rvt::kRedoMsPerShare > std::max(rvt::kDirectPenaltyFloor, rvt::kDirectPenaltyAt0 - rvt::kDirectPenaltySlope * seen) &&
            use_direct(ctx, c, b, nv_out, seen, req, ranges, sel_deferred))
            c.redo_expected = 0.0;
    }
    if (c.direct) c.r = c.direct->r, c.vec = 1, c.waves = c.direct->waves, c.flags = c.direct->flags, c.fn = c.direct->fn;
    else c.r = c.staged->r, c.vec = c.staged->vec, c.waves = c.staged->waves, c.flags = c.staged->flags, c.fn = c.staged->fn;
    if (!c.direct && (c.flags & kNarrowFlags)) c.narrow = narrow;
    return c;
}

// The rest of the pass's parameters, a control block, and the pass queued on the stream -- with the redo kernel behind it when ranges
// are expected to outgrow their slots, and the per-batch counts.  Fills what fused_finish reads.
static void launch_pass(rv_ctx *ctx, FusedLaunch &L, const LaunchChoice &c, int nvals, rv_dcolumn **sel_out, BatchReq *req, RangeOffsets *ranges,
                        double seen) {
    rvk::FusedParams &p = L.p;
    if (c.make_selection) make_selection(ctx, L, sel_out);
    p.ntiles = c.ntiles;
    p.cap_rows = c.cap;
    p.depth = static_cast<int32_t>(c.stages) - 1;

    // the staged pass lists the wave ranges whose survivors outgrew their LDS slot (fused_kernel.hpp, fused_redo_waves): one
    // word per range behind the descriptors, zeroed with them; the direct kernel's rows never leave their registers: no list
    L.range_rows = 64u * static_cast<uint32_t>(c.r);
    L.nranges = c.direct ? 0 : static_cast<uint64_t>(p.ntiles) * c.waves;
    L.ctrl = acquire_launch_ctrl(ctx, p.ntiles, L.nranges);
    Ctrl *ctrl = static_cast<Ctrl *>(L.ctrl.dev);
    p.state = reinterpret_cast<uint64_t *>(static_cast<unsigned char *>(L.ctrl.dev) + kCtrlBytes);
    p.ticket = &ctrl->ticket;
    p.err = &ctrl->err;
    p.out_count = &ctrl->out_count;
    p.out_valid_pop = ctrl->valid_pop;
    p.stamps = ctrl->stamps;
    p.debug = static_cast<int32_t>(ctx->opt_debug);
    p.spin_limit = ctx->opt_spin_limit > 0 ? static_cast<uint32_t>(ctx->opt_spin_limit) : rvk::kSpinLimit;
    p.redo_count = &ctrl->redo_count;
    p.redo = L.nranges ? reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(L.ctrl.dev) + kCtrlBytes + static_cast<size_t>(p.ntiles) * 8) : nullptr;

    const void *fn = reinterpret_cast<const void *>(c.fn);
    enable_lds(ctx, fn, c.lds);
    if (c.narrow) {
        const bool packed = c.narrow->layout == rvn::Layout::kPacked;
        p.narrow.codes = c.narrow->codes->ptr;
        p.narrow.bytes = packed ? std::min<uint64_t>(c.narrow->codes->bytes, rvn::packed_bytes(c.narrow->count)) : c.narrow->codes->bytes;
        p.narrow.base = c.narrow->base;
        require(p.in.nterms == 1, RV_ERR_INTERNAL, "narrow pass: one term");
        // a pass over packed codes: the tile loop's constants (tile_addr.hpp: the ragged tile, where a tile's and a wave's codes lie in the
        // companion), in term slots 2 and 3, which a one-term launch leaves unused (fused_kernel.hpp, put_tile_walk)
        if (packed) rvk::put_tile_walk(p.in, rvtile::codes_walk(p.in.n, c.r, c.waves, p.in.cols[0].offset, p.narrow.bytes, rvtile::kPackedCodes));
        // the pass compares codes: the term, lowered to ONE interval of codes once per launch -- a complement is folded into the
        // interval it is in wrap-around arithmetic.  The one term without an interval, the empty set over 4-byte codes, comes back
        // as it went in, `negate` set: the kernel tests the flag once per tile, outside its row loop, and runs such a launch through
        // the form of the loop that still flips its masks
        const rvk::DevTerm &t0 = p.in.terms[0];
        bool interval = false;
        const rvn::CodeTerm ct = rvn::fold_negate(rvn::lower_term(t0.sel_lt(), t0.sel_eq(), t0.sel_gt(), t0.lit, c.narrow->base), c.narrow->code_bytes, &interval);
        require(interval != ct.negate, RV_ERR_INTERNAL, "narrow pass: a folded term is an interval, and only an unfolded one is negated");
        // (in the term slot behind the launch's one term, which no other reader of `p` looks at: nterms stays 1.  truth(code) =
        // ((code - lo) as uint32 <= span) != negate, fused_kernel.hpp)
        p.in.terms[1].lit = static_cast<int64_t>(static_cast<uint64_t>(ct.lo) | (static_cast<uint64_t>(ct.span) << 32));
        p.in.terms[1].packed = ct.negate ? 1u : 0u;
        // (a pass over packed codes: which ends of the interval a code 0 .. range can fall outside of, narrow_sides.hpp -- its whole tiles
        //  run `code >= lo` or `code <= hi` alone for a one-sided interval.  In the same slot's `pad`: the block stays what it is)
        p.in.terms[1].pad = (packed && interval) ? static_cast<uint32_t>(rvn::classify_sides(ct.lo, ct.span, c.narrow->range)) : 0u;
        L.plain = {c.staged->fn_plain, c.lds_plain, static_cast<int32_t>(c.stages_plain) - 1};
        ctx->narrow_passes += 1;
    }
    // persistent grid: as many workgroups as the device keeps resident (tiles are handed out
    // by the ticket counter, so residency is a speed matter only, never correctness)
    auto occ = ctx->occupancy.find({fn, c.lds});
    if (occ == ctx->occupancy.end()) {
        int q = 0;
        RV_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, fn, c.waves * 64, c.lds));
        occ = ctx->occupancy.emplace(std::make_pair(fn, c.lds), std::max(1, q)).first;
    }
    int per_cu = occ->second;
    if (ctx->opt_wgs_per_cu > 0) per_cu = static_cast<int>(ctx->opt_wgs_per_cu);
    // + 1: workgroup 0 is the scanner (lookback.hpp, scanner_wave)
    uint64_t workers = std::min<uint64_t>(p.ntiles, static_cast<uint64_t>(ctx->props.multiProcessorCount) * per_cu - 1);
    if (ctx->opt_grid_limit > 0 && !c.direct) workers = std::min<uint64_t>(workers, static_cast<uint64_t>(ctx->opt_grid_limit));  // (tests: one workgroup, many tiles)
    const uint32_t grid = 1 + static_cast<uint32_t>(workers);
    p.overflow = &ctrl->overflow;
    if (ranges) {
        ranges->range_rows = 64u * static_cast<uint32_t>(c.r);
        ranges->out_capacity = p.out_capacity;
        ranges->expected_selectivity = seen;
        if (4096u % ranges->range_rows == 0) {
            ranges->offsets = pool_alloc(ctx, static_cast<size_t>(p.ntiles) * c.waves * 8 + 16);
            p.wave_offsets = static_cast<uint64_t *>(ranges->offsets->ptr);
        }
    }
    if (counts_in_pass(req, c.r)) {
        if (req->chunk_rows == 64u * static_cast<uint64_t>(c.r)) {
            // a batch IS a wave range (the reference's 1024-row batches at 16 rows per lane): the pass writes every batch's survivor
            // count where the caller reads it -- 128 bytes per tile over PCIe, spread over the whole pass; no scratch, no second kernel
            // (which took 39 us per 2^28-row window, serialised behind the pass whatever stream it ran on: profiles/r05_seam_*)
            p.batch_counts = req->counts;
            p.nbatch_counts = req->nb;
            req->counted = true;
            ctx->batch_counts_in_pass += 1;
        } else {
            L.wave_counts = pool_alloc(ctx, static_cast<size_t>(p.ntiles) * c.waves * 4 + 16);
            p.wave_counts = static_cast<uint32_t *>(L.wave_counts->ptr);
        }
    }
    L.direct_stamp = c.direct && (c.flags & rvk::FF_STAMP);
    L.fn = c.fn;
    L.grid = grid;
    L.block = static_cast<uint32_t>(c.waves * 64);
    L.lds = c.lds;
    L.timed = ctx->opt_profile != 0;
    L.need = c.need;
    L.nvals = nvals;
    L.stage_row_bytes = c.stage_row_bytes;
    ctx->last_kernel = c.direct ? fmt("fused_direct_compact<%d,%d,%d,%d,%d>", c.direct->np, c.direct->nq, c.r, c.waves, c.flags)
                                : fmt("fused_filter_compact<%d,%d,%d,%d,%d>", nvals, c.r, c.vec, c.waves, c.flags);
    // a free control block for this pass to zero while it runs (big launches: the zeroing hides in the pass), for a later launch
    int zero_at = -1;
    if (p.in.n >= rvt::kRangesFromRows && c.waves >= 2) {
        zero_at = block_to_zero(ctx, L.ctrl);
        if (zero_at >= 0) {
            const rv_ctx::LaunchCtrl &z = ctx->ctrl_free[static_cast<size_t>(zero_at)];
            p.zero_ptr = static_cast<rvk::rv_u32x4 *>(z.dev);
            p.zero_n16 = (std::min(z.dirty, z.bytes) + 15) / 16;
        }
    }
    if (L.timed) {  // the launch's own pair of events: launches of a stream's windows overlap (rv_filter_project_chunked_begin)
        if (!L.ctrl.tk0) {
            RV_HIP(hipEventCreate(&L.ctrl.tk0));
            RV_HIP(hipEventCreate(&L.ctrl.tk1));
        }
        RV_HIP(hipEventRecord(L.ctrl.tk0, ctx->stream));
    }
    hipLaunchKernelGGL(c.fn, dim3(grid), dim3(c.waves * 64), c.lds, ctx->stream, p);
    RV_HIP(hipGetLastError());
    if (zero_at >= 0) {  // queued: whatever follows on this stream finds the block zero
        rv_ctx::LaunchCtrl &z = ctx->ctrl_free[static_cast<size_t>(zero_at)];
        z.clean = std::min(z.dirty, z.bytes);
    }
    p.zero_ptr = nullptr;  // (a re-run after an output overflow zeroes nothing: the block may be in use by then)
    p.zero_n16 = 0;
    // ranges are expected to outgrow their slots (they did the last time): the redo kernel follows the pass on the stream at
    // once instead of waiting for the host to read the count
    L.redo_queued = L.nranges && (c.redo_expected > 0.0 || L.place_edge) && (c.stage_row_bytes || p.nxs);
    if (L.redo_queued) launch_redo(ctx, L);
    if (L.timed) RV_HIP(hipEventRecord(L.ctrl.tk1, ctx->stream));
    if (p.wave_counts) {
        // wave counts -> the caller's per-batch array (pinned host memory, written by the device: no read-back to queue); the scratch is
        // kept until the launch is finished
        const uint64_t per_batch = req->chunk_rows / (64u * static_cast<uint64_t>(c.r)), nwaves = static_cast<uint64_t>(p.ntiles) * c.waves;
        const uint64_t threads = per_batch < 32 ? req->nb : (per_batch < 4096 ? req->nb * 64 : req->nb * 256);
        const dim3 cgrid(static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((threads + 255) / 256, static_cast<uint64_t>(ctx->props.multiProcessorCount) * 8))));
        hipLaunchKernelGGL(rvk::batch_counts_from_waves, cgrid, dim3(256), 0, ctx->stream, static_cast<const uint32_t *>(p.wave_counts), nwaves, per_batch, req->nb, req->counts);
        RV_HIP(hipGetLastError());
        req->counted = true;
        ctx->batch_counts_in_pass += 1;
        p.wave_counts = nullptr;  // a re-run after an output overflow does not count again (the first pass's counts are exact)
    }
    p.batch_counts = nullptr;  // (likewise)
    RV_HIP(hipMemcpyAsync(L.ctrl.host, L.ctrl.dev, kCtrlBytes, hipMemcpyDeviceToHost, ctx->stream));
    RV_HIP(hipEventRecord(L.ctrl.ev, ctx->stream));
    L.launched = true;
}

// One single-pass launch: predicate over `cols`, compaction of the columns in proj; queued on the context's
// stream, not waited for.  out[] / sel_out receive the output handles at once (their length is set by
// fused_finish).
void fused_begin(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const rv_term *terms,
                 uint32_t nterms, rv_null_policy policy, const uint32_t *proj, uint32_t nproj,
                 rv_dcolumn **out, rv_dcolumn **sel_out, FusedLaunch &L, const ExprInfo *ex, BatchReq *req,
                 RangeOffsets *ranges) {
    rvk::FusedParams &p = L.p;
    p = rvk::FusedParams{};
    Bound b = bind_inputs(cols, ncols, terms, nterms, policy, ex, p.in);
    const uint64_t n = p.in.n;
    L.signature = predicate_signature(cols, ncols, terms, nterms, policy, ex);
    double seen = L.place ? L.place_selectivity : ctx->seen_selectivity(L.signature);  // (a segment: its own density, out of the profile)
    bool sampled_now = false;  // `seen` comes from a sample taken by this call: its histogram is in ctx->last_sample_hist
    if (seen < 0.0 && !L.place) {
        seen = first_call_sample(ctx, p.in, b.nvals, L.signature);
        sampled_now = seen >= 0.0;
    }

    // Output capacity (output_capacity above).  Option "out_sizing": 0 = sized from the predicate's known selectivity for big tables,
    // for every row otherwise; -1 = always for every row (no second pass, 2x the input in HBM); 1 = the context's last observed
    // selectivity x 1.5 + 1 % (a stream of similar batches), k >= 2 = a caller-given bound of k rows per million.  A launch that
    // overflows its outputs still counts exactly; fused_finish then re-runs it with buffers of the exact size
    // (record_batch.rs:131-178 never over-allocates either: the builders grow).
    // (a stretch appends at row place_base of the caller's buffers: pointers rounded down to a 128-byte line, the rest enters the
    // chain as the output row of its first survivor -- FusedParams::out_bias -- and every buffer and capacity below counts from there)
    L.out_bias = L.place ? static_cast<uint32_t>(L.place_base & 15) : 0u;
    p.out_bias = L.out_bias;
    const uint64_t cap_out = L.place ? (L.place_capacity > L.place_base ? L.place_capacity - L.place_base : 0) + L.out_bias : output_capacity(ctx, n, seen);
    ctx->fused_rows_scanned += n;
    L.n = n;
    const size_t row_bytes = bind_outputs(b, ncols, proj, nproj, out, L);
    alloc_outputs(ctx, L, cap_out);
    // a selection bitmap wanted only for per-batch counts is decided with the geometry
    const bool sel_deferred = sel_out && req && req->sel_optional && n > 0;
    if (sel_deferred) *sel_out = nullptr;
    else if (sel_out) make_selection(ctx, L, sel_out);
    if (n == 0) {
        for (auto &o : L.outs) {
            o.col->length = 0;
            o.col->null_count = 0;
            o.col->validity.reset();
        }
        L.launched = false;
        return;
    }
    // the lean one-column Int64 pass: the buffer's narrow companion, when it has one this view can read (narrow.hip)
    const rv_dcolumn *lean = (b.nvals == 1 && nterms == 1 && !ex && !L.place && cols[terms[0].column]->dtype == RV_INT64) ? cols[terms[0].column] : nullptr;
    narrow_note_extent(ctx, lean);
    const bool lean_counts = req && req->counts;
    const LaunchChoice c = choose_launch(ctx, L, b, row_bytes, ex != nullptr, sel_deferred, seen, sampled_now, req, ranges, lean ? narrow_codes_for(ctx, lean, lean_counts) : nullptr);
    if (lean && c.staged && !c.direct && (c.flags & rvk::FF_ONE_I64)) {  // counted towards the buffer's whole scans by fused_finish
        L.lean_values = lean->values;
        L.lean_offset = lean->offset;
        L.lean_counts = lean_counts;
    }
    launch_pass(ctx, L, c, b.nvals, sel_out, req, ranges, seen);
}

// What a pass over this predicate would be sized by: the selectivity it had the last time it ran over these buffers, or -- a predicate
// the context has not seen, over a big table -- the strided sample its first launch would take (taken here instead, once); < 0: unknown.
// For decisions that precede the launch (which columns the pass should carry at all: query.hip, filter_by_groups).
double expected_selectivity(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const rv_term *terms, uint32_t nterms, rv_null_policy policy,
                            const ExprInfo *ex) {
    const uint64_t signature = predicate_signature(cols, ncols, terms, nterms, policy, ex);
    const double known = ctx->seen_selectivity(signature);
    if (known >= 0.0) return known;
    rvk::ScanInputs in{};
    const Bound b = bind_inputs(cols, ncols, terms, nterms, policy, ex, in);  // (the errors a pass would raise before its sample)
    return first_call_sample(ctx, in, b.nvals, signature);
}

// Waits for the launch, runs the redo kernel when wave ranges outgrew their slots (unless it was queued behind the pass), fixes the output lengths / null counts.
uint64_t fused_finish(rv_ctx *ctx, FusedLaunch &L) {
    if (!L.launched) return 0;
    rvk::FusedParams &p = L.p;
    std::vector<OutCol> &outs = L.outs;
    struct Release {
        rv_ctx *ctx;
        FusedLaunch &L;
        ~Release() {
            L.wave_counts.reset();
            release_launch_ctrl(ctx, L.ctrl);
            L.launched = false;
        }
    } release{ctx, L};
    RV_HIP(hipEventSynchronize(L.ctrl.ev));
    L.wave_counts.reset();
    const Ctrl *h = static_cast<const Ctrl *>(L.ctrl.host);
    if (L.timed) {
        float ms = 0.f;
        RV_HIP(hipEventElapsedTime(&ms, L.ctrl.tk0, L.ctrl.tk1));
        ctx->kernel_ms += ms;
        ctx->kernel_launches += 1;
    }
    require(h->err == 0, RV_ERR_DEVICE, "fused kernel: look-back spin limit reached (device fault or lost workgroup)");
    ctx->last_selectivity = L.n ? static_cast<double>(h->out_count) / static_cast<double>(L.n) : 0.0;
    ctx->last_rows_out = h->out_count, ctx->last_rows_in = L.n;
    if (!L.place) ctx->remember_selectivity(L.signature, ctx->last_selectivity);
    bool rerun = false;
    if (L.place && (h->overflow || h->out_count > p.out_capacity)) {  // the shared outputs are the caller's: it falls back to one pass
        L.overflowed = true;
        throw SegmentOverflow{};
    }
    if (h->overflow || h->out_count > p.out_capacity) {
        rerun = true;
        // speculative output sizing guessed too low: the count is exact, so give every output exactly that many rows
        // and run the pass once more (same kernel, same geometry, fresh descriptors)
        const uint64_t exact = h->out_count;
        alloc_outputs(ctx, L, exact);
        const size_t zeroed = kCtrlBytes + (static_cast<size_t>(p.ntiles) + L.nranges) * 8;
        RV_HIP(hipMemsetAsync(L.ctrl.dev, 0, (zeroed + 15) & ~size_t(15), ctx->stream));
        // a pass over codes: re-run over the 8-byte values, whose slots of the same rows take 8 bytes per row
        if (L.plain.fn) {
            enable_lds(ctx, reinterpret_cast<const void *>(L.plain.fn), L.plain.lds);
            p.depth = L.plain.depth;  // (the stages plain.lds holds: size_staged)
        }
        hipLaunchKernelGGL(L.plain.fn ? L.plain.fn : L.fn, dim3(L.grid), dim3(L.block), L.plain.fn ? L.plain.lds : L.lds, ctx->stream, p);
        RV_HIP(hipGetLastError());
        RV_HIP(hipMemcpyAsync(L.ctrl.host, L.ctrl.dev, kCtrlBytes, hipMemcpyDeviceToHost, ctx->stream));
        RV_HIP(hipStreamSynchronize(ctx->stream));
        require(h->err == 0 && h->overflow == 0 && h->out_count == exact, RV_ERR_INTERNAL, "re-run after an output overflow disagrees with the first pass");
        ctx->overflow_reruns += 1;
    }
    ctx->last_redo_fraction = L.nranges ? static_cast<double>(h->redo_count) / static_cast<double>(L.nranges) : 0.0;
    if (L.nranges && !L.place) {  // a staged pass ran: what it left to the redo kernel sizes the predicate's next launch (fused_begin, redo_estimate)
        if (rv_ctx::SeenPredicate *q = ctx->seen_entry(L.signature)) {
            q->redo_fraction = ctx->last_redo_fraction, q->redo_at = ctx->last_selectivity;
            q->redo_ratio = L.range_rows ? static_cast<double>(p.cap_rows) / L.range_rows : 1.0;
        }
    }
    if (h->redo_count > 0 && (L.stage_row_bytes || p.nxs) && !(L.redo_queued && !rerun)) {
        if (L.timed) RV_HIP(hipEventRecord(ctx->evk0, ctx->stream));
        launch_redo(ctx, L);
        if (L.timed) RV_HIP(hipEventRecord(ctx->evk1, ctx->stream));
        RV_HIP(hipMemcpyAsync(L.ctrl.host, L.ctrl.dev, kCtrlBytes, hipMemcpyDeviceToHost, ctx->stream));
        RV_HIP(hipStreamSynchronize(ctx->stream));
        if (L.timed) {  // the redo kernel is part of the pass's device time
            float ms = 0.f;
            RV_HIP(hipEventElapsedTime(&ms, ctx->evk0, ctx->evk1));
            ctx->kernel_ms += ms;
        }
        require(h->overflow == 0, RV_ERR_INTERNAL, "redo kernel: outputs too small after the pass fitted them");
    }
    const uint64_t rows = h->out_count;
    if (ctx->opt_debug & 4)
        fprintf(stderr, "[scan] tiles %llu | scanner polls %llu, tiles scanned %llu, empty polls %llu | fallback look-backs %llu\n",
                static_cast<unsigned long long>(p.ntiles), h->stamps[28], h->stamps[29], h->stamps[30], h->stamps[31]);
    if ((ctx->opt_debug & 4) && L.nranges == 0)
        fprintf(stderr, "[scan] direct kernel: tiles whose predecessor's prefix was not there at the top of the iteration: looked again once %llu, twice %llu, three times %llu, four %llu\n",
                h->stamps[16], h->stamps[17], h->stamps[18], h->stamps[19]);
    if (L.direct_stamp) {  // diagnostic instantiations of the direct kernel: where an ordinary wave's cycles go, per tile
        const double t = static_cast<double>(p.ntiles);
        const unsigned long long *q = h->stamps;
        fprintf(stderr, "[stamp direct] cycles/tile (s_memtime, wave 1): load wait %.0f | predicate+count %.0f | barrier 1 %.0f | publish..offset (wave 0: %.0f) %.0f | barrier 2 %.0f | stores %.0f | barrier 3 %.0f | moves+load issue %.0f\n",
                q[0] / t, q[1] / t, q[2] / t, q[8] / t, q[3] / t, q[4] / t, q[5] / t, q[6] / t, q[7] / t);
    }
    if ((L.need & rvk::FF_STAMP) && ctx->opt_stamp) {
        std::memcpy(ctx->last_stamps, h->stamps, sizeof(h->stamps));
        for (int w = 0; w < 2; ++w) {
            const unsigned long long *q = h->stamps + 8 * w;
            const double t = static_cast<double>(std::max<unsigned long long>(1, q[5]));
            if (w == 1) {
                fprintf(stderr, "[stamp] wave1 cycles/tile: of eval: load wait %.0f, stage %.0f\n", q[6] / t, q[7] / t);
            }
            fprintf(stderr, "[stamp] wave%d cycles/tile: eval(+ticket,+load wait) %.0f | scatter+prefetch %.0f | lookback %.0f | barrierB %.0f | flush %.0f | tiles %llu | polls/tile %.2f windows/tile %.2f\n",
                    w, q[0] / t, q[1] / t, q[2] / t, q[3] / t, q[4] / t, q[5], q[6] / t, q[7] / t);
        }
    }
    for (auto &o : outs) {
        o.col->length = rows;
        o.col->offset = 0;
        long long valid_pop = -1;
        if (o.value_slot >= 0 && o.col->validity) valid_pop = static_cast<long long>(h->valid_pop[o.value_slot]);
        if (o.xs_valid >= 0) valid_pop = static_cast<long long>(h->valid_pop[rvk::kMaxValueCols + o.xs_valid]);
        if (valid_pop < 0) {
            o.col->null_count = 0;
        } else {
            o.col->null_count = static_cast<int64_t>(rows) - valid_pop;
            // builder drops it (primitive.rs:179-185) -- a stretch keeps its own: the table's bitmap is put together from all of them
            if (o.col->null_count == 0 && !L.place) o.col->validity.reset();
        }
    }
    if (L.lean_values) {  // a whole scan more of the column's buffer?  Its narrow companion is queued behind this pass then (narrow.hip)
        const DevBufRef values = std::move(L.lean_values);
        L.lean_values.reset();
        narrow_after_pass(ctx, *values, L.lean_offset, L.n, L.lean_counts);
    }
    return rows;
}

void abandon_launch(rv_ctx *ctx, FusedLaunch &L) {
    if (!L.launched) return;
    (void)hipStreamSynchronize(ctx->stream);
    L.wave_counts.reset();
    release_launch_ctrl(ctx, L.ctrl);
    L.launched = false;
}

// ---- a table filtered stretch by stretch ------------------------------------------------------------------------------------------
// The reference filters whatever order its source has (plan.rs:112-147) and `col > lit` columns are ids and timestamps: SORTED.  The
// survivors of such a table sit in one or two long stretches -- which the strided sample shows as a profile of its 1024 blocks in table
// order (agg_kernel.hpp).  One launch sized for the table's global selectivity is wrong everywhere there: the staged pass's slots
// overflow where every row survives (the redo kernel re-reads those ranges), the direct kernel crawls at its chain's pace where none
// does.  So the table is cut at the profile's edges and every stretch gets the kernel ITS density asks for -- the staged pass where
// (nearly) nothing survives, the direct kernel where (nearly) everything does -- all writing into one set of outputs, each stretch
// from the row where the one before it ended (the host reads that count between two launches: ~30 us each).  No range is read twice.
namespace {
struct Stretch {
    uint64_t row0, row1;
    double density;
};
// at most kMost stretches, each at least kLeast blocks long and clearly sparse or clearly dense (thresholds.hpp); anything else --
// survivors in many runs, independent rows -- is not a table to cut
bool plan_stretches(const rv_ctx::SeenPredicate &q, uint64_t n, std::vector<Stretch> &out) {
    constexpr int kBlocks = 1024, kLeast = rvt::kStretchLeastBlocks, kMost = rvt::kStretchesMost;
    if (!q.profile_stride || q.profile_rows != n) return false;
    int cls[kBlocks];
    for (int b = 0; b < kBlocks; ++b) cls[b] = q.profile[b] <= rvt::kStretchSparseUpTo * 1024 ? 0 : (q.profile[b] >= rvt::kStretchDenseFrom * 1024 ? 2 : 1);
    // single blocks of another class inside a stretch (a run's edge falls into the block) take their neighbours' class
    for (int b = 1; b + 1 < kBlocks; ++b)
        if (cls[b] != cls[b - 1] && cls[b - 1] == cls[b + 1]) cls[b] = cls[b - 1];
    struct Run {
        int first, count, cls;
        uint64_t survivors;
    };
    std::vector<Run> runs;
    for (int b = 0; b < kBlocks; ++b) {
        if (runs.empty() || runs.back().cls != cls[b]) runs.push_back(Run{b, 0, cls[b], 0});
        runs.back().count += 1;
        runs.back().survivors += q.profile[b];
    }
    // an in-between block or two at an edge joins the stretch before it
    std::vector<Run> merged;
    for (const Run &r : runs) {
        if (r.cls == 1 && r.count <= 2 && !merged.empty()) {
            merged.back().count += r.count;
            merged.back().survivors += r.survivors;
        } else if (!merged.empty() && merged.back().cls == r.cls) {
            merged.back().count += r.count;
            merged.back().survivors += r.survivors;
        } else {
            merged.push_back(r);
        }
    }
    if (merged.size() < 2 || merged.size() > static_cast<size_t>(kMost)) return false;
    bool sparse = false, dense = false;
    for (const Run &r : merged) {
        if (r.cls == 1 || r.count < kLeast) return false;
        sparse = sparse || r.cls == 0;
        dense = dense || r.cls == 2;
    }
    if (!sparse || !dense) return false;
    out.clear();
    uint64_t at = 0;
    for (size_t k = 0; k < merged.size(); ++k) {
        const Run &r = merged[k];
        // the edge lies somewhere between two sampled blocks: cut at the start of the next stretch's first block, on a tile boundary
        uint64_t end = k + 1 == merged.size() ? n : std::min<uint64_t>(n, (static_cast<uint64_t>(r.first + r.count) * q.profile_stride) & ~uint64_t(16383));
        if (end <= at) return false;
        out.push_back(Stretch{at, end, static_cast<double>(r.survivors) / (1024.0 * r.count)});
        at = end;
    }
    return true;
}
}  // namespace

bool run_segmented_pass(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const rv_term *terms, uint32_t nterms, rv_null_policy policy,
                        const uint32_t *proj, uint32_t nproj, rv_dcolumn **out, const ExprInfo *ex, uint64_t *rows_out) {
    const uint64_t n = ncols ? cols[0]->length : 0;
    if (ctx->opt_segments < 0 || n < (ctx->opt_segments > 0 ? static_cast<uint64_t>(ctx->opt_segments) : rvt::kStretchFromRows) || nproj == 0 || ctx->opt_out_sizing < 0 || ctx->opt_rows_per_lane > 0 || ctx->opt_cap_rows > 0 || ctx->opt_debug) return false;
    for (uint32_t j = 0; j < nproj; ++j)
        if (proj[j] >= ncols || !is_value_type(cols[proj[j]]->dtype)) return false;  // 8-byte values land in place; a bitmap is put together afterwards
    const uint64_t signature = predicate_signature(cols, ncols, terms, nterms, policy, ex);
    // (a predicate the context has not seen: the strided sample its first launch would take, taken here -- once, the pass will not repeat it)
    if (!ctx->seen_entry(signature)) (void)expected_selectivity(ctx, cols, ncols, terms, nterms, policy, ex);
    const rv_ctx::SeenPredicate *q = ctx->seen_entry(signature);
    std::vector<Stretch> plan;
    if (!q || !plan_stretches(*q, n, plan)) return false;
    {  // what a pass over the whole table has counted since the sample was taken outranks the profile
        double promised = 0.0;
        for (const Stretch &s : plan) promised += s.density * static_cast<double>(s.row1 - s.row0);
        const double known = ctx->seen_selectivity(signature);
        if (known >= 0.0 && std::fabs(known - promised / static_cast<double>(n)) > rvt::kStretchKnownBand) return false;
    }
    // one set of outputs for all stretches: what the profile says survives x 1.2 + 2 % of the rows
    double expect = 0.0;
    for (const Stretch &s : plan) expect += s.density * static_cast<double>(s.row1 - s.row0);
    const uint64_t capacity = std::min<uint64_t>(n, static_cast<uint64_t>(expect * rvt::kOutSizingFactor + static_cast<double>(n) * rvt::kOutSizingSlack) + 4096);
    std::vector<DevBufRef> bufs;
    for (uint32_t j = 0; j < nproj; ++j) bufs.push_back(pool_alloc(ctx, std::max<size_t>(elem_bytes(cols[proj[j]]->dtype, capacity), 8)));
    uint64_t base = 0;
    std::string kernels;
    const uint64_t launches_before = ctx->kernel_launches;
    // a column that keeps nulls: every stretch writes a bitmap of its own (bit 0 = its first survivor), concatenated at the end
    struct Bits {
        DevBufRef words;
        uint64_t first, rows;  // bit of the first survivor (the stretch's out_bias), survivors
        int64_t nulls;
    };
    std::vector<std::vector<Bits>> bitmaps(nproj);
    try {
        for (const Stretch &s : plan) {
            std::vector<std::unique_ptr<rv_dcolumn>> views;
            std::vector<const rv_dcolumn *> vc;
            for (uint32_t c = 0; c < ncols; ++c) {
                auto v = std::make_unique<rv_dcolumn>(*cols[c]);
                v->offset = cols[c]->offset + s.row0;
                v->length = s.row1 - s.row0;
                v->null_count = cols[c]->dtype == RV_NULL ? static_cast<int64_t>(v->length) : (cols[c]->validity ? -1 : 0);  // (rv_slice)
                vc.push_back(v.get());
                views.emplace_back(std::move(v));
            }
            FusedLaunch L;
            L.place = &bufs;
            L.place_base = base;
            L.place_capacity = capacity;
            L.place_selectivity = s.density;
            L.place_edge = s.density < 0.5;  // (a plan alternates sparse and dense stretches: queue the redo kernel behind the pass, ~13 us,
                                             //  instead of a second launch after the host has read the count, ~45 us)
            std::vector<rv_dcolumn *> tmp(nproj, nullptr);
            struct Drop {  // the stretch's output handles are views of the shared buffers: dropped, whatever happens
                std::vector<rv_dcolumn *> &t;
                ~Drop() {
                    for (auto *d : t) delete d;
                }
            } drop{tmp};
            fused_begin(ctx, vc.data(), ncols, terms, nterms, policy, proj, nproj, tmp.data(), nullptr, L, ex, nullptr, nullptr);
            uint64_t kept = 0;
            try {
                kept = fused_finish(ctx, L);
            } catch (...) {
                abandon_launch(ctx, L);
                throw;
            }
            for (uint32_t j = 0; j < nproj; ++j)
                if (tmp[j] && tmp[j]->validity) bitmaps[j].push_back(Bits{tmp[j]->validity, L.out_bias, kept, tmp[j]->null_count});
            base += kept;
            kernels += (kernels.empty() ? "" : " + ") + ctx->last_kernel;
        }
    } catch (const SegmentOverflow &) {
        RV_HIP(hipStreamSynchronize(ctx->stream));
        if (rv_ctx::SeenPredicate *m = ctx->seen_entry(signature)) m->profile_stride = 0;  // a profile that lied is not asked again
        ctx->segment_fallbacks += 1;
        return false;  // more survivors than the profile promised: the one-pass path, which counts exactly and re-runs itself
    }
    std::vector<std::unique_ptr<rv_dcolumn>> made;
    for (uint32_t j = 0; j < nproj; ++j) {
        auto o = std::make_unique<rv_dcolumn>();
        o->dtype = cols[proj[j]]->dtype;
        o->values = bufs[j];
        o->length = base;
        o->null_count = 0;
        for (const Bits &b : bitmaps[j]) o->null_count += b.nulls;
        if (o->null_count > 0) {  // (record_batch.rs:277-342's bitmap concatenation, over the stretches' bitmaps as Boolean columns)
            std::vector<std::unique_ptr<rv_dcolumn>> parts;
            std::vector<const rv_dcolumn *> pp;
            for (const Bits &b : bitmaps[j]) {
                auto c = std::make_unique<rv_dcolumn>();
                c->dtype = RV_BOOLEAN, c->values = b.words, c->offset = b.first, c->length = b.rows, c->null_count = 0;
                pp.push_back(c.get());
                parts.emplace_back(std::move(c));
            }
            rv_dcolumn *merged = nullptr;
            require(bitmaps[j].size() == plan.size(), RV_ERR_INTERNAL, "a stretch lost its bitmap");
            if (rv_concat(ctx, pp.data(), static_cast<uint32_t>(pp.size()), &merged) != RV_OK) throw Error(RV_ERR_INTERNAL, "stretches: the bitmaps could not be put together");
            o->validity = merged->values;
            delete merged;
        }
        made.emplace_back(std::move(o));
    }
    for (uint32_t j = 0; j < nproj; ++j) out[j] = made[j].release();
    ctx->last_selectivity = n ? static_cast<double>(base) / static_cast<double>(n) : 0.0;
    ctx->last_rows_out = base, ctx->last_rows_in = n;
    ctx->remember_selectivity(signature, ctx->last_selectivity);
    ctx->last_kernel = "stretches: " + kernels;
    if (ctx->kernel_launches > launches_before) ctx->kernel_launches = launches_before + 1;  // (the stretches' device times add up to ONE pass over the table)
    ctx->segmented_passes += 1;
    *rows_out = base;
    return true;
}

// begin + finish: the synchronous form
uint64_t run_fused_pass(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const rv_term *terms,
                        uint32_t nterms, rv_null_policy policy, const uint32_t *proj, uint32_t nproj,
                        rv_dcolumn **out, rv_dcolumn **sel_out, const ExprInfo *ex, BatchReq *req,
                        const AfterLaunch *after_launch, RangeOffsets *ranges) {
    FusedLaunch L;
    fused_begin(ctx, cols, ncols, terms, nterms, policy, proj, nproj, out, sel_out, L, ex, req, ranges);
    if (after_launch && *after_launch) {
        try {
            (*after_launch)(sel_out ? *sel_out : nullptr);
        } catch (...) {
            abandon_launch(ctx, L);  // the pass may still be running: drain before its buffers go
            throw;
        }
    }
    return fused_finish(ctx, L);
}

}  // namespace rvl
