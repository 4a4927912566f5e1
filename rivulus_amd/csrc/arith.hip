// Arithmetic expressions on the device (K8): rv_eval_arith types a postfix program of + - * / over columns and literals once, on
// the host, and evaluates it for every row in one launch of arith_kernel (arith_kernel.hpp; the cell rules are arith_cell.hpp's).
// One unit of the backend library behind include/rivulus_gpu.h (gfx950 only; compiled with hipcc, -ffp-contract=off: a * b + c is
// two roundings).  Shared helpers are declared in launch.hpp (namespace rvl).
#include "arith_kernel.hpp"
#include "launch.hpp"

using namespace rvh;
using namespace rvl;

namespace rvl {
namespace {

// what the typing walk knows about one entry of the operand stack
struct Operand {
    int dtype;      // rvarith::T_NULL / T_INT64 / T_FLOAT64
    int lit_step;   // a bare literal: index of its S_PUSH_LIT in the typed program (converted in place); else -1
};

// The typed program of a call, or what the call is without a launch
struct Typed {
    rvk::ArithParams p{};
    std::vector<const rv_dcolumn *> read;  // the distinct columns read, in the order of first use
    int dtype = rvarith::T_NULL;
    uint32_t depth = 0;
    bool all_null = false;  // some leaf is an RV_NULL column or a Null literal
    bool int_div = false;
};

void add_step(Typed &t, uint32_t op, uint32_t arg = 0, int64_t lit = 0) {
    require(t.p.nsteps < rvarith::kMaxTypedSteps, RV_ERR_INTERNAL, "rv_eval_arith: typed program too long");
    t.p.steps[t.p.nsteps++] = rvk::ArithStep{op, arg, lit};
}

// Int64 operand `o` (top: the top entry, else the one below) meets a Float64: a bare literal is converted here, anything else by a step
void promote(Typed &t, Operand &o, bool top) {
    if (o.dtype != rvarith::T_INT64) return;
    if (o.lit_step >= 0) {
        rvk::ArithStep &s = t.p.steps[o.lit_step];
        s.lit = static_cast<int64_t>(rvarith::f64_bits(rvarith::i64_to_f64(s.lit)));
    } else {
        add_step(t, top ? rvarith::S_I2F_TOP : rvarith::S_I2F_SECOND);
    }
    o.dtype = rvarith::T_FLOAT64;
}

Typed type_program(const rv_dcolumn *const *cols, uint32_t ncols, const rv_arith_step *steps, uint32_t n_steps) {
    Typed t;
    require(n_steps >= 1, RV_ERR_INVALID_ARG, "rv_eval_arith: empty program");
    require(n_steps <= rvarith::kMaxSteps, RV_ERR_UNSUPPORTED, fmt("rv_eval_arith: %u steps, at most %u are supported", n_steps, rvarith::kMaxSteps));
    std::vector<Operand> stack;
    for (uint32_t k = 0; k < n_steps; ++k) {
        const rv_arith_step &s = steps[k];
        if (s.op == RV_ARITH_COL) {
            require(s.column < ncols && cols[s.column], RV_ERR_INVALID_ARG, fmt("rv_eval_arith: step %u reads column %u of %u", k, s.column, ncols));
            const rv_dcolumn *c = cols[s.column];
            require(c->dtype == RV_NULL || is_value_type(c->dtype), RV_ERR_TYPE_MISMATCH,
                    fmt("rv_eval_arith: column %u is neither Int64 nor Float64: no arithmetic on Boolean / String", s.column));
            uint32_t slot = 0;
            while (slot < t.read.size() && t.read[slot] != c) ++slot;
            if (slot == t.read.size()) {
                require(t.read.size() < rvarith::kMaxCols, RV_ERR_UNSUPPORTED, fmt("rv_eval_arith: more than %u distinct columns", rvarith::kMaxCols));
                t.read.push_back(c);
            }
            if (c->dtype == RV_NULL) t.all_null = true;
            add_step(t, rvarith::S_PUSH_COL, slot);
            stack.push_back(Operand{static_cast<int>(c->dtype), -1});
        } else if (s.op == RV_ARITH_LIT) {
            require(s.lit_type != RV_BOOLEAN && s.lit_type != RV_STRING, RV_ERR_TYPE_MISMATCH,
                    fmt("rv_eval_arith: step %u: no arithmetic on Boolean / String literals", k));
            require(s.lit_type == RV_NULL || is_value_type(s.lit_type), RV_ERR_INVALID_ARG, fmt("rv_eval_arith: step %u: unknown literal type", k));
            if (s.lit_type == RV_NULL) t.all_null = true;
            const int64_t bits = s.lit_type == RV_FLOAT64 ? static_cast<int64_t>(rvarith::f64_bits(s.lit.f)) : s.lit_type == RV_INT64 ? s.lit.i : 0;
            add_step(t, rvarith::S_PUSH_LIT, 0, bits);
            stack.push_back(Operand{static_cast<int>(s.lit_type), static_cast<int>(t.p.nsteps) - 1});
        } else {
            require(s.op >= RV_ARITH_ADD && s.op <= RV_ARITH_DIV, RV_ERR_INVALID_ARG, fmt("rv_eval_arith: step %u: unknown operator", k));
            require(stack.size() >= 2, RV_ERR_INVALID_ARG, fmt("rv_eval_arith: step %u: operator with fewer than two operands", k));
            Operand b = stack.back();
            stack.pop_back();
            Operand a = stack.back();
            stack.pop_back();
            const int r = rvarith::result_dtype(a.dtype, b.dtype);
            if (r == rvarith::T_FLOAT64) {
                promote(t, a, false);
                promote(t, b, true);
            }
            const uint32_t base = r == rvarith::T_FLOAT64 ? rvarith::S_ADD_F64 : rvarith::S_ADD_I64;
            add_step(t, base + static_cast<uint32_t>(s.op - RV_ARITH_ADD));
            if (r == rvarith::T_INT64 && s.op == RV_ARITH_DIV) t.int_div = true;
            stack.push_back(Operand{r, -1});
        }
        require(stack.size() <= rvarith::kMaxDepth, RV_ERR_UNSUPPORTED, fmt("rv_eval_arith: operand stack deeper than %u", rvarith::kMaxDepth));
        t.depth = std::max<uint32_t>(t.depth, static_cast<uint32_t>(stack.size()));
    }
    require(stack.size() == 1, RV_ERR_INVALID_ARG, fmt("rv_eval_arith: the program leaves %zu values, not one", stack.size()));
    require(!t.read.empty(), RV_ERR_INVALID_ARG, "rv_eval_arith: the program reads no column");
    for (const rv_dcolumn *c : t.read)
        require(c->length == t.read[0]->length, RV_ERR_LENGTH_MISMATCH,
                fmt("rv_eval_arith: columns of %llu and %llu rows", static_cast<unsigned long long>(t.read[0]->length), static_cast<unsigned long long>(c->length)));
    t.dtype = stack[0].dtype;
    return t;
}

// arith_kernel<K>: one wave per arith_words<K>() bitmap words, one workgroup per four such waves up to the cap, grid-stride beyond it
template <int K>
void launch(rv_ctx *ctx, const rvk::ArithParams &p) {
    const uint64_t waves = ((p.n + 63) / 64 + rvk::arith_words<K>() - 1) / rvk::arith_words<K>();
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((waves + 3) / 4, rvt::kArithGridMost));
    hipLaunchKernelGGL(rvk::arith_kernel<K>, dim3(grid), dim3(256), 0, ctx->stream, p);
    RV_HIP(hipGetLastError());
    ctx->last_kernel = fmt("arith_kernel<%d>", K);
}

}  // namespace
}  // namespace rvl

extern "C" {

rv_status rv_eval_arith(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const rv_arith_step *steps, uint32_t n_steps,
                        rv_dcolumn **out) {
    return guarded([&] {
        require(ctx && cols && steps && out, RV_ERR_INVALID_ARG, "rv_eval_arith: NULL argument");
        *out = nullptr;
        Typed t = type_program(cols, ncols, steps, n_steps);
        set_device(ctx);
        const uint64_t n = t.read[0]->length;
        auto o = std::make_unique<rv_dcolumn>();
        o->dtype = static_cast<rv_dtype>(t.dtype);
        o->length = n;
        if (t.all_null) {  // decided here: no kernel.  Placeholders under an all-zero bitmap; a Null result is a length alone
            o->null_count = static_cast<int64_t>(n);
            if (o->dtype != RV_NULL) {
                const size_t vb = std::max<size_t>(n * 8, 16), mb = std::max<size_t>(bitmap_words_bytes(n), 16);
                o->values = pool_alloc(ctx, vb);
                o->validity = pool_alloc(ctx, mb);
                RV_HIP(hipMemsetAsync(o->values->ptr, 0, vb, ctx->stream));
                RV_HIP(hipMemsetAsync(o->validity->ptr, 0, mb, ctx->stream));
                RV_HIP(hipStreamSynchronize(ctx->stream));
            }
            ctx->last_kernel = "arith_all_null";
            *out = o.release();
            return;
        }
        bool nullable = t.int_div;
        for (uint32_t k = 0; k < t.read.size(); ++k) {
            t.p.cols[k] = dev_view(t.read[k]);
            nullable = nullable || t.read[k]->validity;
        }
        t.p.ncols = static_cast<uint32_t>(t.read.size());
        t.p.n = n;
        o->values = pool_alloc(ctx, std::max<size_t>(n * 8, 16));
        if (nullable) o->validity = pool_alloc(ctx, std::max<size_t>(bitmap_words_bytes(n), 16));
        o->null_count = 0;
        if (n == 0) {
            ctx->last_kernel = "arith_empty";
            *out = o.release();
            return;
        }
        Ctrl *ctrl = prepare_ctrl(ctx, 0);
        t.p.out_values = static_cast<uint64_t *>(o->values->ptr);
        t.p.out_validity = nullable ? static_cast<uint64_t *>(o->validity->ptr) : nullptr;
        t.p.out_valid_pop = striped(ctx, &ctrl->valid_pop[0]);
        const uint32_t k = std::max(t.depth, t.p.ncols);  // entries of the stack, and columns held in registers
        if (k <= 2) launch<2>(ctx, t.p);
        else if (k <= 4) launch<4>(ctx, t.p);
        else launch<8>(ctx, t.p);
        const Ctrl *h = fetch_ctrl(ctx);
        if (nullable) o->null_count = static_cast<int64_t>(n - h->valid_pop[0]);
        *out = o.release();
    });
}

}  // extern "C"
