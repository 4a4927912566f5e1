// Cell semantics of arithmetic expressions (Expr::add / sub / mul / div, expr.rs:17-20, 44-74), written once for the device and the
// host: plain g++ compiles this header for the CPU test (tests/cpp/arith_cell_fuzz.cpp), hipcc for the kernel (arith_kernel.hpp).
//
// The reference types such an expression (infer_binary_result_type, logical_plan/plan.rs:235-262) and names it (resolve_expr_schema,
// :204-233) but never executes one (planner.rs:124-126, :151-156), so the rules below are this project's decisions, each leaning on
// the reference line next to it:
//   result dtype  infer_binary_result_type, bottom-up: Float64 on either side -> Float64; Int64 o Int64 -> Int64 (Divide included);
//                 Null o T / T o Null -> T; Null o Null -> Null.  A Boolean or String operand is a type mismatch (the reference
//                 infers Null silently there, plan.rs:259).
//   nulls         a null operand makes the cell null, as BooleanArray::and / or do (boolean.rs:120-152); the slot under a null
//                 holds the placeholder 0 / 0.0, as take_array writes it (record_batch.rs:142-146).  A Null leaf (an RV_NULL
//                 column, a Null literal) makes every cell null.
//   Int64         + - * wrap in two's complement (Rust's release build: wrapping_add / _sub / _mul); / truncates toward zero as
//                 Rust's does; x / 0 is NULL (Rust panics: a query must not); INT64_MIN / -1 is INT64_MIN (wrapping_div).
//   Int64 meeting Float64: the Int64 side is converted first, round to nearest even (`as f64`, Series::new's promotion,
//                 series.rs:210-212).
//   Float64       every operator is ONE correctly rounded IEEE-754 operation: x / 0.0 is +-inf or NaN, never null; NaN-ness is
//                 kept (payloads need not be); subnormals are kept; a * b + c is a multiply and an add, never a fused
//                 multiply-add -- the unit that includes this header for the device is built with -ffp-contract=off.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RVARITH_HD __host__ __device__ inline
#else
#define RVARITH_HD inline
#endif

namespace rvarith {

// rv_dtype / execution::DataType codes (schema.rs:1-8)
enum : int { T_NULL = 0, T_BOOLEAN = 1, T_INT64 = 2, T_FLOAT64 = 3, T_STRING = 4, T_MISMATCH = -1 };

// infer_binary_result_type for Plus / Minus / Multiply / Divide (plan.rs:250-260); T_MISMATCH for a Boolean / String operand
RVARITH_HD int result_dtype(int left, int right) {
    if (left == T_BOOLEAN || left == T_STRING || right == T_BOOLEAN || right == T_STRING) return T_MISMATCH;
    if (left == T_FLOAT64 || right == T_FLOAT64) return T_FLOAT64;
    if (left == T_INT64 || right == T_INT64) return T_INT64;  // Int64 o Int64, Null o Int64, Int64 o Null
    return T_NULL;
}

// the limits of one program (rv_eval_arith)
constexpr uint32_t kMaxSteps = 32;  // steps as the caller writes them
constexpr uint32_t kMaxDepth = 8;   // operand stack
constexpr uint32_t kMaxCols = 8;    // distinct columns read
// ... and of its typed form: every binary step may add one conversion (a literal is converted on the host)
constexpr uint32_t kMaxTypedSteps = kMaxSteps + kMaxSteps / 2;

// One step of the TYPED postfix program the host makes of the caller's: types are resolved once, so the program is the same for
// every row.  PUSH_COL: `arg` = slot of the column among the columns read; PUSH_LIT: `lit` = the Int64 value or the Float64 bits.
enum : uint32_t {
    S_PUSH_COL = 0,
    S_PUSH_LIT = 1,
    S_I2F_TOP = 2,     // the top entry, Int64 -> Float64
    S_I2F_SECOND = 3,  // the entry below it
    S_ADD_I64 = 4,
    S_SUB_I64 = 5,
    S_MUL_I64 = 6,
    S_DIV_I64 = 7,
    S_ADD_F64 = 8,
    S_SUB_F64 = 9,
    S_MUL_F64 = 10,
    S_DIV_F64 = 11
};

RVARITH_HD int64_t add_i64(int64_t a, int64_t b) { return static_cast<int64_t>(static_cast<uint64_t>(a) + static_cast<uint64_t>(b)); }
RVARITH_HD int64_t sub_i64(int64_t a, int64_t b) { return static_cast<int64_t>(static_cast<uint64_t>(a) - static_cast<uint64_t>(b)); }
RVARITH_HD int64_t mul_i64(int64_t a, int64_t b) { return static_cast<int64_t>(static_cast<uint64_t>(a) * static_cast<uint64_t>(b)); }
// false: the cell is null (b == 0), *out the placeholder 0
RVARITH_HD bool div_i64(int64_t a, int64_t b, int64_t *out) {
    if (b == 0) {
        *out = 0;
        return false;
    }
    if (b == -1) {  // wrapping_div: INT64_MIN / -1 == INT64_MIN
        *out = static_cast<int64_t>(uint64_t{0} - static_cast<uint64_t>(a));
        return true;
    }
    *out = a / b;
    return true;
}
RVARITH_HD double i64_to_f64(int64_t a) { return static_cast<double>(a); }  // round to nearest even
RVARITH_HD double add_f64(double a, double b) { return a + b; }
RVARITH_HD double sub_f64(double a, double b) { return a - b; }
RVARITH_HD double mul_f64(double a, double b) { return a * b; }
RVARITH_HD double div_f64(double a, double b) { return a / b; }

RVARITH_HD uint64_t f64_bits(double x) {
    union {
        double d;
        uint64_t u;
    } c;
    c.d = x;
    return c.u;
}
RVARITH_HD double bits_f64(uint64_t u) {
    union {
        double d;
        uint64_t u;
    } c;
    c.u = u;
    return c.d;
}

// One binary step on raw 8-byte cells.  *ok is cleared by an Int64 division by zero and otherwise left alone.
RVARITH_HD uint64_t apply(uint32_t step, uint64_t a, uint64_t b, bool *ok) {
    switch (step) {
        case S_ADD_I64: return static_cast<uint64_t>(add_i64(static_cast<int64_t>(a), static_cast<int64_t>(b)));
        case S_SUB_I64: return static_cast<uint64_t>(sub_i64(static_cast<int64_t>(a), static_cast<int64_t>(b)));
        case S_MUL_I64: return static_cast<uint64_t>(mul_i64(static_cast<int64_t>(a), static_cast<int64_t>(b)));
        case S_DIV_I64: {
            int64_t q;
            if (!div_i64(static_cast<int64_t>(a), static_cast<int64_t>(b), &q)) *ok = false;
            return static_cast<uint64_t>(q);
        }
        case S_ADD_F64: return f64_bits(add_f64(bits_f64(a), bits_f64(b)));
        case S_SUB_F64: return f64_bits(sub_f64(bits_f64(a), bits_f64(b)));
        case S_MUL_F64: return f64_bits(mul_f64(bits_f64(a), bits_f64(b)));
        default: return f64_bits(div_f64(bits_f64(a), bits_f64(b)));
    }
}

}  // namespace rvarith
