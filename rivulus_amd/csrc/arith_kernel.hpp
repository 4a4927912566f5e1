// K8: one typed postfix program of + - * / over up to eight Int64 / Float64 columns and literals, evaluated for every row in one
// launch (rv_eval_arith).  The shape of the auxiliary kernels (aux_kernels.hpp): one lane per row, a wave per 64-row bitmap word,
// grid-stride over the words.  The cell rules are arith_cell.hpp's.
//
// The host resolves every type once, so the program is the same for every lane: its steps are read with a wave-uniform index from
// the kernel arguments (scalar loads) and every branch on a step is uniform.  A wave first loads its cells of EVERY column the
// program reads, and of every nullable one the byte that holds the lane's validity bit (any bit offset; a ballot makes the word),
// all of them in flight before the first is waited for, then walks the program.
//
// The operand stack is K named registers per row: a push or a pop moves every entry with static moves (2 x K v_mov), never an
// index computed at run time, which would put the stack into scratch memory.  The kernel is instantiated for K = 2, 4 and 8 --
// K bounds both the stack and the columns held in registers -- and a program runs on the smallest that holds it: `a + b` moves two
// entries per step, not eight.  The two small forms take R = 2 bitmap words (128 rows) per wave and step, so that twice the loads
// are in flight; the largest keeps to one, for its registers.
#pragma once

#include "arith_cell.hpp"
#include "device_common.hpp"

namespace rvk {

struct ArithStep {  // dwords and one qword: read through the scalar cache
    uint32_t op;    // rvarith::S_*
    uint32_t arg;   // S_PUSH_COL: slot in ArithParams::cols
    int64_t lit;    // S_PUSH_LIT: Int64 value / Float64 bits
};

struct ArithParams {
    DevCol cols[rvarith::kMaxCols];  // the columns the program reads, each once
    ArithStep steps[rvarith::kMaxTypedSteps];
    uint32_t ncols, nsteps;
    uint64_t *out_values;
    uint64_t *out_validity;  // nullptr: no column read is nullable and the program has no Int64 division
    unsigned long long *out_valid_pop;
    uint64_t n;
};

template <int K>
struct ArithStack {
    uint64_t s[K];  // s[0] is the top; only ever indexed by constants
    __device__ __forceinline__ void push(uint64_t v) {
#pragma unroll
        for (int k = K - 1; k > 0; --k) s[k] = s[k - 1];
        s[0] = v;
    }
    // the two top entries replaced by r
    __device__ __forceinline__ void fold(uint64_t r) {
        s[0] = r;
#pragma unroll
        for (int k = 1; k < K - 1; ++k) s[k] = s[k + 1];
    }
};

// x, as a value the optimizer has to hold in registers here (device_common.hpp, opaque)
__device__ __forceinline__ uint64_t arith_keep(uint64_t x) {
    uint32_t lo = static_cast<uint32_t>(x), hi = static_cast<uint32_t>(x >> 32);
    asm volatile("" : "+v"(lo), "+v"(hi));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}
// Element `slot` of a register array, slot wave-uniform: a chain of uniform branches.  Left to itself the optimizer folds the chain
// into ONE access at a run-time index, moves the array to LDS for it, and every column's load then waits for its ds_write before the
// next is issued; arith_keep makes each element a register value of its own first.
template <int K>
__device__ __forceinline__ uint64_t arith_pick(const uint64_t (&v)[K], uint32_t slot) {
    uint64_t x = arith_keep(v[0]);
#pragma unroll
    for (int k = 1; k < K; ++k)
        if (slot == static_cast<uint32_t>(k)) x = arith_keep(v[k]);
    return x;
}

// rows of one wave and step: R words of 64
template <int K>
constexpr int arith_words() {
    return K == 8 ? 1 : 2;
}

template <int K>
static __global__ __launch_bounds__(256) void arith_kernel(const ArithParams p) {
    constexpr int R = arith_words<K>();
    const int lane = lane_id();
    const uint64_t nchunks = (p.n + 63) / 64;
    const uint64_t wave0 = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = (static_cast<uint64_t>(gridDim.x) * blockDim.x) >> 6;
    unsigned long long pop = 0;
    for (uint64_t g = wave0; g * R < nchunks; g += nwaves) {
        // Every load of the step is issued before anything waits for one: no branch on a lane's row (rows past the end re-read the
        // last row, which exists -- n >= 1 -- and are masked afterwards), and a nullable column's validity is the lane's own bit
        // (byte (offset + row) / 8 of a bitmap that covers offset + n bits) rather than load_bits64's word, whose tail branch and
        // immediate use made every column wait for the one before (1.4x the time of `a * b + c` with two nullable inputs)
        uint64_t v[R][K], row[R];
        uint32_t vbyte[R][K];
        bool in[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t i = (g * R + r) * 64 + lane;
            in[r] = i < p.n;
            row[r] = in[r] ? i : p.n - 1;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                v[r][k] = 0;
                vbyte[r][k] = 0xFFu;
            }
            if (static_cast<uint32_t>(k) < p.ncols) {
                const DevCol &col = p.cols[k];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint64_t e = col.offset + row[r];
                    v[r][k] = static_cast<const uint64_t *>(col.values)[e];
                    if (col.validity) vbyte[r][k] = col.validity[e >> 3];
                }
            }
        }
        uint64_t M[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            bool valid = in[r];
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (static_cast<uint32_t>(k) < p.ncols) valid = valid && ((vbyte[r][k] >> ((p.cols[k].offset + row[r]) & 7)) & 1);
            M[r] = ballot64(valid);
        }
        ArithStack<K> st[R];
        bool ok[R];  // no Int64 division by zero so far
#pragma unroll
        for (int r = 0; r < R; ++r) {
            ok[r] = true;
#pragma unroll
            for (int k = 0; k < K; ++k) st[r].s[k] = 0;
        }
        for (uint32_t k = 0; k < p.nsteps; ++k) {
            const uint32_t op = p.steps[k].op;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (op == rvarith::S_PUSH_COL) st[r].push(arith_pick<K>(v[r], p.steps[k].arg));
                else if (op == rvarith::S_PUSH_LIT) st[r].push(static_cast<uint64_t>(p.steps[k].lit));
                else if (op == rvarith::S_I2F_TOP) st[r].s[0] = rvarith::f64_bits(rvarith::i64_to_f64(static_cast<int64_t>(st[r].s[0])));
                else if (op == rvarith::S_I2F_SECOND) st[r].s[1] = rvarith::f64_bits(rvarith::i64_to_f64(static_cast<int64_t>(st[r].s[1])));
                else st[r].fold(rvarith::apply(op, st[r].s[1], st[r].s[0], &ok[r]));
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t c = g * R + r;
            const uint64_t valid = M[r] & ballot64(ok[r]);
            if (in[r]) p.out_values[c * 64 + lane] = ((valid >> lane) & 1) ? st[r].s[0] : 0;  // the placeholder under a null
            if (p.out_validity && lane == 0 && c < nchunks) {
                p.out_validity[c] = valid;
                pop += static_cast<unsigned long long>(__popcll(valid));
            }
        }
    }
    if (lane == 0 && pop) striped_add(p.out_valid_pop, pop);
}

}  // namespace rvk
