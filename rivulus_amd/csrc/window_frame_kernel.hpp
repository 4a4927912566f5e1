// Window frames (window_frame.hip): aggregates over bounded and unbounded ROWS frames, FIRST_VALUE / LAST_VALUE and NTILE over the
// sequence of window_kernel.hpp.  The semantics are those of include/rivulus_gpu.h (rv_window_frames) and DESIGN.md section 4 K12a; the
// case rule is window_frame_rule.hpp, the combine window_combine.hpp, the workgroup scan and the carry scan window_kernel.hpp's.
//
// Everything but the first read and the last store runs over consecutive addresses in SEQUENCE order:
//   window_frame_gather       (perm != nullptr only) one lane per position j: the cell at perm[j] to cells[j], its validity one ballot per wave
//   window_frame_scan         K12's segmented scan in its three launches (tile_agg, window_carry_scan, apply) over scan index i, which is
//                             position i (forward) or position n - 1 - i (mirrored); it keeps the scanned value AND the count per position.
//                             WFS_HEAD_POS / WFS_TAIL_POS: the partition geometry -- a MAX scan of (partition head ? j : 0) and the mirrored
//                             MIN scan of (partition tail ? j : ~0), no flags, 32-bit results.  WFS_CELL / WFS_VALID: the block prefix
//                             (forward, heads = block heads) and the block suffix (mirrored, heads = block tails: the position before a
//                             block head, and n - 1) of a value column.
//   window_frame_block_heads  one lane per position: partition head, or (j - head_pos[j]) % w == 0; one ballot per wave
//                             (a call without partition keys has ONE partition: no geometry is scanned, head_pos is 0 and tail_pos n - 1)
//   window_frame              one lane per position: lo / hi of its frame from head_pos / tail_pos, the case, the one final (+), the
//                             finish, and the store at out[perm[j]] -- the one scatter per output
// No kernel waits for another workgroup.
//
// THE BRACKETING of a Float64 SUM.  prefix[hi] is bracketed as window_kernel.hpp states it, with the block heads in the place of the
// partition heads.  suffix[lo] is its mirror: the same construction over scan index i = n - 1 - j, so a thread folds its 8 positions from
// the highest down, and a (+) b stands for a AFTER b in the sequence.  A frame inside one block is prefix[hi] or suffix[lo] as it stands;
// across two blocks it is the ONE further addition suffix[lo] + prefix[hi].
#pragma once

#include "window_frame_rule.hpp"
#include "window_kernel.hpp"

namespace rvk {

// a value column in sequence order: cell j at values[offset + j], its validity at bit offset + j
struct WfCells {
    const uint64_t *values;   // not read by WFS_VALID
    const uint8_t *validity;  // nullptr: no null cell
    uint64_t offset;
    uint32_t all_null;        // a NullArray
    uint32_t pad;
};

__device__ __forceinline__ bool wf_valid(const WfCells &c, uint64_t j) {
    if (c.all_null) return false;
    const uint64_t at = c.offset + j;
    return !c.validity || ((c.validity[at >> 3] >> (at & 7)) & 1);
}

// ---- gather ------------------------------------------------------------------------------------------------------------------------
struct WfGatherParams {
    const uint64_t *perm;
    DevCol col;
    uint64_t n;
    uint64_t *cells;     // [n]; nullptr: validity only (a column that is only counted)
    uint64_t *validity;  // (n + 63) / 64 words; nullptr: the column has no null cell
};

static __global__ __launch_bounds__(kWinThreads) void window_frame_gather(const WfGatherParams p) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kWinThreads + threadIdx.x;
    const bool in = j < p.n;
    bool valid = false;
    if (in) {
        const uint64_t at = p.col.offset + p.perm[j];
        valid = !p.col.validity || ((p.col.validity[at >> 3] >> (at & 7)) & 1);
        if (p.cells) p.cells[j] = static_cast<const uint64_t *>(p.col.values)[at];
    }
    if (p.validity) {
        const uint64_t m = ballot64(valid);
        if (lane_id() == 0 && in) p.validity[j >> 6] = m;
    }
}

// ---- scan --------------------------------------------------------------------------------------------------------------------------
enum : uint32_t {
    WFS_CELL = 0,      // the cell, the identity under a null; count: the cell is non-null
    WFS_VALID = 1,     // value 0; count: the cell is non-null                       (COUNT over a column that is no number)
    WFS_HEAD_POS = 2,  // j at a partition head, else 0; no flag (under WC_MAX_U64)   -> out32[j] = head_pos[j]
    WFS_TAIL_POS = 3,  // j at a partition tail, else ~0; no flag (WC_MIN_U64, mirrored) -> out32[j] = tail_pos[j]
};

struct WfScanParams {
    WfCells cells;
    const uint64_t *heads;  // the segment heads (forward) whose predecessors are the segment tails (mirrored); WFS_*_POS: the partition heads
    uint64_t n;
    uint64_t ntiles;
    uint32_t src;
    uint32_t mirrored;
    uint32_t is_float, is_max;
    WinTriple *tile_agg, *carry;  // [ntiles]
    uint64_t *out_value;          // [n] by position; nullptr: not kept
    uint32_t *out32;              // [n] by position: the count (WFS_CELL / WFS_VALID) or the value (WFS_*_POS)
};

// a segment ends at j
__device__ __forceinline__ bool wf_tail_bit(const uint64_t *heads, uint64_t j, uint64_t n) { return j + 1 == n || win_bit(heads, j + 1); }

template <uint32_t OP>
__device__ __forceinline__ WinTriple wf_element(const WfScanParams &p, uint64_t i) {
    WinTriple e = rvwin::identity_triple<OP>();
    if (i >= p.n) return e;
    const uint64_t j = p.mirrored ? p.n - 1 - i : i;
    if (p.src == WFS_HEAD_POS) {
        e.value = win_bit(p.heads, j) ? j : 0;
        return e;
    }
    if (p.src == WFS_TAIL_POS) {
        e.value = wf_tail_bit(p.heads, j, p.n) ? j : ~0ull;
        return e;
    }
    e.flag = p.mirrored ? wf_tail_bit(p.heads, j, p.n) : win_bit(p.heads, j);
    const bool valid = wf_valid(p.cells, j);
    e.count = valid ? 1 : 0;
    if (p.src == WFS_VALID) e.value = 0;
    else if (valid) {
        const uint64_t bits = p.cells.values[p.cells.offset + j];
        if (OP == rvwin::WC_ADD_F64) e.value = (bits << 1) == 0 ? 0 : bits;  // a zero of either sign adds +0.0
        else if (OP == rvwin::WC_ADD_I64) e.value = bits;
        else e.value = agg_order_key(bits, p.is_float != 0, p.is_max != 0);
    }
    return e;
}

// (a) one workgroup per tile of scan indices: its aggregate.  (b) is window_carry_scan.
template <uint32_t OP>
static __global__ __launch_bounds__(kWinThreads) void window_frame_tile_agg(const WfScanParams p) {
    __shared__ WinTriple s_wave[kWinThreads / 64];
    const uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * kWinTileRows + threadIdx.x * kWinItems;
    WinTriple acc = rvwin::identity_triple<OP>();
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) acc = rvwin::combine<OP>(acc, wf_element<OP>(p, i0 + k));
    WinTriple excl, total;
    win_block_scan<OP>(acc, excl, total, s_wave);
    if (threadIdx.x == 0) p.tile_agg[blockIdx.x] = total;
}

// (c) one workgroup per tile: the scanned value and count of every position, stored by position
template <uint32_t OP>
static __global__ __launch_bounds__(kWinThreads) void window_frame_apply(const WfScanParams p) {
    __shared__ WinTriple s_wave[kWinThreads / 64];
    const uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * kWinTileRows + threadIdx.x * kWinItems;
    WinTriple e[kWinItems];
    WinTriple acc = rvwin::identity_triple<OP>();
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
        e[k] = wf_element<OP>(p, i0 + k);
        acc = rvwin::combine<OP>(acc, e[k]);
    }
    WinTriple excl, total;
    win_block_scan<OP>(acc, excl, total, s_wave);
    acc = rvwin::combine<OP>(p.carry[blockIdx.x], excl);
    const bool geometry = p.src == WFS_HEAD_POS || p.src == WFS_TAIL_POS;
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
        acc = rvwin::combine<OP>(acc, e[k]);
        const uint64_t i = i0 + k;
        if (i >= p.n) continue;
        const uint64_t j = p.mirrored ? p.n - 1 - i : i;
        if (p.out_value) p.out_value[j] = acc.value;
        p.out32[j] = static_cast<uint32_t>(geometry ? acc.value : acc.count);
    }
}

// ---- block heads -------------------------------------------------------------------------------------------------------------------
struct WfBlockHeadsParams {
    const uint64_t *part_heads;
    const uint32_t *head_pos;  // nullptr: one partition, every head_pos is 0
    uint64_t n;
    uint32_t width;  // 1 <= width < n
    uint32_t pad;
    uint64_t *block_heads;  // (n + 63) / 64 words
};

static __global__ __launch_bounds__(kWinThreads) void window_frame_block_heads(const WfBlockHeadsParams p) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kWinThreads + threadIdx.x;
    const bool in = j < p.n;
    const bool head = in && rvframe::block_head(static_cast<uint32_t>(j) - (p.head_pos ? p.head_pos[j] : 0u), p.width);  // a partition head is its block 0's
    const uint64_t m = ballot64(head);
    if (lane_id() == 0 && in) p.block_heads[j >> 6] = m;
}

// ---- combine -----------------------------------------------------------------------------------------------------------------------
enum : uint32_t {
    WFO_COUNT = 0,   // the frame's non-null cells
    WFO_VALUE = 1,   // SUM: the value as it stands
    WFO_MINMAX = 2,  // agg_order_value(value), null when the count is 0
    WFO_AVG = 3,     // value / count (one IEEE division; an Int64 sum converted first), null when the count is 0
    WFO_FIRST = 4,   // the row index at the frame's first position, ~0 for an empty frame (a nullable index list)
    WFO_LAST = 5,    // ... at its last position
    WFO_NTILE = 6,   // the row's bucket of `buckets`
};

struct WfCombineParams {
    const uint64_t *perm;  // nullptr: the identity
    const uint32_t *head_pos, *tail_pos;  // both nullptr: one partition, 0 and n - 1
    uint64_t n;
    rvframe::Frame frame;
    const uint64_t *prefix_value, *suffix_value;  // by position; the side a frame never needs is nullptr
    const uint32_t *prefix_count, *suffix_count;
    uint32_t fin;       // WFO_*
    uint32_t op;        // rvwin::WC_* of the scans
    uint32_t is_float;  // the column is Float64
    uint32_t pad;
    uint64_t buckets;             // WFO_NTILE
    uint64_t *out;                // [n], row order
    uint64_t *out_validity;       // WFO_MINMAX / WFO_AVG: (n + 63) / 64 words, zeroed when perm != nullptr
    unsigned long long *nulls;    // ... and the striped counter of the null results
};

__device__ __forceinline__ uint64_t wf_apply_op(uint32_t op, uint64_t a, uint64_t b) {
    if (op == rvwin::WC_ADD_F64) return rvwin::apply<rvwin::WC_ADD_F64>(a, b);
    if (op == rvwin::WC_MIN_U64) return rvwin::apply<rvwin::WC_MIN_U64>(a, b);
    if (op == rvwin::WC_MAX_U64) return rvwin::apply<rvwin::WC_MAX_U64>(a, b);
    return rvwin::apply<rvwin::WC_ADD_I64>(a, b);
}

static __global__ __launch_bounds__(kWinThreads) void window_frame(const WfCombineParams p) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kWinThreads + threadIdx.x;
    unsigned long long nulls = 0;
    bool valid = false;
    if (j < p.n) {
        const uint64_t row = p.perm ? p.perm[j] : j;
        const uint32_t head = p.head_pos ? p.head_pos[j] : 0u, tail = p.tail_pos ? p.tail_pos[j] : static_cast<uint32_t>(p.n - 1);
        const uint32_t pos = static_cast<uint32_t>(j) - head + 1, len = tail - head + 1;
        uint64_t v = 0;
        if (p.fin == WFO_NTILE) v = rvframe::ntile_bucket(pos, len, p.buckets);
        else {
            const rvframe::Pick k = rvframe::frame_pick(p.frame, pos, len);
            const uint64_t lo = static_cast<uint64_t>(head) + k.lo - 1, hi = static_cast<uint64_t>(head) + k.hi - 1;  // positions of the sequence
            if (p.fin == WFO_FIRST || p.fin == WFO_LAST) {
                const uint64_t at = p.fin == WFO_FIRST ? lo : hi;
                v = k.which == rvframe::FC_EMPTY ? ~0ull : p.perm ? p.perm[at] : at;
            } else {
                uint64_t value = p.op == rvwin::WC_MIN_U64 ? ~0ull : 0ull, count = 0;
                if (k.which == rvframe::FC_PREFIX) value = p.prefix_value ? p.prefix_value[hi] : 0, count = p.prefix_count[hi];
                else if (k.which == rvframe::FC_SUFFIX) value = p.suffix_value ? p.suffix_value[lo] : 0, count = p.suffix_count[lo];
                else if (k.which == rvframe::FC_BOTH) {
                    value = p.prefix_value ? wf_apply_op(p.op, p.suffix_value[lo], p.prefix_value[hi]) : 0;
                    count = static_cast<uint64_t>(p.suffix_count[lo]) + p.prefix_count[hi];
                }
                if (p.fin == WFO_COUNT) v = count;
                else if (p.fin == WFO_VALUE) v = value;
                else if (count == 0) ++nulls;  // v = 0 under the null
                else {
                    if (p.fin == WFO_MINMAX) v = agg_order_value(value, p.is_float != 0);
                    else {
                        const double sum = p.is_float ? rvwin::bits_to_double(value) : static_cast<double>(static_cast<int64_t>(value));
                        v = rvwin::double_to_bits(sum / static_cast<double>(count));
                    }
                    valid = true;
                    if (p.perm) atomicOr(reinterpret_cast<unsigned long long *>(&p.out_validity[row >> 6]), 1ull << (row & 63));
                }
            }
        }
        p.out[row] = v;
    }
    if (p.fin == WFO_MINMAX || p.fin == WFO_AVG) {
        if (!p.perm) {  // in place the wave's 64 results are one word of the bitmap: one ballot, one store
            const uint64_t m = ballot64(valid);
            if (lane_id() == 0 && j < p.n) p.out_validity[j >> 6] = m;
        }
        nulls = wave_sum64(nulls);
        if (lane_id() == 0 && nulls) striped_add(p.nulls, nulls);
    }
}

}  // namespace rvk
