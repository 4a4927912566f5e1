// Window functions (window.hip): rank, running aggregates, lag / lead over PARTITION BY ... ORDER BY.  The reference has no window
// expression; the semantics are those of include/rivulus_gpu.h (rv_window) and DESIGN.md section 4 K12.
//
// Everything runs over the SEQUENCE: the rows in the order perm[0], perm[1], ... that puts every partition's rows side by side, each
// partition in its window order (perm == nullptr: the identity -- one partition in row order).  No kernel waits for another workgroup:
// every dependency between workgroups is a kernel boundary.
//   window_heads   one lane per position j: bit j of two LSB-first bitmaps, PARTITION HEAD (the partition id at perm[j] differs from the one
//                  at perm[j - 1], or j == 0) and PEER HEAD (partition head, or an order key tells the two rows apart).  A lane reads its
//                  predecessor's cells itself and the wave's 64 flags are one ballot: no LDS, no scratch.
//   window_scan    the segmented inclusive scan of rvwin::combine (window_combine.hpp) over the positions, in three launches over fixed
//                  tiles of kWinTileRows positions: window_tile_agg (every tile's aggregate), window_carry_scan (one workgroup: the
//                  exclusive scan of the tile aggregates, 2048 at a time, the running carry kept in registers), window_apply (carry, wave
//                  scan, workgroup combine, and the store at out[perm[j]]).
//   window_shift   LAG / LEAD: idx[perm[j]] = perm[j -/+ k] when that position exists and carries the same partition id, else the null
//                  index ~0 -- a nullable index list in row order that take_nullable_on_device gathers any dtype through.
//
// THE BRACKETING of the scan (what a Float64 CUM_SUM's bits follow from).  With (+) the combine, a (+) b for a before b:
//   thread t of a tile's 256 holds the positions 8 t .. 8 t + 7 of the tile and folds them left to right: T_t = ((e_0 (+) e_1) (+) ...) (+) e_7;
//   a wave's 64 thread aggregates are scanned by the steps d = 1, 2, 4, 8, 16, 32: lane l >= d replaces x_l by x_{l-d} (+) x_l, and
//   L_l is what lane l - 1 ends with (the identity for lane 0);
//   W_w is the left fold of the last lanes' results of the waves before wave w: ((id (+) w_0) (+) w_1) ...;
//   C_i, the carry into tile i, is made the same way out of the tile aggregates, 2048 tiles to a round: thread t folds tiles 8 t .. 8 t + 7
//   of the round, R (+) (W (+) L) is what the thread starts from, R the left fold of the rounds' totals before;
//   the result at the thread's k-th position is ((C_i (+) (W_w (+) L_l)) (+) e_0) (+) ... (+) e_k.
// Only the position in the sequence, the positions of the partition heads (where (+) drops its left side) and this geometry enter it.
// A null cell is the operator's identity (+0.0 for a sum) and a cell that is a zero of either sign enters as +0.0, so no sum is ever -0.0.
#pragma once

#include "device_common.hpp"
#include "group_agg_kernel.hpp"  // agg_order_key / agg_order_value: MIN / MAX and their NaN rule are K9's
#include "order_key.hpp"
#include "window_combine.hpp"

namespace rvk {

constexpr int kWinThreads = 256;
constexpr int kWinItems = 8;                               // consecutive positions per thread
constexpr int kWinTileRows = kWinThreads * kWinItems;      // 2048 positions per workgroup
constexpr int kWinOrderKeysMost = 8;

using WinTriple = rvwin::Triple;

// ---- heads -------------------------------------------------------------------------------------------------------------------------
struct WinHeadsParams {
    const uint64_t *perm;  // nullptr: the identity
    const int64_t *ids;    // partition id per ROW, nullptr: one partition
    uint64_t n;
    uint32_t norder;
    uint32_t pad;
    DevCol order[kWinOrderKeysMost];
    uint64_t *part_heads, *peer_heads;  // (n + 63) / 64 words each
};

// null-ness and the sort's key of a cell: what tells two rows apart in the window order (the bits under a null are not read)
__device__ __forceinline__ bool win_order_cell(const DevCol &c, uint64_t row, uint64_t &key) {
    key = 0;
    if (c.dtype == DT_NULL) return false;
    const uint64_t at = c.offset + row;
    if (c.validity && !((c.validity[at >> 3] >> (at & 7)) & 1)) return false;
    key = rvorder::sort_key(static_cast<const uint64_t *>(c.values)[at], c.dtype == DT_FLOAT64);
    return true;
}

static __global__ __launch_bounds__(kWinThreads) void window_heads(const WinHeadsParams p) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kWinThreads + threadIdx.x;
    const bool in = j < p.n;
    bool part = false, peer = false;
    if (in) {
        part = j == 0;
        if (j > 0) {
            const uint64_t row = p.perm ? p.perm[j] : j, before = p.perm ? p.perm[j - 1] : j - 1;
            if (p.ids) part = p.ids[row] != p.ids[before];
            for (uint32_t k = 0; k < p.norder && !peer; ++k) {
                uint64_t a, b;
                const bool va = win_order_cell(p.order[k], row, a), vb = win_order_cell(p.order[k], before, b);
                peer = va != vb || (va && a != b);
            }
        }
        peer = peer || part;
    }
    const uint64_t pm = ballot64(part), qm = ballot64(peer);
    if (lane_id() == 0 && in) {  // the wave's 64 positions are word j / 64 of both bitmaps
        p.part_heads[j >> 6] = pm;
        p.peer_heads[j >> 6] = qm;
    }
}

// ---- scan --------------------------------------------------------------------------------------------------------------------------
// what a position contributes (WinScanParams::src) ...
enum : uint32_t {
    WS_ONE = 0,       // 1                                              (ROW_NUMBER)
    WS_PEER = 1,      // its peer-head bit                              (DENSE_RANK)
    WS_PEER_POS = 2,  // value: j at a peer head, else 0; count: 1       (RANK, under WC_MAX_U64: the position of the last peer head)
    WS_VALID = 3,     // 1 for a non-null cell                          (CUM_COUNT)
    WS_CELL = 4,      // the cell, the identity under a null; count: the cell is non-null (CUM_SUM; MIN / MAX through agg_order_key)
};
// ... and what is stored of the scanned triple (WinScanParams::fin)
enum : uint32_t {
    WF_VALUE = 0,   // the value
    WF_RANK = 1,    // value - j + count: the last peer head's position within the partition, 1-based
    WF_MINMAX = 2,  // agg_order_value(value), or a null (0, validity bit clear) when count == 0
};

struct WinScanParams {
    const uint64_t *perm;  // nullptr: the identity
    const uint64_t *part_heads, *peer_heads;
    uint64_t n;
    uint64_t ntiles;
    DevCol col;
    uint32_t src, fin;
    uint32_t is_float, is_max;
    WinTriple *tile_agg, *carry;  // [ntiles]
    uint64_t *out;                // [n], row order
    uint64_t *out_validity;       // WF_MINMAX: zeroed, (n + 63) / 64 words
    unsigned long long *nulls;    // WF_MINMAX: striped counter of the null results
};

__device__ __forceinline__ uint32_t win_bit(const uint64_t *words, uint64_t j) { return static_cast<uint32_t>((words[j >> 6] >> (j & 63)) & 1); }

template <uint32_t OP>
__device__ __forceinline__ WinTriple win_element(const WinScanParams &p, uint64_t j) {
    WinTriple e = rvwin::identity_triple<OP>();
    if (j >= p.n) return e;
    e.flag = win_bit(p.part_heads, j);
    e.count = 1;
    if (p.src == WS_ONE) e.value = 1;
    else if (p.src == WS_PEER) e.value = win_bit(p.peer_heads, j);
    else if (p.src == WS_PEER_POS) e.value = win_bit(p.peer_heads, j) ? j : 0;
    else {
        const uint64_t row = p.perm ? p.perm[j] : j, at = p.col.offset + row;
        const bool valid = p.col.dtype != DT_NULL && (!p.col.validity || ((p.col.validity[at >> 3] >> (at & 7)) & 1));
        e.count = valid ? 1 : 0;
        if (p.src == WS_VALID) e.value = valid ? 1 : 0;
        else if (valid) {
            const uint64_t bits = static_cast<const uint64_t *>(p.col.values)[at];
            if (OP == rvwin::WC_ADD_F64) e.value = (bits << 1) == 0 ? 0 : bits;  // a zero of either sign adds +0.0
            else if (OP == rvwin::WC_ADD_I64) e.value = bits;
            else e.value = agg_order_key(bits, p.is_float != 0, p.is_max != 0);
        }
    }
    return e;
}

__device__ __forceinline__ WinTriple win_shfl_up(const WinTriple &x, int d) {
    WinTriple y;
    y.value = (static_cast<uint64_t>(static_cast<uint32_t>(__shfl_up(static_cast<int>(x.value >> 32), d, 64))) << 32) |
              static_cast<uint32_t>(__shfl_up(static_cast<int>(x.value), d, 64));
    y.count = (static_cast<uint64_t>(static_cast<uint32_t>(__shfl_up(static_cast<int>(x.count >> 32), d, 64))) << 32) |
              static_cast<uint32_t>(__shfl_up(static_cast<int>(x.count), d, 64));
    y.flag = static_cast<uint32_t>(__shfl_up(static_cast<int>(x.flag), d, 64));
    y.pad = 0;
    return y;
}

// the workgroup's exclusive scan of one triple per thread: excl = W (+) L of the header comment, total = the fold of the four waves.
// s_wave: 4 triples of LDS, free again when this returns.
template <uint32_t OP>
__device__ __forceinline__ void win_block_scan(const WinTriple &mine, WinTriple &excl, WinTriple &total, WinTriple *s_wave) {
    const int lane = lane_id(), wave = static_cast<int>(threadIdx.x >> 6);
    WinTriple x = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const WinTriple y = win_shfl_up(x, d);
        if (lane >= d) x = rvwin::combine<OP>(y, x);
    }
    const WinTriple before = win_shfl_up(x, 1);
    const WinTriple lane_excl = lane ? before : rvwin::identity_triple<OP>();
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    WinTriple w = rvwin::identity_triple<OP>(), wave_excl = w;
#pragma unroll
    for (int k = 0; k < kWinThreads / 64; ++k) {
        if (k == wave) wave_excl = w;
        w = rvwin::combine<OP>(w, s_wave[k]);
    }
    total = w;
    excl = rvwin::combine<OP>(wave_excl, lane_excl);
    __syncthreads();
}

// (a) one workgroup per tile: its aggregate
template <uint32_t OP>
static __global__ __launch_bounds__(kWinThreads) void window_tile_agg(const WinScanParams p) {
    __shared__ WinTriple s_wave[kWinThreads / 64];
    const uint64_t j0 = static_cast<uint64_t>(blockIdx.x) * kWinTileRows + threadIdx.x * kWinItems;
    WinTriple acc = rvwin::identity_triple<OP>();
#pragma unroll
    for (int i = 0; i < kWinItems; ++i) acc = rvwin::combine<OP>(acc, win_element<OP>(p, j0 + i));
    WinTriple excl, total;
    win_block_scan<OP>(acc, excl, total, s_wave);
    if (threadIdx.x == 0) p.tile_agg[blockIdx.x] = total;
}

// (b) ONE workgroup: carry[i] = the fold of the aggregates of the tiles before tile i, kWinTileRows aggregates to a round
template <uint32_t OP>
static __global__ __launch_bounds__(kWinThreads) void window_carry_scan(const WinTriple *tile_agg, uint64_t ntiles, WinTriple *carry) {
    __shared__ WinTriple s_wave[kWinThreads / 64];
    WinTriple run = rvwin::identity_triple<OP>();
    for (uint64_t base = 0; base < ntiles; base += kWinTileRows) {  // workgroup-uniform
        const uint64_t i0 = base + threadIdx.x * kWinItems;
        WinTriple a[kWinItems];
        WinTriple acc = rvwin::identity_triple<OP>();
#pragma unroll
        for (int i = 0; i < kWinItems; ++i) {
            a[i] = i0 + i < ntiles ? tile_agg[i0 + i] : rvwin::identity_triple<OP>();
            acc = rvwin::combine<OP>(acc, a[i]);
        }
        WinTriple excl, total;
        win_block_scan<OP>(acc, excl, total, s_wave);
        acc = rvwin::combine<OP>(run, excl);
#pragma unroll
        for (int i = 0; i < kWinItems; ++i) {
            if (i0 + i < ntiles) carry[i0 + i] = acc;
            acc = rvwin::combine<OP>(acc, a[i]);
        }
        run = rvwin::combine<OP>(run, total);
    }
}

// (c) one workgroup per tile: the results, stored in row order
template <uint32_t OP>
static __global__ __launch_bounds__(kWinThreads) void window_apply(const WinScanParams p) {
    __shared__ WinTriple s_wave[kWinThreads / 64];
    // in place (perm == nullptr) a thread's 8 results are 64 consecutive bytes, 64 lanes 64 bytes apart: staged here (9 words per thread:
    // the lanes' words fall on different banks) and stored by the whole workgroup, consecutive lanes consecutive words
    __shared__ uint64_t s_out[kWinThreads * (kWinItems + 1)];
    const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kWinTileRows;
    const uint64_t j0 = tile0 + threadIdx.x * kWinItems;
    WinTriple e[kWinItems];
    WinTriple acc = rvwin::identity_triple<OP>();
#pragma unroll
    for (int i = 0; i < kWinItems; ++i) {
        e[i] = win_element<OP>(p, j0 + i);
        acc = rvwin::combine<OP>(acc, e[i]);
    }
    WinTriple excl, total;
    win_block_scan<OP>(acc, excl, total, s_wave);
    acc = rvwin::combine<OP>(p.carry[blockIdx.x], excl);
    unsigned long long nulls = 0;
#pragma unroll
    for (int i = 0; i < kWinItems; ++i) {
        acc = rvwin::combine<OP>(acc, e[i]);
        const uint64_t j = j0 + i;
        if (j >= p.n) continue;
        const uint64_t row = p.perm ? p.perm[j] : j;
        uint64_t v = acc.value;
        if (p.fin == WF_RANK) v = acc.value - j + acc.count;
        else if (p.fin == WF_MINMAX) {
            if (acc.count) {
                v = agg_order_value(acc.value, p.is_float != 0);
                atomicOr(reinterpret_cast<unsigned long long *>(&p.out_validity[row >> 6]), 1ull << (row & 63));
            } else {
                v = 0;
                ++nulls;
            }
        }
        if (p.perm) p.out[row] = v;
        else s_out[threadIdx.x * (kWinItems + 1) + i] = v;
    }
    if (!p.perm) {  // workgroup-uniform
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kWinItems; ++i) {
            const uint32_t at = i * kWinThreads + threadIdx.x;  // the tile's position: thread at / 8, item at % 8
            if (tile0 + at < p.n) p.out[tile0 + at] = s_out[(at / kWinItems) * (kWinItems + 1) + at % kWinItems];
        }
    }
    if (p.fin == WF_MINMAX) {
        nulls = wave_sum64(nulls);
        if (lane_id() == 0 && nulls) striped_add(p.nulls, nulls);
    }
}

// ---- shift -------------------------------------------------------------------------------------------------------------------------
struct WinShiftParams {
    const uint64_t *perm;  // nullptr: the identity
    const int64_t *ids;    // nullptr: one partition
    uint64_t n;
    uint64_t k;
    uint32_t lead;         // 0: LAG (position j - k), 1: LEAD (j + k)
    uint32_t pad;
    uint64_t *idx;         // [n], row order; ~0: null
};

static __global__ __launch_bounds__(kWinThreads) void window_shift(const WinShiftParams p) {
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kWinThreads + threadIdx.x; j < p.n; j += static_cast<uint64_t>(gridDim.x) * kWinThreads) {
        const bool in_range = p.lead ? p.k < p.n - j : p.k <= j;
        const uint64_t row = p.perm ? p.perm[j] : j;
        uint64_t from = ~0ull;
        if (in_range) {
            const uint64_t s = p.lead ? j + p.k : j - p.k;
            const uint64_t src_row = p.perm ? p.perm[s] : s;
            if (!p.ids || p.ids[row] == p.ids[src_row]) from = src_row;
        }
        p.idx[row] = from;
    }
}

}  // namespace rvk
