// Grouped aggregation (group_agg.hip): group_by(key).agg(count / sum / min / max).  The reference has no aggregate operator; the
// semantics are those of include/rivulus_gpu.h (rv_hash_aggregate) and DESIGN.md section 4 K9.
//
// Layout of the group table (the string dictionary's, string_dict_kernel.hpp, with the key's 64 bits in place of a string's bytes):
//   slots  open addressing, a power of two >= 2 x min(rows, option "agg_max_groups"), linear probing; ONE 64-bit word per distinct
//          non-null key: hash_high32 << 32 | (row + 1), 0: empty.  The word is published by a single compare-and-swap, so no reader
//          ever sees half a slot; the key's bits are those of `row` in the key column.  The tag only spares key reads: a hit is a hit
//          once the bits are equal.  A slot's tag never changes once claimed and its row only ever falls (atomicMin: same tag, so the
//          smaller word is the smaller row), to the key's FIRST ROW -- which slot a key sits in may depend on the order the atomics
//          land in, its first row does not.
//   null   all null keys are one group (AnyValue: Null == Null, as in the join): its first row is one word next to the table.
// A group's POSITION in the output is the rank of its first row among all first rows: group_mark_first sets bit `first row` of a
// bitmap of the key's rows, the selection scan (strings.hip) counts the bits per word, and position = bits below the first row.
// Nothing of the result depends on which lane or workgroup came first.  Every chain walk is bounded by the slot count.
#pragma once

#include "device_common.hpp"
#include "join_kernel.hpp"  // join_hash: murmur3's 64-bit finaliser
#include "order_key.hpp"    // the order map MIN / MAX share with the sort

namespace rvk {

constexpr int kGroupAggThreads = 256;
constexpr int kGroupAggRowsPerThread = 8;                                    // rows per lane of an accumulate tile, kGroupAggThreads apart
constexpr int kGroupAggTileRows = kGroupAggThreads * kGroupAggRowsPerThread;  // 2048 rows per workgroup and step
constexpr int kAggOpsMost = 4;                                               // accumulators of one accumulate launch

struct GroupTableView {
    unsigned long long *slots;
    unsigned long long *null_first;  // row of the first null key, ~0: none
    uint64_t slot_mask;              // slots - 1
    uint64_t hash_mask;              // ~0, or the low bits option "agg_hash_bits" leaves (collision tests)
    DevCol key;                      // DT_INT64 (or DT_NULL: no table, every row is in the null group)
    uint64_t n;
};

__device__ __forceinline__ bool group_key(const DevCol &c, uint64_t i, uint64_t &bits) {
    bits = 0;
    if (c.dtype == DT_NULL) return false;
    const uint64_t at = c.offset + i;
    if (c.validity && !((c.validity[at >> 3] >> (at & 7)) & 1)) return false;
    bits = static_cast<const uint64_t *>(c.values)[at];
    return true;
}

struct GroupInsertParams {
    GroupTableView t;
    unsigned long long *distinct;  // striped counter of the slots claimed
    unsigned long long *claimed;   // one word, or nullptr: rows <= agg_max_groups, the table cannot fill
    uint64_t max_groups;
    uint32_t *error;               // bit 0: a chain walk exhausted the table; bit 1: more keys than max_groups, claiming has stopped
};

// One lane per row.  A row whose key equals the previous lane's leaves the insert to the head of its run (the head has the smaller
// row): a one-group or a sorted key column costs one probe per run and wave, not 64 on one address.  A lane that finds its key under
// a smaller row does nothing (no atomic).  With `claimed` set, a wave adds the slots it claimed to that word and raises error bit 1
// once the sum passes max_groups; every lane looks at the flag before it starts and every 64 steps of a walk, so an overfull table is
// left alone instead of walked end to end.
static __global__ __launch_bounds__(kGroupAggThreads) void group_insert(const GroupInsertParams q) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kGroupAggThreads + threadIdx.x;
    const int lane = lane_id();
    uint64_t bits = 0;
    const bool in = i < q.t.n;
    const bool keyed = in && group_key(q.t.key, i, bits);
    const bool isnull = in && !keyed;
    const uint64_t nm = ballot64(isnull);
    if (nm && lane == __ffsll(static_cast<long long>(nm)) - 1) {  // the wave's first null row
        if (__hip_atomic_load(q.t.null_first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i) atomicMin(q.t.null_first, i);
    }
    const uint64_t prev_bits = shfl64(bits, lane > 0 ? lane - 1 : 0);
    const uint64_t km = ballot64(keyed);
    const bool head = keyed && !(lane > 0 && ((km >> (lane - 1)) & 1) && prev_bits == bits);
    bool claimed = false;
    const bool stopped = q.claimed && (__hip_atomic_load(q.error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2u);
    if (head && !stopped) {
        const uint64_t h = join_hash(bits) & q.t.hash_mask;
        const unsigned long long mine = (h & 0xFFFFFFFF00000000ull) | (i + 1);
        uint64_t s = h & q.t.slot_mask;
        bool placed = false;
        for (uint64_t step = 0; step <= q.t.slot_mask && !placed; ++step, s = (s + 1) & q.t.slot_mask) {
            if (q.claimed && (step & 63) == 63 && (__hip_atomic_load(q.error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2u)) {
                placed = true;  // claiming has stopped: the call fails whatever this row would have found
                break;
            }
            unsigned long long e = __hip_atomic_load(&q.t.slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (e == 0) {
                e = atomicCAS(&q.t.slots[s], 0ull, mine);
                if (e == 0) {
                    claimed = placed = true;
                    break;
                }
                // lost the slot: another row of the SAME key may have taken it -- look at what it holds now
            }
            if ((e >> 32) == (mine >> 32) && static_cast<const uint64_t *>(q.t.key.values)[q.t.key.offset + static_cast<uint32_t>(e) - 1] == bits) {
                if (mine < e) atomicMin(&q.t.slots[s], mine);
                placed = true;
            }
        }
        if (!placed) atomicOr(q.error, 1u);
    }
    const uint64_t m = ballot64(claimed);
    if (lane == 0 && m) {
        const unsigned long long c = __popcll(m);
        striped_add(q.distinct, c);
        if (q.claimed && atomicAdd(q.claimed, c) + c > q.max_groups) atomicOr(q.error, 2u);
    }
}

// One lane per slot (and one for the null group): bit `first row` of `marks` (zeroed, one bit per key row).
static __global__ __launch_bounds__(kGroupAggThreads) void group_mark_first(const GroupTableView t, uint64_t nslots, unsigned long long *marks) {
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kGroupAggThreads + threadIdx.x; s <= nslots; s += static_cast<uint64_t>(gridDim.x) * kGroupAggThreads) {
        const unsigned long long e = s < nslots ? t.slots[s] : *t.null_first + 1;  // (~0 + 1 == 0: no null group)
        if (e == 0) continue;
        const uint64_t row = static_cast<uint32_t>(e) - 1;
        atomicOr(&marks[row >> 6], 1ull << (row & 63));
    }
}

// the first row of the group of row i (every key is in the table: the insert ran over the same column)
__device__ __forceinline__ uint64_t group_first_row(const GroupTableView &t, uint64_t i, uint32_t *error) {
    uint64_t bits;
    if (!group_key(t.key, i, bits)) return *t.null_first;
    const uint64_t h = join_hash(bits) & t.hash_mask;
    const uint32_t tag = static_cast<uint32_t>(h >> 32);
    uint64_t s = h & t.slot_mask;
    for (uint64_t step = 0; step <= t.slot_mask; ++step, s = (s + 1) & t.slot_mask) {
        const unsigned long long e = t.slots[s];
        if (e == 0) break;
        const uint64_t row = static_cast<uint32_t>(e) - 1;
        if (static_cast<uint32_t>(e >> 32) == tag && static_cast<const uint64_t *>(t.key.values)[t.key.offset + row] == bits) return row;
    }
    atomicOr(error, 1u);
    return 0;
}

// One lane per row: the position of the row's group = first rows below the group's own (excl: marks' set bits before each word).
template <typename ID>
static __global__ __launch_bounds__(kGroupAggThreads) void group_ids(const GroupTableView t, const uint64_t *marks, const uint64_t *excl, ID *gids, uint32_t *error) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kGroupAggThreads + threadIdx.x;
    if (i >= t.n) return;
    const uint64_t fr = group_first_row(t, i, error);
    gids[i] = static_cast<ID>(excl[fr >> 6] + __popcll(marks[fr >> 6] & low_mask(fr & 63)));
}

// ---- accumulate ------------------------------------------------------------------------------------------------------------------
// Every accumulator is one uint64 per group, combined by an INTEGER operation that is associative and commutative: the result is
// exact and the same on every run, whatever order lanes, waves and workgroups arrive in.
//   AK_COUNT_ROWS  + 1 per row                         AK_COUNT  + 1 per non-null cell
//   AK_SUM_I64     + the cell (two's complement wrap)
//   AK_MIN / AK_MAX  unsigned min / max of the cell's ORDER KEY (agg_order_key): Int64 with the sign bit flipped; Float64 as the
//                    total order -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN, with every NaN moved to the end that wins
//                    (0 for MIN, ~0 for MAX) so that one NaN makes the group NaN.  Whether the group had a non-null cell at all
//                    comes from an AK_COUNT accumulator next to it (group_minmax_finish).
enum : uint32_t { AK_COUNT_ROWS = 0, AK_COUNT = 1, AK_SUM_I64 = 2, AK_MIN = 3, AK_MAX = 4 };

struct AggAcc {
    unsigned long long *acc;  // [groups]; AK_MIN: initialised to ~0, every other kind to 0
    uint32_t kind;
    uint32_t col;             // index into GroupAccParams::cols (ignored by AK_COUNT_ROWS)
};

struct GroupAccParams {
    const uint32_t *gids;
    uint64_t n;
    uint32_t groups;
    uint32_t nacc;
    AggAcc acc[kAggOpsMost];
    DevCol cols[kAggOpsMost];
};

__host__ __device__ __forceinline__ uint64_t agg_order_key(uint64_t bits, bool is_float, bool is_max) {
    if (is_float && rvorder::order_key_is_nan(bits)) return is_max ? ~0ull : 0ull;
    return rvorder::order_key(bits, is_float);
}
__host__ __device__ __forceinline__ uint64_t agg_order_value(uint64_t key, bool is_float) {
    if (is_float && (key == 0 || key == ~0ull)) return 0x7FF8000000000000ull;  // a NaN won
    return rvorder::order_value(key, is_float);
}

__device__ __forceinline__ uint64_t agg_identity(uint32_t kind) { return kind == AK_MIN ? ~0ull : 0ull; }
__device__ __forceinline__ uint64_t agg_combine(uint32_t kind, uint64_t a, uint64_t b) {
    return kind == AK_MIN ? (a < b ? a : b) : kind == AK_MAX ? (a > b ? a : b) : a + b;
}
__device__ __forceinline__ void agg_atomic(uint32_t kind, unsigned long long *at, unsigned long long v) {
    if (kind == AK_MIN) atomicMin(at, v);
    else if (kind == AK_MAX) atomicMax(at, v);
    else atomicAdd(at, v);
}

// what row i gives accumulator a (the kind's identity for a null cell)
__device__ __forceinline__ uint64_t agg_cell(const AggAcc &a, const DevCol &c, uint64_t i) {
    if (a.kind == AK_COUNT_ROWS) return 1;
    if (c.dtype == DT_NULL) return agg_identity(a.kind);
    const uint64_t at = c.offset + i;
    if (c.validity && !((c.validity[at >> 3] >> (at & 7)) & 1)) return agg_identity(a.kind);
    if (a.kind == AK_COUNT) return 1;
    const uint64_t bits = static_cast<const uint64_t *>(c.values)[at];
    if (a.kind == AK_SUM_I64) return bits;
    return agg_order_key(bits, c.dtype == DT_FLOAT64, a.kind == AK_MAX);
}

// One kernel over (gid, value columns), 2048 rows per workgroup and step, grid-strided.  In every step a wave holds 64 consecutive
// rows; lanes next to each other with the same group are a RUN, and a segmented wave scan leaves each run's combined value in its
// last lane, which alone issues the atomic: one group, or sorted keys, cost one atomic per wave and accumulator instead of 64 on one
// address (steps whose neighbours all differ skip the scan).
//   LDS = true   groups <= rvt::kGroupAggLdsGroupsMost: the workgroup's own accumulators in LDS (nacc x groups words, dynamic), LDS
//                integer atomics per run, then one global integer atomic per group, accumulator and workgroup that touched it;
//   LDS = false  global integer atomics per run.
template <bool LDS>
static __global__ __launch_bounds__(kGroupAggThreads) void group_accumulate(const GroupAccParams p) {
    extern __shared__ unsigned long long s_acc[];
    const int lane = lane_id();
    if (LDS) {
        for (uint32_t k = 0; k < p.nacc; ++k) {
            const uint64_t id = agg_identity(p.acc[k].kind);
            for (uint32_t g = threadIdx.x; g < p.groups; g += kGroupAggThreads) s_acc[k * p.groups + g] = id;
        }
        __syncthreads();
    }
    const uint64_t ntiles = (p.n + kGroupAggTileRows - 1) / kGroupAggTileRows;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int r = 0; r < kGroupAggRowsPerThread; ++r) {
            const uint64_t i = tile * kGroupAggTileRows + static_cast<uint64_t>(r) * kGroupAggThreads + threadIdx.x;
            const bool in = i < p.n;
            const uint32_t g = in ? p.gids[i] : 0xFFFFFFFFu;
            const uint32_t gprev = static_cast<uint32_t>(__shfl(static_cast<int>(g), lane > 0 ? lane - 1 : 0, 64));
            const uint32_t gnext = static_cast<uint32_t>(__shfl(static_cast<int>(g), lane < 63 ? lane + 1 : 63, 64));
            const bool head = lane == 0 || gprev != g;
            const bool tail = lane == 63 || gnext != g;
            const uint64_t heads = ballot64(head);
            const bool runs = heads != ~0ull;  // wave-uniform
            for (uint32_t k = 0; k < p.nacc; ++k) {
                const uint32_t kind = p.acc[k].kind;
                uint64_t v = in ? agg_cell(p.acc[k], p.cols[p.acc[k].col], i) : agg_identity(kind);
                if (runs) {
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const uint64_t y = shfl64(v, lane >= d ? lane - d : 0);
                        // lane - d is in this lane's run: no head in (lane - d, lane]
                        if (lane >= d && ((heads >> (lane - d + 1)) & low_mask(d)) == 0) v = agg_combine(kind, v, y);
                    }
                }
                if (in && tail && v != agg_identity(kind)) {
                    if (LDS) agg_atomic(kind, &s_acc[k * p.groups + g], v);
                    else agg_atomic(kind, &p.acc[k].acc[g], v);
                }
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t k = 0; k < p.nacc; ++k) {
            const uint32_t kind = p.acc[k].kind;
            for (uint32_t g = threadIdx.x; g < p.groups; g += kGroupAggThreads) {
                const unsigned long long v = s_acc[k * p.groups + g];
                if (v != agg_identity(kind)) agg_atomic(kind, &p.acc[k].acc[g], v);
            }
        }
    }
}

// MIN / MAX in place: acc[g] = the winning cell's bits (0 under a null), bit g of `validity` = the group had a non-null cell (whole
// words are written: 64 groups per wave), the nulls counted into the striped counter `nulls`.
static __global__ __launch_bounds__(kGroupAggThreads) void group_minmax_finish(unsigned long long *acc, const unsigned long long *counts, uint64_t groups,
                                                                                int is_float, uint64_t *validity, unsigned long long *nulls) {
    const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kGroupAggThreads + threadIdx.x;
    const bool in = g < groups;
    const bool valid = in && counts[g] != 0;
    if (in) acc[g] = valid ? agg_order_value(acc[g], is_float != 0) : 0ull;
    const uint64_t m = ballot64(valid), all = ballot64(in);
    if (lane_id() == 0 && all) {
        validity[g >> 6] = m;
        if (m != all) striped_add(nulls, __popcll(all & ~m));
    }
}

// ---- Float64 SUM: no atomics --------------------------------------------------------------------------------------------------------
// `rows` holds every row of the key column grouped by group id, each group's rows ascending (a stable radix sort of (gid, row));
// starts[g] is where group g's list begins, starts[groups] = n.
static __global__ __launch_bounds__(kGroupAggThreads) void group_list_starts(const uint32_t *sorted_gids, uint64_t n, uint32_t groups, uint64_t *starts) {
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kGroupAggThreads + threadIdx.x; j <= n; j += static_cast<uint64_t>(gridDim.x) * kGroupAggThreads) {
        if (j == n) starts[groups] = n;
        else if (j == 0 || sorted_gids[j - 1] != sorted_gids[j]) starts[sorted_gids[j]] = j;
    }
}

__device__ __forceinline__ double group_f64_cell(const DevCol &c, uint32_t row) {
    const uint64_t at = c.offset + row;
    if (c.validity && !((c.validity[at >> 3] >> (at & 7)) & 1)) return 0.0;  // a null adds +0.0: whatever lies under it never shows
    return static_cast<const double *>(c.values)[at];
}

// The segmented sum.  The order of the additions of a group follows from the LENGTH L of its list (all its rows, null cells
// included, each adding +0.0) and from every row's POSITION j in that list, and from nothing else:
//   L <= list_wave_most  one wave: lane l adds the cells at positions l, l + 64, l + 128, ... in that order, starting from +0.0; the
//                        64 partial sums meet in the xor butterfly of wave_sum_f64 (32, 16, ..., 1);
//   longer               the workgroup: thread t (of 256) adds positions t, t + 256, ...; each of the 4 waves runs the same
//                        butterfly, and the wave sums are added as (w0 + w1) + (w2 + w3).
// The result is +0.0 + that sum: never -0.0, and +0.0 for a group without a non-null cell.  A workgroup takes 4 consecutive groups:
// first each wave its own short one, then all four waves each long one in turn.
static __global__ __launch_bounds__(kGroupAggThreads) void group_f64_sum(const DevCol col, const uint32_t *rows, const uint64_t *starts, uint32_t groups,
                                                                          uint32_t list_wave_most, double *out) {
    __shared__ double s_wave[4];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * 4;
    {
        const uint64_t g = g0 + wave;
        if (g < groups) {
            const uint64_t b = starts[g], e = starts[g + 1];
            if (e - b <= list_wave_most) {
                double v = 0.0;
                for (uint64_t j = b + lane; j < e; j += 64) v += group_f64_cell(col, rows[j]);
                v = wave_sum_f64(v);
                if (lane == 0) out[g] = 0.0 + v;
            }
        }
    }
    for (int k = 0; k < 4; ++k) {
        const uint64_t g = g0 + k;
        if (g >= groups) break;  // workgroup-uniform
        const uint64_t b = starts[g], e = starts[g + 1];
        if (e - b <= list_wave_most) continue;  // workgroup-uniform
        double v = 0.0;
        for (uint64_t j = b + threadIdx.x; j < e; j += kGroupAggThreads) v += group_f64_cell(col, rows[j]);
        v = wave_sum_f64(v);
        __syncthreads();  // the previous long list's s_wave has been read
        if (lane == 0) s_wave[wave] = v;
        __syncthreads();
        if (threadIdx.x == 0) out[g] = 0.0 + ((s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]));
    }
}

// 0, 1, ..., n - 1: the values the stable sort of the group ids carries along
static __global__ __launch_bounds__(kGroupAggThreads) void group_iota_rows(uint64_t n, uint32_t *rows) {
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kGroupAggThreads + threadIdx.x; j < n; j += static_cast<uint64_t>(gridDim.x) * kGroupAggThreads)
        rows[j] = static_cast<uint32_t>(j);
}

}  // namespace rvk
