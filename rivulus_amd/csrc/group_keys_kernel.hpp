// Grouping by several key columns (group_agg.hip): the insert / first-row / id passes of group_agg_kernel.hpp over TUPLES of cells --
// rv_group_ids_keys and rv_hash_aggregate_keys.  The semantics are those of include/rivulus_gpu.h (K9a) and DESIGN.md section 4 K9a.
//
// The group table is K9's: one 64-bit word per distinct tuple, hash_high32 << 32 | (first row + 1), claimed by one compare-and-swap,
// its row only ever falling by atomicMin under an equal tag and an equal tuple.  The key is read THROUGH THE ROW, so a slot's key is
// the tuple of cells at the slot's row, one cell per key column; everything behind the ids (group_mark_first, the selection scan, the
// accumulate stage) never looks at a key and runs as it is.
//
// A cell is (is_null, word):
//   Int64    the bits.
//   Float64  the bits, every NaN replaced by ONE pattern (kKeysNan): the equality the sort's order induces -- all NaNs are one key,
//            -0.0 and +0.0 are two.
//   Boolean  bit `offset + i` of the LSB-first buffer, 0 or 1.
//   Null     no word: every cell is null.
// What lies under a null cell is never read as a value; its word is 0 and its flag tells it from a valid 0.  A null cell equals a
// null cell of the same column and no value, so (null, 0), (0, null), (0, 0) and (null, null) are four ordinary tuples in the table:
// there is no null group beside it.
//
// Hash: h = kKeysSeed; h = join_hash(h ^ word_k) for k = 0 .. nkeys - 1, in key order; h = join_hash(h ^ null flags), bit k = cell k
// is null.  join_hash is a bijection, so the fold depends on the ORDER of the words -- (1, 2) and (2, 1) meet only by accident -- and
// the flags are a word of their own: two tuples that differ only in which cells are null differ in the last word folded.
//
// The kernels are templates on the number of key columns: the loops over the columns unroll, a lane's cells live in registers and the
// column views are read from the kernel arguments at constant offsets (no scratch, no LDS).
#pragma once

#include "group_agg_kernel.hpp"

namespace rvk {

constexpr int kGroupKeysMost = 8;
constexpr uint64_t kKeysNan = 0x7FF8000000000000ull;   // the one NaN of a Float64 key
constexpr uint64_t kKeysSeed = 0x9E3779B97F4A7C15ull;  // join_hash(0) == 0: an all-zero tuple must not start every fold at 0

struct GroupKeysView {
    unsigned long long *slots;
    uint64_t slot_mask;  // slots - 1
    uint64_t hash_mask;  // ~0, or the low bits option "agg_hash_bits" leaves (collision tests)
    uint64_t n;
    uint32_t nkeys;
    uint32_t pad;
    DevCol key[kGroupKeysMost];
};

// cell i of one key column: false for a null (word 0)
__device__ __forceinline__ bool keys_cell(const DevCol &c, uint64_t i, uint64_t &word) {
    word = 0;
    if (c.dtype == DT_NULL) return false;
    const uint64_t at = c.offset + i;
    if (c.validity && !((c.validity[at >> 3] >> (at & 7)) & 1)) return false;
    if (c.dtype == DT_BOOLEAN) {
        word = (static_cast<const uint8_t *>(c.values)[at >> 3] >> (at & 7)) & 1;
        return true;
    }
    word = static_cast<const uint64_t *>(c.values)[at];
    if (c.dtype == DT_FLOAT64 && rvorder::order_key_is_nan(word)) word = kKeysNan;
    return true;
}

// a lane's tuple: the words and the null flags (bit k: cell k is null)
template <int NK>
struct KeysTuple {
    uint64_t word[NK];
    uint32_t nulls;
};

template <int NK>
__device__ __forceinline__ KeysTuple<NK> keys_tuple(const GroupKeysView &t, uint64_t i) {
    KeysTuple<NK> r;
    r.nulls = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k)
        if (!keys_cell(t.key[k], i, r.word[k])) r.nulls |= 1u << k;
    return r;
}

template <int NK>
__device__ __forceinline__ uint64_t keys_hash(const KeysTuple<NK> &a) {
    uint64_t h = kKeysSeed;
#pragma unroll
    for (int k = 0; k < NK; ++k) h = join_hash(h ^ a.word[k]);
    return join_hash(h ^ a.nulls);
}

// the tuple at `row` against a lane's own, column by column; stops at the first cell that differs
template <int NK>
__device__ __forceinline__ bool keys_equal_at(const GroupKeysView &t, uint64_t row, const KeysTuple<NK> &a) {
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        uint64_t w;
        const bool valid = keys_cell(t.key[k], row, w);
        if (valid == static_cast<bool>((a.nulls >> k) & 1) || w != a.word[k]) return false;
    }
    return true;
}

struct GroupKeysInsertParams {
    GroupKeysView t;
    unsigned long long *distinct;  // striped counter of the slots claimed
    unsigned long long *claimed;   // one word, or nullptr: rows <= agg_max_groups, the table cannot fill
    uint64_t max_groups;
    uint32_t *error;               // bit 0: a chain walk exhausted the table; bit 1: more tuples than max_groups, claiming has stopped
};

// group_insert over tuples.  One lane per row; a lane whose tuple equals the previous lane's -- every word and the null flags -- leaves
// the insert to the head of its run.  A lane outside n is never a head and never equal to one inside: the comparison asks for the
// previous lane to be a row.
template <int NK>
static __global__ __launch_bounds__(kGroupAggThreads) void group_insert_keys(const GroupKeysInsertParams q) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kGroupAggThreads + threadIdx.x;
    const int lane = lane_id();
    const bool in = i < q.t.n;
    KeysTuple<NK> a;
    if (in) a = keys_tuple<NK>(q.t, i);
    else {
        a.nulls = 0;
#pragma unroll
        for (int k = 0; k < NK; ++k) a.word[k] = 0;
    }
    const int prev = lane > 0 ? lane - 1 : 0;
    // every lane takes part in every shuffle (a lane that is switched off hands its neighbour 0): no `&&` that would skip one
    uint64_t differ = static_cast<uint32_t>(__shfl(static_cast<int>(a.nulls), prev, 64)) ^ a.nulls;
#pragma unroll
    for (int k = 0; k < NK; ++k) differ |= shfl64(a.word[k], prev) ^ a.word[k];
    const bool same = differ == 0;
    const uint64_t rows = ballot64(in);
    const bool head = in && !(lane > 0 && ((rows >> (lane - 1)) & 1) && same);
    bool claimed = false;
    const bool stopped = q.claimed && (__hip_atomic_load(q.error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2u);
    if (head && !stopped) {
        const uint64_t h = keys_hash<NK>(a) & q.t.hash_mask;
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
                // lost the slot: another row of the SAME tuple may have taken it -- look at what it holds now
            }
            if ((e >> 32) == (mine >> 32) && keys_equal_at<NK>(q.t, static_cast<uint32_t>(e) - 1, a)) {
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

// the first row of the group of row i (every tuple is in the table: the insert ran over the same columns)
template <int NK>
__device__ __forceinline__ uint64_t group_first_row_keys(const GroupKeysView &t, uint64_t i, uint32_t *error) {
    const KeysTuple<NK> a = keys_tuple<NK>(t, i);
    const uint64_t h = keys_hash<NK>(a) & t.hash_mask;
    const uint32_t tag = static_cast<uint32_t>(h >> 32);
    uint64_t s = h & t.slot_mask;
    for (uint64_t step = 0; step <= t.slot_mask; ++step, s = (s + 1) & t.slot_mask) {
        const unsigned long long e = t.slots[s];
        if (e == 0) break;
        const uint64_t row = static_cast<uint32_t>(e) - 1;
        if (static_cast<uint32_t>(e >> 32) == tag && (row == i || keys_equal_at<NK>(t, row, a))) return row;
    }
    atomicOr(error, 1u);
    return 0;
}

// One lane per row: the position of the row's group = first rows below the group's own (group_ids of group_agg_kernel.hpp).
template <int NK, typename ID>
static __global__ __launch_bounds__(kGroupAggThreads) void group_ids_keys(const GroupKeysView t, const uint64_t *marks, const uint64_t *excl, ID *gids, uint32_t *error) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kGroupAggThreads + threadIdx.x;
    if (i >= t.n) return;
    const uint64_t fr = group_first_row_keys<NK>(t, i, error);
    gids[i] = static_cast<ID>(excl[fr >> 6] + __popcll(marks[fr >> 6] & low_mask(fr & 63)));
}

}  // namespace rvk
