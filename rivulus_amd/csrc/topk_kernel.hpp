// Top-k (topk.hip): the first k rows of the sort without sorting the column -- rv_top_k_indices, rv_top_k.  The semantics are those of
// include/rivulus_gpu.h (rv_top_k_indices) and DESIGN.md section 4 K11; the decisions are in topk_rule.hpp.
//
// An MSD radix SELECT over the 8-bit digits of the first key's working key (sort_kernel.hpp: the order key, complemented when descending):
//   topk_hist     one read of the key column: the digits of the non-null keys at all eight positions (LDS counters, the wave-uniform
//                 shortcut, one flush per workgroup) -- sort_map_hist without its two stores.
//   topk_plan     one workgroup.  After topk_hist: the non-null rows, the mask of positions at which two non-null keys differ, the digits
//                 every non-null key shares at the other positions, the values owed (topk_rule.hpp, null_class) and the bin rule
//                 (choose_bin) over the histogram of the highest differing position.  After a refine pass: the bin rule over its histogram.
//   topk_refine   one more read of the key column: the histogram of the digit at `pos` over the non-null rows whose key agrees with the
//                 chosen prefix above `pos`.
//   topk_collect  the candidates -- null rows when they are taken, non-null rows whose key from the last position up is <= the prefix's --
//                 as ascending row ids: topk_tile_count (per-tile counts), the exclusive scan of them (strings.hip), topk_collect (rank by
//                 ballot and mbcnt).  Two reads of the key column.
// No kernel here waits for another workgroup: every dependency between workgroups is a kernel boundary.
#pragma once

#include "sort_kernel.hpp"
#include "topk_rule.hpp"

namespace rvk {

constexpr int kTopKThreads = kSortThreads;
constexpr int kTopKWaves = kTopKThreads / kWave;
constexpr int kTopKRowsPerLane = static_cast<int>(rvt::kTopKCollectRowsPerLane);
constexpr int kTopKTileRows = kTopKThreads * kTopKRowsPerLane;  // a tile of the collect: one workgroup, wave w the w-th quarter of it
static_assert(rvtopk::kBins == kSortDigits && rvtopk::kPositions == kSortPositions, "the select's digits are the sort's");

struct TopKHistParams {
    DevCol key;
    uint64_t n;
    uint64_t flip;             // ~0: descending, 0: ascending
    unsigned long long *hist;  // [kSortPositions][kSortDigits], zeroed: digit counts of the non-null keys
};

__device__ __forceinline__ uint64_t topk_working_key(const DevCol &key, uint64_t row, bool is_float, uint64_t flip) {
    return rvorder::sort_key(static_cast<const uint64_t *>(key.values)[key.offset + row], is_float) ^ flip;
}

// Grid-strided, one row per lane and step.
static __global__ __launch_bounds__(kTopKThreads) void topk_hist(const TopKHistParams p) {
    __shared__ uint32_t s_hist[kSortPositions * kSortDigits];
    for (int k = threadIdx.x; k < kSortPositions * kSortDigits; k += kTopKThreads) s_hist[k] = 0;
    __syncthreads();
    const bool is_float = p.key.dtype == DT_FLOAT64;
    const int lane = lane_id();
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kTopKThreads; base < p.n; base += static_cast<uint64_t>(gridDim.x) * kTopKThreads) {
        const uint64_t i = base + threadIdx.x;
        const bool valid = i < p.n && !sort_cell_is_null(p.key, i);
        uint64_t k = 0;
        if (valid) k = topk_working_key(p.key, i, is_float, p.flip);
        const uint64_t vm = ballot64(valid);
        if (vm == 0) continue;
        const int first = __ffsll(static_cast<long long>(vm)) - 1;
        const uint64_t k0 = readlane64(k, first);
#pragma unroll
        for (int pos = 0; pos < kSortPositions; ++pos) {
            const uint32_t d = static_cast<uint32_t>(k >> (8 * pos)) & 0xFF, d0 = static_cast<uint32_t>(k0 >> (8 * pos)) & 0xFF;
            // the usual case at the high positions: every valid lane holds the same digit -- one add for the wave
            if (ballot64(valid && d == d0) == vm) {
                if (lane == first) atomicAdd(&s_hist[pos * kSortDigits + d0], static_cast<uint32_t>(__popcll(vm)));
            } else if (valid) atomicAdd(&s_hist[pos * kSortDigits + d], 1u);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kSortPositions * kSortDigits; k += kTopKThreads)
        if (s_hist[k]) atomicAdd(&p.hist[k], static_cast<unsigned long long>(s_hist[k]));
}

struct TopKRefineParams {
    DevCol key;
    uint64_t n;
    uint64_t flip;
    uint64_t prefix;           // the digits chosen (or shared by every key) at the positions above `pos`
    uint32_t pos;
    unsigned long long *hist;  // [kSortDigits], zeroed
};

static __global__ __launch_bounds__(kTopKThreads) void topk_refine(const TopKRefineParams p) {
    __shared__ uint32_t s_hist[kSortDigits];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const bool is_float = p.key.dtype == DT_FLOAT64;
    const uint64_t want = rvtopk::high_above(p.prefix, p.pos);
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kTopKThreads; base < p.n; base += static_cast<uint64_t>(gridDim.x) * kTopKThreads) {
        const uint64_t i = base + threadIdx.x;
        const bool valid = i < p.n && !sort_cell_is_null(p.key, i);
        uint64_t k = 0;
        if (valid) k = topk_working_key(p.key, i, is_float, p.flip);
        const bool match = valid && rvtopk::high_above(k, p.pos) == want;
        if (ballot64(match) == 0) continue;
        const uint32_t d = static_cast<uint32_t>(k >> (8 * p.pos)) & 0xFF;
        const uint64_t peers = sort_peers(d, match);
        if (match && mbcnt(peers) == 0) atomicAdd(&s_hist[d], static_cast<uint32_t>(__popcll(peers)));  // the first of its peers adds for all
    }
    __syncthreads();
    if (s_hist[threadIdx.x]) atomicAdd(&p.hist[threadIdx.x], static_cast<unsigned long long>(s_hist[threadIdx.x]));
}

// what topk_plan leaves in the control block, one 8-byte word each
enum : int { TOPK_OUT_VALID = 0, TOPK_OUT_MASK, TOPK_OUT_PREFIX, TOPK_OUT_BELOW, TOPK_OUT_IN_BIN, TOPK_OUT_POS, TOPK_OUT_WORDS };

struct TopKPlanParams {
    const unsigned long long *hist;  // FIRST: [kSortPositions][kSortDigits] of topk_hist; else [kSortDigits] of topk_refine
    uint64_t n, k;                   // FIRST: the rows and the rows asked for, 0 < k < n
    uint32_t nulls_last;             // FIRST
    uint64_t r;                      // a refine pass: values owed among the rows it counted
    uint64_t prefix;                 // a refine pass: its prefix
    uint32_t pos;                    // a refine pass: its position
    unsigned long long *out;         // [TOPK_OUT_WORDS]
};

template <bool FIRST>
static __global__ __launch_bounds__(kTopKThreads) void topk_plan(const TopKPlanParams p) {
    __shared__ unsigned long long s_hist[kSortDigits];
    __shared__ uint32_t s_used[kSortPositions], s_digit[kSortPositions];
    __shared__ unsigned long long s_rows;
    uint64_t valid_rows = 0, mask = 0, prefix = p.prefix, r = p.r;
    uint32_t pos = p.pos;
    bool choose = true;
    if constexpr (FIRST) {
        if (threadIdx.x < kSortPositions) s_used[threadIdx.x] = s_digit[threadIdx.x] = 0;
        if (threadIdx.x == 0) s_rows = 0;
        __syncthreads();
        for (int q = 0; q < kSortPositions; ++q) {
            const unsigned long long c = p.hist[q * kSortDigits + threadIdx.x];
            if (c) {
                atomicAdd(&s_used[q], 1u);
                atomicMax(&s_digit[q], static_cast<uint32_t>(threadIdx.x));  // read only where one digit is used
            }
            if (q == 0 && c) atomicAdd(&s_rows, c);
        }
        __syncthreads();
        valid_rows = s_rows;
        prefix = 0;
        for (int q = 0; q < kSortPositions; ++q) {
            if (s_used[q] > 1) mask |= 1ull << q;
            else prefix |= static_cast<uint64_t>(s_digit[q]) << (8 * q);
        }
        pos = rvtopk::highest_position(mask);  // no differing position: position 0, whose one used bin holds every value
        const rvtopk::NullClass nc = rvtopk::null_class(p.n, valid_rows, p.k, p.nulls_last != 0);
        choose = nc.kind == rvtopk::kValues;
        r = nc.r;
    }
    s_hist[threadIdx.x] = p.hist[(FIRST ? pos * kSortDigits : 0) + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        rvtopk::BinChoice b{0, 0, 0};
        if (choose) {
            b = rvtopk::choose_bin(s_hist, r);
            prefix = rvtopk::with_digit(prefix, pos, b.bin);
        }
        p.out[TOPK_OUT_VALID] = valid_rows;
        p.out[TOPK_OUT_MASK] = mask;
        p.out[TOPK_OUT_PREFIX] = prefix;
        p.out[TOPK_OUT_BELOW] = b.below;
        p.out[TOPK_OUT_IN_BIN] = b.in_bin;
        p.out[TOPK_OUT_POS] = pos;
    }
}

struct TopKCollectParams {
    DevCol key;
    uint64_t n;
    uint64_t flip;
    uint64_t limit;            // a non-null row is a candidate when its key from `pos` up is <= this
    uint32_t pos;
    uint32_t take_values;      // 0: no non-null row is a candidate
    uint32_t take_nulls;       // 1: every null row is a candidate
    uint32_t *tile_counts;     // [ntiles]: topk_tile_count writes
    const uint64_t *bases;     // the exclusive scan of tile_counts: topk_collect reads
    int64_t *out;              // [capacity]: the scan's total rows, which the host knows from the plan
    uint64_t capacity;
};

__device__ __forceinline__ bool topk_is_candidate(const TopKCollectParams &p, uint64_t row, bool is_float) {
    if (sort_cell_is_null(p.key, row)) return p.take_nulls != 0;
    return p.take_values && rvtopk::high_from(topk_working_key(p.key, row, is_float, p.flip), p.pos) <= p.limit;
}

// One workgroup per tile.  Wave w holds rows [w x 64 x R, (w + 1) x 64 x R) of the tile, 64 consecutive rows per step: lane order inside a
// step, step order inside a wave and wave order inside the tile are all row order.
static __global__ __launch_bounds__(kTopKThreads) void topk_tile_count(const TopKCollectParams p) {
    __shared__ uint32_t s_total;
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    const bool is_float = p.key.dtype == DT_FLOAT64;
    const int lane = lane_id(), wave = static_cast<int>(threadIdx.x) >> 6;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kTopKTileRows + static_cast<uint64_t>(wave) * kTopKRowsPerLane * kWave;
    uint32_t count = 0;
#pragma unroll
    for (int r = 0; r < kTopKRowsPerLane; ++r) {
        const uint64_t i = base + static_cast<uint64_t>(r) * kWave + lane;
        count += static_cast<uint32_t>(__popcll(ballot64(i < p.n && topk_is_candidate(p, i, is_float))));
    }
    if (lane == 0 && count) atomicAdd(&s_total, count);
    __syncthreads();
    if (threadIdx.x == 0) p.tile_counts[blockIdx.x] = s_total;
}

static __global__ __launch_bounds__(kTopKThreads) void topk_collect(const TopKCollectParams p) {
    __shared__ uint32_t s_wave_total[kTopKWaves];
    const bool is_float = p.key.dtype == DT_FLOAT64;
    const int lane = lane_id(), wave = static_cast<int>(threadIdx.x) >> 6;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kTopKTileRows + static_cast<uint64_t>(wave) * kTopKRowsPerLane * kWave;
    uint64_t ballots[kTopKRowsPerLane];
    uint32_t total = 0;
#pragma unroll
    for (int r = 0; r < kTopKRowsPerLane; ++r) {
        const uint64_t i = base + static_cast<uint64_t>(r) * kWave + lane;
        ballots[r] = ballot64(i < p.n && topk_is_candidate(p, i, is_float));
        total += static_cast<uint32_t>(__popcll(ballots[r]));
    }
    if (lane == 0) s_wave_total[wave] = total;
    __syncthreads();
    uint64_t at = p.bases[blockIdx.x];
    for (int w = 0; w < wave; ++w) at += s_wave_total[w];
#pragma unroll
    for (int r = 0; r < kTopKRowsPerLane; ++r) {
        const uint64_t q = at + mbcnt(ballots[r]);
        if (((ballots[r] >> lane) & 1) && q < p.capacity) p.out[q] = static_cast<int64_t>(base + static_cast<uint64_t>(r) * kWave + lane);
        at += static_cast<uint32_t>(__popcll(ballots[r]));
    }
}

}  // namespace rvk
