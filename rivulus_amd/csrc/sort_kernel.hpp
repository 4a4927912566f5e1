// Sort (sort.hip): the stable permutation of a key column -- rv_sort_indices, and rv_sort on top of it and the gather.  The reference has
// no sort; the semantics are those of include/rivulus_gpu.h (rv_sort_indices) and DESIGN.md section 4 K10.
//
// An LSD radix sort over the 8-bit digits of a 64-bit WORKING KEY, with the row as a 4-byte payload:
//   sort_map_hist   one pass over the key column (read through `prior` when there is one, whose indices it also checks): the working key
//                   of a non-null cell is its order key (order_key.hpp, sort_key), complemented for a descending sort; a null cell's is 0
//                   and whatever lies under it is not loaded.  The same pass counts the digits of the non-null keys at all eight positions
//                   (LDS counters, one flush per workgroup); sort_plan turns the counts into the positions that need a pass -- those at
//                   which two non-null keys differ -- and the number of non-null rows.
//   per pass        sort_tile_hist (per-tile digit counts, digit-major), the exclusive scan of them (strings.hip), sort_scatter.
//   nulls           one more pass of the same kernels over the "digit" null / not null, read from the key's validity at the payload's
//                   row, as the LAST (most significant) pass -- run only when some but not all rows are null.  The null rows ride through
//                   the value passes with the key 0: equal among themselves, so they stay in row order, and where they end up relative to
//                   the non-null rows does not matter before the last pass.  (That is also why a position at which only the nulls' 0
//                   differs from the one digit of all non-null keys can be skipped.)
//   the last pass   writes the rows as Int64 and no keys.  No pass at all (an all-equal key): sort_widen.
// No kernel here waits for another workgroup: every dependency between workgroups is a kernel boundary.
#pragma once

#include "device_common.hpp"
#include "order_key.hpp"
#include "thresholds.hpp"

namespace rvk {

constexpr int kSortThreads = 256;  // == the digits of a pass: thread d owns digit d in the tile scan
constexpr int kSortWaves = kSortThreads / kWave;
constexpr int kSortRowsPerLane = static_cast<int>(rvt::kSortRowsPerLane);
constexpr int kSortTileRows = kSortThreads * kSortRowsPerLane;
constexpr int kSortDigits = 256;
constexpr int kSortPositions = 8;  // digit positions of a 64-bit key
static_assert(kSortThreads == kSortDigits, "one thread per digit in the tile scan");

__device__ __forceinline__ bool sort_cell_is_null(const DevCol &c, uint64_t row) {
    if (c.dtype == DT_NULL) return true;
    const uint64_t at = c.offset + row;
    return c.validity && !((c.validity[at >> 3] >> (at & 7)) & 1);
}

// the lanes of the wave that are `in` and hold the same 8-bit digit as this one (itself included): eight ballots
__device__ __forceinline__ uint64_t sort_peers(uint32_t digit, bool in) {
    uint64_t peers = ballot64(in);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1;
        const uint64_t m = ballot64(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

struct SortMapParams {
    DevCol key;
    const uint64_t *prior;             // nullptr: the identity
    uint64_t n;
    uint64_t flip;                     // ~0: descending (the working key of a non-null cell is complemented), 0: ascending
    uint64_t *keys;                    // [n] out
    uint32_t *rows;                    // [n] out
    unsigned long long *hist;          // [kSortPositions][kSortDigits], zeroed: digit counts of the non-null keys
    unsigned long long *first_bad;     // ~0: the smallest position of `prior` whose index is >= n
};

// Grid-strided, one row per lane and step.
static __global__ __launch_bounds__(kSortThreads) void sort_map_hist(const SortMapParams p) {
    __shared__ uint32_t s_hist[kSortPositions * kSortDigits];
    for (int k = threadIdx.x; k < kSortPositions * kSortDigits; k += kSortThreads) s_hist[k] = 0;
    __syncthreads();
    const bool is_float = p.key.dtype == DT_FLOAT64;
    const int lane = lane_id();
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kSortThreads; base < p.n; base += static_cast<uint64_t>(gridDim.x) * kSortThreads) {
        const uint64_t i = base + threadIdx.x;
        const bool in = i < p.n;
        uint64_t row = i;
        bool readable = in;
        if (in && p.prior) {
            row = p.prior[i];
            if (row >= p.n) {  // nothing is read through it; the call fails
                readable = false;
                row = 0;
                atomicMin(p.first_bad, static_cast<unsigned long long>(i));
            }
        }
        const bool valid = readable && !sort_cell_is_null(p.key, row);
        uint64_t k = 0;
        if (valid) k = rvorder::sort_key(static_cast<const uint64_t *>(p.key.values)[p.key.offset + row], is_float) ^ p.flip;
        if (in) {
            p.keys[i] = k;
            p.rows[i] = static_cast<uint32_t>(row);
        }
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
    for (int k = threadIdx.x; k < kSortPositions * kSortDigits; k += kSortThreads)
        if (s_hist[k]) atomicAdd(&p.hist[k], static_cast<unsigned long long>(s_hist[k]));
}

// One workgroup: *passes = bit `pos` for every digit position at which the non-null keys hold more than one digit; *valid_rows = the
// non-null rows.
static __global__ __launch_bounds__(kSortThreads) void sort_plan(const unsigned long long *hist, unsigned long long *passes, unsigned long long *valid_rows) {
    __shared__ uint32_t s_used[kSortPositions];
    __shared__ unsigned long long s_rows;
    if (threadIdx.x < kSortPositions) s_used[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_rows = 0;
    __syncthreads();
    for (int pos = 0; pos < kSortPositions; ++pos) {
        const unsigned long long c = hist[pos * kSortDigits + threadIdx.x];
        if (c) atomicAdd(&s_used[pos], 1u);
        if (pos == 0 && c) atomicAdd(&s_rows, c);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = 0;
        for (int pos = 0; pos < kSortPositions; ++pos)
            if (s_used[pos] > 1) m |= 1ull << pos;
        *passes = m;
        *valid_rows = s_rows;
    }
}

struct SortPassParams {
    const uint64_t *keys_in;   // value passes
    const uint32_t *rows_in;
    uint64_t *keys_out;        // every pass but the last
    uint32_t *rows_out;
    int64_t *index_out;        // the last pass
    uint32_t *tile_counts;     // [nbins x ntiles] digit-major: sort_tile_hist writes
    const uint64_t *bases;     // the exclusive scan of tile_counts: sort_scatter reads
    DevCol key;                // the null pass reads the validity at the payload's row
    uint64_t n;
    uint32_t ntiles;
    uint32_t shift;            // value passes: the digit is bits [shift, shift + 8) of the working key
    uint32_t nbins;            // 256, or 2 in the null pass
    uint32_t null_digit;       // null pass: the digit of a null row (0: nulls first, 1: nulls last); a non-null row has the other one
};

template <bool NULLS>
__device__ __forceinline__ uint32_t sort_digit(const SortPassParams &p, uint64_t key, uint32_t row) {
    if constexpr (NULLS) return sort_cell_is_null(p.key, row) ? p.null_digit : 1u - p.null_digit;
    else return static_cast<uint32_t>(key >> p.shift) & 0xFF;
}

// One workgroup per tile: tile_counts[digit x ntiles + tile] = the tile's rows with that digit.
template <bool NULLS>
static __global__ __launch_bounds__(kSortThreads) void sort_tile_hist(const SortPassParams p) {
    __shared__ uint32_t s_count[kSortDigits];
    s_count[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kSortTileRows;
#pragma unroll
    for (int r = 0; r < kSortRowsPerLane; ++r) {
        const uint64_t i = base + static_cast<uint64_t>(r) * kSortThreads + threadIdx.x;
        const bool in = i < p.n;
        uint32_t d = 0;
        if (in) d = NULLS ? sort_digit<true>(p, 0, p.rows_in[i]) : sort_digit<false>(p, p.keys_in[i], 0);
        const uint64_t peers = sort_peers(d, in);
        if (in && mbcnt(peers) == 0) atomicAdd(&s_count[d], static_cast<uint32_t>(__popcll(peers)));  // the first of its peers adds for all
    }
    __syncthreads();
    if (threadIdx.x < p.nbins) p.tile_counts[static_cast<uint64_t>(threadIdx.x) * p.ntiles + blockIdx.x] = s_count[threadIdx.x];
}

// One workgroup per tile.  Wave w holds rows [w x 64 x R, (w + 1) x 64 x R) of the tile, 64 consecutive rows per step, so that lane
// order inside a step, step order inside a wave and wave order inside the tile are all row order: a row's rank among the tile's rows of
// its digit is (rows of the digit in earlier waves) + (in earlier steps of its wave) + (in lower lanes of its step).
//   1. per step: the peers of the lane's digit (sort_peers); rank = the wave's counter of the digit + the peers below the lane; the LAST
//      peer stores the counter back, advanced by the peers -- a plain LDS store: the counters are the wave's own and a wave's LDS
//      accesses are served in program order (volatile keeps the compiler from moving them);
//   2. thread d: the waves' counters of digit d -> exclusive over the waves, the total -> exclusive over the digits (where the digit's
//      run starts in the tile), and the run's place in the output from the scanned tile counts;
//   3. keys, rows and digits staged in LDS at start + wave offset + rank: the tile sorted by the digit, stably;
//   4. LDS position q goes to base[digit] + (q - start[digit]): every digit's run leaves as consecutive stores.
template <bool NULLS, bool LAST>
static __global__ __launch_bounds__(kSortThreads) void sort_scatter(const SortPassParams p) {
    __shared__ uint32_t s_count[kSortWaves * kSortDigits];
    __shared__ uint32_t s_start[kSortDigits], s_delta[kSortDigits], s_wave_total[kSortWaves];
    __shared__ uint64_t s_keys[LAST ? 1 : kSortTileRows];
    __shared__ uint32_t s_rows[kSortTileRows];
    __shared__ uint8_t s_digit[kSortTileRows];
    const int lane = lane_id(), wave = static_cast<int>(threadIdx.x) >> 6;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kSortTileRows;
    const uint32_t tile_rows = static_cast<uint32_t>(p.n - base < static_cast<uint64_t>(kSortTileRows) ? p.n - base : kSortTileRows);
    for (int k = threadIdx.x; k < kSortWaves * kSortDigits; k += kSortThreads) s_count[k] = 0;
    __syncthreads();

    volatile uint32_t *mine = s_count + wave * kSortDigits;
    uint64_t key[kSortRowsPerLane];
    uint32_t row[kSortRowsPerLane], ranked[kSortRowsPerLane];  // digit | rank in the wave << 8
#pragma unroll
    for (int r = 0; r < kSortRowsPerLane; ++r) {
        const uint32_t local = static_cast<uint32_t>(wave * kSortRowsPerLane + r) * kWave + lane;
        const bool in = local < tile_rows;
        key[r] = 0;
        row[r] = 0;
        if (in) {
            row[r] = p.rows_in[base + local];
            if constexpr (!NULLS) key[r] = p.keys_in[base + local];
        }
        const uint32_t d = in ? sort_digit<NULLS>(p, key[r], row[r]) : 0;
        const uint64_t peers = sort_peers(d, in);
        const uint32_t below = mbcnt(peers);
        uint32_t before = 0;
        if (in) before = mine[d];
        if (in && (peers >> lane) == 1) mine[d] = before + below + 1;  // the last of its peers
        ranked[r] = d | (before + below) << 8;
    }
    __syncthreads();

    {
        const uint32_t d = threadIdx.x;
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < kSortWaves; ++w) {
            const uint32_t c = s_count[w * kSortDigits + d];
            s_count[w * kSortDigits + d] = total;
            total += c;
        }
        const uint32_t incl = wave_scan_u32(total);
        if (lane == kWave - 1) s_wave_total[wave] = incl;
        __syncthreads();
        uint32_t start = incl - total;
        for (int w = 0; w < wave; ++w) start += s_wave_total[w];
        s_start[d] = start;
        // 32-bit arithmetic that may wrap: base - start + q is below n < 2^32 for every q of the run
        s_delta[d] = (d < p.nbins ? static_cast<uint32_t>(p.bases[static_cast<uint64_t>(d) * p.ntiles + blockIdx.x]) : 0u) - start;
    }
    __syncthreads();

#pragma unroll
    for (int r = 0; r < kSortRowsPerLane; ++r) {
        const uint32_t local = static_cast<uint32_t>(wave * kSortRowsPerLane + r) * kWave + lane;
        if (local < tile_rows) {
            const uint32_t d = ranked[r] & 0xFF;
            const uint32_t q = s_start[d] + s_count[wave * kSortDigits + d] + (ranked[r] >> 8);
            if constexpr (!LAST) s_keys[q] = key[r];
            s_rows[q] = row[r];
            s_digit[q] = static_cast<uint8_t>(d);
        }
    }
    __syncthreads();

    for (uint32_t q = threadIdx.x; q < tile_rows; q += kSortThreads) {
        const uint32_t at = s_delta[s_digit[q]] + q;
        if constexpr (LAST) p.index_out[at] = static_cast<int64_t>(s_rows[q]);
        else {
            p.keys_out[at] = s_keys[q];
            p.rows_out[at] = s_rows[q];
        }
    }
}

// no pass ran (every non-null key equal, and no or only nulls): the rows as they are, as Int64
static __global__ __launch_bounds__(kSortThreads) void sort_widen(const uint32_t *rows, uint64_t n, int64_t *out) {
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSortThreads + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * kSortThreads)
        out[i] = static_cast<int64_t>(rows[i]);
}

}  // namespace rvk
