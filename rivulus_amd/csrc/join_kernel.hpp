// Hash join (reference PhysicalPlan::HashJoin, plan.rs:174-284): the build-side table and the probe kernels, for the inner join and
// the outer, semi and anti joins.
//
// Layout of a build table (join.hip, build_table):
//   rows   uint32 build row ids: the non-null, non-NaN rows grouped by key, each group ascending (a stable radix sort of
//          (key bits, row)), followed by the null rows, ascending -- the Vec push order of the reference's
//          HashMap<AnyValue, Vec<usize>>;
//   slots  open addressing, a power of two >= 2 x the non-null rows, linear probing; one 16-byte slot per distinct key:
//          x = the key's 64 bits (Int64 value, Float64 to_bits, Boolean 0 / 1), y = start into `rows` | count << 32;
//          y == 0: empty.
// A probe row's matches are rows[start, start + count): the key's group, the null group for a null probe key, nothing for a
// miss or a NaN.  Output positions come from scans of match counts (no atomics): the pairs are in probe-row order and, within
// a probe row, in ascending build-row order, identically on every run.
#pragma once

#include "device_common.hpp"

namespace rvk {

constexpr int kJoinThreads = 256;                             // one workgroup of the probe kernels
constexpr int kJoinRowsPerThread = 16;                        // rows per lane of a probe tile, kJoinThreads apart
constexpr int kJoinTileRows = kJoinThreads * kJoinRowsPerThread;  // 4096 probe rows per workgroup
constexpr int kJoinClassWords = 16;                           // 64-row words per wave of join_classify
constexpr uint64_t kJoinClaimed = 0xFFFFFFFF00000000ull;      // y of a slot whose head has claimed it and whose count is not set yet

// key classes of a cell
enum : uint32_t { JK_VALUE = 0, JK_NULL = 1, JK_NEVER = 2 };

// class and 64 key bits of row i of a key column (AnyValue's Hash / PartialEq, series.rs:72-98): a null cell is JK_NULL (Null ==
// Null), a NaN JK_NEVER (PartialEq fails even for the same bits); every other cell is its bits.  +0.0 and -0.0 differ in their
// bits and so never match: the reference hashes them apart (to_bits) and could pair them only on a SipHash bucket-and-tag collision.
__device__ __forceinline__ uint32_t join_key(const DevCol &c, uint64_t i, uint64_t &bits) {
    bits = 0;
    if (c.dtype == DT_NULL) return JK_NULL;
    const uint64_t at = c.offset + i;
    if (c.validity && !((c.validity[at >> 3] >> (at & 7)) & 1)) return JK_NULL;
    if (c.dtype == DT_BOOLEAN) {
        bits = (static_cast<const uint8_t *>(c.values)[at >> 3] >> (at & 7)) & 1;
        return JK_VALUE;
    }
    bits = static_cast<const uint64_t *>(c.values)[at];
    if (c.dtype == DT_FLOAT64 && (bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return JK_NEVER;
    return JK_VALUE;
}

__device__ __forceinline__ uint64_t join_wave_max64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t y = (static_cast<uint64_t>(__shfl_xor(static_cast<uint32_t>(v >> 32), d, 64)) << 32) | __shfl_xor(static_cast<uint32_t>(v), d, 64);
        v = y > v ? y : v;
    }
    return v;
}

// murmur3's 64-bit finaliser: every key bit reaches the low bits the slot index is taken from
__device__ __forceinline__ uint64_t join_hash(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

struct JoinTableView {
    unsigned long long *slots;  // 2 words per slot (x, y)
    const uint32_t *rows;
    uint64_t slot_mask;   // slots - 1
    uint64_t hash_mask;   // ~0, or the low bits option "join_hash_bits" leaves (collision tests)
    uint32_t null_start, null_count;
    int32_t match_values;  // 0: the key dtypes differ (or one is Null): only null meets null
    int32_t pad;
};

// (start, count) of the matches of one probe cell.  `group` (the full outer join's count pass; nullptr everywhere else, and nothing of it
// is left in those inlined copies): the group met, for the marks -- the slot of a key group, the table's slot count for the null group
// (bit `slots` of the marks).  Meaningful only where the returned count is not 0.
__device__ __forceinline__ uint32_t join_lookup(const JoinTableView &t, uint32_t cls, uint64_t bits, uint32_t &start, uint64_t *group = nullptr) {
    start = 0;
    if (group) *group = t.slot_mask + 1;
    if (cls == JK_NULL) {
        start = t.null_start;
        return t.null_count;
    }
    if (cls != JK_VALUE || !t.match_values) return 0;
    uint64_t s = join_hash(bits) & t.hash_mask & t.slot_mask;
    for (;;) {
        const ulonglong2 e = *reinterpret_cast<const ulonglong2 *>(&t.slots[2 * s]);
        if (e.y == 0) return 0;
        if (e.x == bits) {
            start = static_cast<uint32_t>(e.y);
            if (group) *group = s;
            return static_cast<uint32_t>(e.y >> 32);
        }
        s = (s + 1) & t.slot_mask;
    }
}

// ---- join kinds -----------------------------------------------------------------------------------------------------------------
// rv_join_kind as a compile-time constant of the probe kernels: one body and one __global__ wrapper per pass, the inner join one of the
// kinds -- the row rule below is all that tells them apart.
enum : int { JOIN_INNER = 0, JOIN_OUTER = 1, JOIN_FULL = 2, JOIN_SEMI = 3, JOIN_ANTI = 4 };
constexpr uint64_t kJoinNone = ~0ull;  // "no partner" inside the index buffers; the public columns get a null cell for it

// Output rows of a probe row with c matches: the one rule the count passes and the emit pass share.
template <int KIND>
__device__ __forceinline__ uint32_t join_rows(uint32_t c) {
    if (KIND == JOIN_OUTER || KIND == JOIN_FULL) return c ? c : 1u;
    if (KIND == JOIN_SEMI) return c != 0;
    if (KIND == JOIN_ANTI) return c == 0;
    return c;
}

// One bit per group a probe row met (JOIN_FULL's count pass): a plain load first, the atomic only while the bit is clear, so a hot
// key costs one atomic and not one per probe row.  A stale load only repeats an idempotent OR.
__device__ __forceinline__ void join_mark(uint32_t *marks, uint64_t group) {
    const uint32_t bit = 1u << (group & 31);
    if (!(marks[group >> 5] & bit)) atomicOr(&marks[group >> 5], bit);
}

// ---- build ----------------------------------------------------------------------------------------------------------------------
// Bitmaps (offset 0) of the rows whose key goes into the table (`keep`: valid, not NaN) and of the null rows; their popcounts
// are added to counts[0] / counts[1] once per wave.
static __global__ __launch_bounds__(256) void join_classify(DevCol key, uint64_t n, uint64_t *keep, uint64_t *nulls, unsigned long long *counts) {
    const int lane = lane_id();
    const uint64_t wave = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwords = (n + 63) / 64;
    unsigned long long nk = 0, nn = 0;
    for (int w = 0; w < kJoinClassWords; ++w) {
        const uint64_t word = wave * kJoinClassWords + w;
        if (word >= nwords) break;  // wave-uniform
        const uint64_t i = word * 64 + lane;
        uint64_t bits;
        const uint32_t cls = i < n ? join_key(key, i, bits) : JK_NEVER;
        const uint64_t k = ballot64(cls == JK_VALUE), z = ballot64(cls == JK_NULL);
        if (lane == 0) {
            keep[word] = k;
            nulls[word] = z;
        }
        nk += __popcll(k);
        nn += __popcll(z);
    }
    if (lane == 0 && (nk | nn)) {
        atomicAdd(&counts[0], nk);
        atomicAdd(&counts[1], nn);
    }
}

// (key bits, row) of the kept rows, in row order: the input of the stable sort
static __global__ __launch_bounds__(256) void join_gather_keys(DevCol key, const uint64_t *idx, uint64_t n, uint64_t *keys, uint32_t *rows) {
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < n; j += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t r = idx[j];
        uint64_t bits;
        (void)join_key(key, r, bits);
        keys[j] = bits;
        rows[j] = static_cast<uint32_t>(r);
    }
}

// the null rows (ascending) behind the key groups
static __global__ __launch_bounds__(256) void join_null_rows(const uint64_t *idx, uint64_t n, uint32_t *rows) {
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < n; j += static_cast<uint64_t>(gridDim.x) * blockDim.x)
        rows[j] = static_cast<uint32_t>(idx[j]);
}

// The first row of every group of equal keys claims a free slot.  Each distinct key has exactly one head, so a head never meets
// its own key on the way: it takes the first empty slot.
static __global__ __launch_bounds__(256) void join_insert_heads(JoinTableView t, const uint64_t *keys, uint64_t n) {
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < n; j += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t k = keys[j];
        if (j > 0 && keys[j - 1] == k) continue;
        uint64_t s = join_hash(k) & t.hash_mask & t.slot_mask;
        while (atomicCAS(&t.slots[2 * s + 1], 0ull, kJoinClaimed | j) != 0ull) s = (s + 1) & t.slot_mask;
        t.slots[2 * s] = k;
    }
}

// The last row of every group finds its key's slot (every head has been inserted: a launch earlier on the stream) and sets the
// count; the largest count goes to *max_count.
static __global__ __launch_bounds__(256) void join_insert_tails(JoinTableView t, const uint64_t *keys, uint64_t n, unsigned long long *max_count) {
    unsigned long long most = 0;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < n; j += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t k = keys[j];
        if (j + 1 < n && keys[j + 1] == k) continue;
        uint64_t s = join_hash(k) & t.hash_mask & t.slot_mask;
        while (t.slots[2 * s] != k || t.slots[2 * s + 1] == 0) s = (s + 1) & t.slot_mask;
        const uint64_t start = t.slots[2 * s + 1] & 0xFFFFFFFFull;
        const uint64_t count = j + 1 - start;
        t.slots[2 * s + 1] = start | (count << 32);
        most = count > most ? count : most;
    }
    most = join_wave_max64(most);
    if (lane_id() == 0 && most) atomicMax(max_count, most);
}

// ---- probe ----------------------------------------------------------------------------------------------------------------------
struct JoinProbeParams {
    JoinTableView table;
    DevCol key;
    uint64_t n;
    uint64_t *tile_counts;  // count pass: matches per tile; emit pass: their exclusive prefixes
    int64_t *out_probe, *out_build;
    uint32_t lane_most;     // emit, mode 2: lists longer than this are written by the whole workgroup
};

// Pass 1: output rows per tile of kJoinTileRows probe rows (64-bit: one row can match every build row).  JOIN_FULL also marks
// the groups it meets.
template <int KIND>
__device__ __forceinline__ void join_count_body(const JoinProbeParams p, uint32_t *marks) {
    __shared__ uint64_t s_wave[kJoinThreads / 64];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kJoinTileRows + threadIdx.x;
    uint64_t mine = 0;
#pragma unroll
    for (int k = 0; k < kJoinRowsPerThread; ++k) {
        const uint64_t i = base + static_cast<uint64_t>(k) * kJoinThreads;
        if (i < p.n) {
            uint64_t bits;
            const uint32_t cls = join_key(p.key, i, bits);
            uint32_t start;
            if (KIND == JOIN_FULL) {
                uint64_t group;
                const uint32_t c = join_lookup(p.table, cls, bits, start, &group);
                if (c) join_mark(marks, group);
                mine += join_rows<KIND>(c);
            } else {
                mine += join_rows<KIND>(join_lookup(p.table, cls, bits, start));
            }
        }
    }
    mine = wave_sum64(mine);
    if (lane_id() == 0) s_wave[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < kJoinThreads / 64; ++w) t += s_wave[w];
        p.tile_counts[blockIdx.x] = t;
    }
}
template <int KIND>
static __global__ __launch_bounds__(kJoinThreads) void join_probe_count(JoinProbeParams p, uint32_t *marks) { join_count_body<KIND>(p, marks); }

// Pass 1 of a probe cut into batches of chunk_rows rows (rv_hash_join_chunked): the tile counts of join_probe_count and, in the
// same pass, the pairs of every batch -- batch b is probe rows [b * chunk_rows, min((b + 1) * chunk_rows, n)).
//   FAST (chunk_rows == rvt::kJoinFastBatchRows == kJoinTileRows / 4): a tile holds exactly four batches, and batch q of the tile is
//        rows k = 4q .. 4q + 3 of every lane (256 apart).  Four per-lane partial sums, four block reductions, four plain stores.
//   general: at every step k a wave holds 64 consecutive rows; a wave scan of their counts gives the sum of each batch's run, which
//        the run's last lane adds to the batch's LDS counter (the tile's first kJoinTileBatchSlots batches) or straight to
//        batch_counts.  One thread per LDS counter then stores it (a batch inside the tile) or adds it (a batch that spans tiles).
//        batch_counts is zeroed by the caller.
// Integer sums: the counts are the same on every run, whatever order the atomics land in.
constexpr int kJoinTileBatchSlots = 256;
struct JoinBatchParams {
    uint64_t chunk_rows;
    uint64_t nbatches;
    unsigned long long *batch_counts;  // [nbatches]
};

template <bool FAST, int KIND>
__device__ __forceinline__ void join_count_batched_body(const JoinProbeParams p, const JoinBatchParams b) {
    __shared__ uint64_t s_wave[4][kJoinThreads / 64];
    __shared__ unsigned long long s_batch[FAST ? 1 : kJoinTileBatchSlots];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kJoinTileRows;
    if (FAST) {
        uint64_t part[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < kJoinRowsPerThread; ++k) {
            const uint64_t i = tile0 + threadIdx.x + static_cast<uint64_t>(k) * kJoinThreads;
            if (i < p.n) {
                uint64_t bits;
                const uint32_t cls = join_key(p.key, i, bits);
                uint32_t start;
                part[k >> 2] += join_rows<KIND>(join_lookup(p.table, cls, bits, start));
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint64_t v = wave_sum64(part[q]);
            if (lane == 0) s_wave[q][wave] = v;
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            const int q = threadIdx.x;
            uint64_t t = 0;
#pragma unroll
            for (int w = 0; w < kJoinThreads / 64; ++w) t += s_wave[q][w];
            const uint64_t bi = static_cast<uint64_t>(blockIdx.x) * 4 + q;
            if (bi < b.nbatches) b.batch_counts[bi] = t;
        }
        if (threadIdx.x == 0) {
            uint64_t t = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int w = 0; w < kJoinThreads / 64; ++w) t += s_wave[q][w];
            p.tile_counts[blockIdx.x] = t;
        }
        return;
    }
    const uint64_t chunk = b.chunk_rows;
    const uint64_t tile_end = tile0 + kJoinTileRows < p.n ? tile0 + kJoinTileRows : p.n;
    const uint64_t b0 = tile0 / chunk, b1 = (tile_end - 1) / chunk;
    const uint64_t nslots = b1 - b0 + 1 < static_cast<uint64_t>(kJoinTileBatchSlots) ? b1 - b0 + 1 : kJoinTileBatchSlots;
    for (int t = threadIdx.x; t < kJoinTileBatchSlots; t += kJoinThreads) s_batch[t] = 0;
    __syncthreads();
    uint64_t mine = 0;
    for (int k = 0; k < kJoinRowsPerThread; ++k) {
        const uint64_t row0 = tile0 + static_cast<uint64_t>(k) * kJoinThreads + static_cast<uint64_t>(wave) * 64;
        if (row0 >= p.n) break;  // wave-uniform; no barrier inside the loop
        const uint64_t i = row0 + lane;
        uint64_t c = 0;
        if (i < p.n) {
            uint64_t bits;
            const uint32_t cls = join_key(p.key, i, bits);
            uint32_t start;
            c = join_rows<KIND>(join_lookup(p.table, cls, bits, start));
        }
        mine += c;
        uint64_t incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t y = (static_cast<uint64_t>(__shfl_up(static_cast<uint32_t>(incl >> 32), d, 64)) << 32) | __shfl_up(static_cast<uint32_t>(incl), d, 64);
            if (lane >= d) incl += y;
        }
        // the run of batch bi in this step starts at lane `first`; its sum is incl(last lane) - incl(first - 1)
        const uint64_t bi = i / chunk;
        const uint64_t bstart = bi * chunk;
        const int first = bstart > row0 ? static_cast<int>(bstart - row0) : 0;
        const int src = first > 0 ? first - 1 : 0;
        const uint64_t at_src = (static_cast<uint64_t>(__shfl(static_cast<uint32_t>(incl >> 32), src, 64)) << 32) | __shfl(static_cast<uint32_t>(incl), src, 64);
        const uint64_t before = first > 0 ? at_src : 0;
        const bool last = lane == 63 || i + 1 >= p.n || i + 1 == bstart + chunk;
        if (i < p.n && last) {
            const unsigned long long sum = incl - before;
            if (sum) {
                const uint64_t slot = bi - b0;
                if (slot < static_cast<uint64_t>(kJoinTileBatchSlots)) atomicAdd(&s_batch[slot], sum);
                else atomicAdd(&b.batch_counts[bi], sum);
            }
        }
    }
    mine = wave_sum64(mine);
    if (lane == 0) s_wave[0][wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < kJoinThreads / 64; ++w) t += s_wave[0][w];
        p.tile_counts[blockIdx.x] = t;
    }
    for (uint64_t t = threadIdx.x; t < nslots; t += kJoinThreads) {
        const uint64_t bi = b0 + t;
        const uint64_t lo = bi * chunk, hi = lo + chunk < p.n ? lo + chunk : p.n;
        if (lo >= tile0 && hi <= tile0 + kJoinTileRows) b.batch_counts[bi] = s_batch[t];  // the batch lies inside this tile
        else if (s_batch[t]) atomicAdd(&b.batch_counts[bi], s_batch[t]);
    }
}
template <bool FAST, int KIND>
static __global__ __launch_bounds__(kJoinThreads) void join_probe_count_batched(JoinProbeParams p, JoinBatchParams b) {
    join_count_batched_body<FAST, KIND>(p, b);
}

// exclusive prefix of v over the workgroup, in thread order; *total = the workgroup's sum (every thread)
__device__ __forceinline__ uint64_t join_block_scan(uint64_t v, uint64_t *s_wave, uint64_t &total) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    uint64_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = (static_cast<uint64_t>(__shfl_up(static_cast<uint32_t>(incl >> 32), d, 64)) << 32) | __shfl_up(static_cast<uint32_t>(incl), d, 64);
        if (lane >= d) incl += y;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kJoinThreads / 64; ++w) {
        before += w < wave ? s_wave[w] : 0;
        all += s_wave[w];
    }
    __syncthreads();
    total = all;
    return before + incl - v;
}

// Pass 2: the pairs of a tile at its prefix, rows in order.  MODE 0: every list holds at most one row (unique build keys, the
// foreign-key join): a stream compaction, positions from a ballot.  MODE 1: lists of at most lane_most rows, each written by its
// lane.  MODE 2: longer lists as well -- queued in LDS and written by the whole workgroup, so that a key with thousands of build
// rows does not serialise on one lane.
// KIND: JOIN_OUTER / JOIN_FULL write (row, kJoinNone) for a probe row without a match, at its place.  JOIN_SEMI / JOIN_ANTI keep
// or drop a probe row as a whole and write its index only: always MODE 0's compaction, whatever the lists' lengths.
template <int MODE, int KIND>
__device__ __forceinline__ void join_emit_body(const JoinProbeParams p) {
    constexpr bool kPairs = KIND != JOIN_SEMI && KIND != JOIN_ANTI;
    constexpr bool kKeepsMisses = KIND == JOIN_OUTER || KIND == JOIN_FULL;
    static_assert(kPairs || MODE == 0, "semi and anti joins are compactions");
    __shared__ uint64_t s_wave[kJoinThreads / 64];
    __shared__ uint64_t s_q_out[kJoinThreads], s_q_row[kJoinThreads];
    __shared__ uint32_t s_q_start[kJoinThreads], s_q_count[kJoinThreads];
    __shared__ uint32_t s_q_n;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    uint64_t out = p.tile_counts[blockIdx.x];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kJoinTileRows + threadIdx.x;
    if (MODE == 2 && threadIdx.x == 0) s_q_n = 0;
    for (int k = 0; k < kJoinRowsPerThread; ++k) {
        const uint64_t i = base + static_cast<uint64_t>(k) * kJoinThreads;
        if (static_cast<uint64_t>(blockIdx.x) * kJoinTileRows + static_cast<uint64_t>(k) * kJoinThreads >= p.n) break;  // workgroup-uniform
        uint32_t count = 0, start = 0;
        if (i < p.n) {
            uint64_t bits;
            const uint32_t cls = join_key(p.key, i, bits);
            count = join_lookup(p.table, cls, bits, start);
        }
        if (MODE == 0) {
            const bool keep = KIND == JOIN_INNER ? count != 0 : (i < p.n && join_rows<KIND>(count) != 0);
            const uint64_t m = ballot64(keep);
            if (lane == 0) s_wave[wave] = __popcll(m);
            __syncthreads();
            uint64_t before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < kJoinThreads / 64; ++w) {
                before += w < wave ? s_wave[w] : 0;
                all += s_wave[w];
            }
            if (keep) {
                const uint64_t o = out + before + __popcll(m & low_mask(lane));
                p.out_probe[o] = static_cast<int64_t>(i);
                if (kPairs) p.out_build[o] = (!kKeepsMisses || count) ? static_cast<int64_t>(p.table.rows[start]) : static_cast<int64_t>(kJoinNone);
            }
            out += all;
            __syncthreads();
        } else {
            const uint32_t rows = KIND == JOIN_INNER ? count : (i < p.n ? join_rows<KIND>(count) : 0u);
            uint64_t all;
            const uint64_t o = out + join_block_scan(rows, s_wave, all);
            if (MODE == 2 && count > p.lane_most) {
                const uint32_t q = atomicAdd(&s_q_n, 1u);
                s_q_out[q] = o;
                s_q_row[q] = i;
                s_q_start[q] = start;
                s_q_count[q] = count;
            } else {
                for (uint32_t j = 0; j < count; ++j) {
                    p.out_probe[o + j] = static_cast<int64_t>(i);
                    p.out_build[o + j] = p.table.rows[start + j];
                }
                if (kKeepsMisses && rows && !count) {
                    p.out_probe[o] = static_cast<int64_t>(i);
                    p.out_build[o] = static_cast<int64_t>(kJoinNone);
                }
            }
            out += all;
            if (MODE == 2) {
                __syncthreads();
                const uint32_t nq = s_q_n;
                for (uint32_t q = 0; q < nq; ++q) {
                    const uint64_t qo = s_q_out[q], qr = s_q_row[q];
                    const uint32_t qs = s_q_start[q], qc = s_q_count[q];
                    for (uint32_t j = threadIdx.x; j < qc; j += kJoinThreads) {
                        p.out_probe[qo + j] = static_cast<int64_t>(qr);
                        p.out_build[qo + j] = p.table.rows[qs + j];
                    }
                }
                __syncthreads();
                if (threadIdx.x == 0) s_q_n = 0;
                __syncthreads();
            }
        }
    }
}
template <int MODE, int KIND>
static __global__ __launch_bounds__(kJoinThreads) void join_probe_emit(JoinProbeParams p) { join_emit_body<MODE, KIND>(p); }

// ---- full outer join: the build rows no probe row met ----------------------------------------------------------------------------
// marks (one bit per slot, bit `slots` for the null group) -> a bitmap of the build rows of the marked groups.  A wave takes 64 slots:
// short groups are set by their lane, longer ones by the whole wave.  The bits are ORed in: the bitmap is the same whatever order
// the atomics land in.  Rows in no group (NaN keys) are never set.
constexpr uint32_t kJoinMarkLaneMost = 8;
static __global__ __launch_bounds__(256) void join_mark_rows(JoinTableView t, const uint32_t *marks, unsigned long long *matched) {
    const int lane = lane_id();
    const uint64_t nslots = t.slot_mask + 1;
    const uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;  // group: a slot, or nslots for the null group
    uint32_t start = 0, count = 0;
    if (g <= nslots && ((marks[g >> 5] >> (g & 31)) & 1)) {
        if (g == nslots) {
            start = t.null_start;
            count = t.null_count;
        } else {
            const uint64_t y = t.slots[2 * g + 1];
            start = static_cast<uint32_t>(y);
            count = static_cast<uint32_t>(y >> 32);
        }
    }
    if (count <= kJoinMarkLaneMost)
        for (uint32_t j = 0; j < count; ++j) {
            const uint32_t r = t.rows[start + j];
            atomicOr(&matched[r >> 6], 1ull << (r & 63));
        }
    uint64_t wide = ballot64(count > kJoinMarkLaneMost);
    while (wide) {  // wave-uniform
        const int src = __ffsll(static_cast<long long>(wide)) - 1;
        wide &= wide - 1;
        const uint32_t s = __shfl(start, src, 64), c = __shfl(count, src, 64);
        for (uint32_t j = lane; j < c; j += 64) {
            const uint32_t r = t.rows[s + j];
            atomicOr(&matched[r >> 6], 1ull << (r & 63));
        }
    }
}

// unmatched = the complement of `matched` over [0, n), bits past the last row zero; *count += its set bits
static __global__ __launch_bounds__(256) void join_unmatched_words(const unsigned long long *matched, uint64_t n, uint64_t *unmatched, unsigned long long *count) {
    const uint64_t nwords = (n + 63) / 64;
    unsigned long long pop = 0;
    for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; w < nwords; w += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t u = ~matched[w] & low_mask(n - w * 64);
        unmatched[w] = u;
        pop += __popcll(u);
    }
    pop = wave_sum64(pop);
    if (lane_id() == 0 && pop) atomicAdd(count, pop);
}

// the tail of the full outer join: (none, b) for the unmatched build rows, ascending
static __global__ __launch_bounds__(256) void join_unmatched_tail(const uint64_t *rows, uint64_t n, int64_t *out_probe, int64_t *out_build) {
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < n; j += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        out_probe[j] = static_cast<int64_t>(kJoinNone);
        out_build[j] = static_cast<int64_t>(rows[j]);
    }
}

// An index buffer with kJoinNone cells as a nullable Int64 column: the validity words, 0 under a null, *valid_pop += the valid cells.
static __global__ __launch_bounds__(256) void join_index_nulls(int64_t *idx, uint64_t n, uint64_t *validity, unsigned long long *valid_pop) {
    const int lane = lane_id();
    const uint64_t nchunks = (n + 63) / 64;
    const uint64_t wave0 = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = (static_cast<uint64_t>(gridDim.x) * blockDim.x) >> 6;
    unsigned long long pop = 0;
    for (uint64_t c = wave0; c < nchunks; c += nwaves) {
        const uint64_t i = c * 64 + lane;
        bool valid = false;
        if (i < n) {
            valid = static_cast<uint64_t>(idx[i]) != kJoinNone;
            if (!valid) idx[i] = 0;
        }
        const uint64_t m = ballot64(valid);
        if (lane == 0) {
            validity[c] = m;
            pop += static_cast<unsigned long long>(__popcll(m));
        }
    }
    if (lane == 0 && pop) atomicAdd(valid_pop, pop);
}

}  // namespace rvk
