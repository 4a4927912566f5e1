// Device string dictionary (string_dict.hip): the distinct non-null strings of a String column, each named by the row of its
// FIRST occurrence -- what reduces a String join key to the 64 key bits per cell the join kernels are built around.
//
// Layout of a dictionary:
//   slots  open addressing, a power of two >= rvt::kStrDictSlotsPerRow x the non-null rows, linear probing; ONE 64-bit word per
//          distinct string: hash_high32 << 32 | (row + 1), 0: empty.  The word is published by a single compare-and-swap, so no
//          reader ever sees half a slot (no second launch, as the join's heads / tails need); the string's bytes are those of
//          `row` in the source column, which the dictionary keeps alive and nobody writes.
// The tag (the hash's high half) only spares byte compares: a hit is a hit once string_equal has confirmed the bytes.
// A slot's tag never changes once claimed and its row only ever falls (atomicMin: same tag, so the smaller word is the smaller
// row), to the string's first row -- the ids do not depend on the order the atomics land in; which slot a string sits in may.
// Every chain walk is bounded by the slot count; a walk that runs out raises StrDictParams::error (RV_ERR_INTERNAL on the host).
#pragma once

#include "device_common.hpp"
#include "string_hash.hpp"

namespace rvk {

constexpr int kStrDictThreads = 256;

// a StringArray as the kernels read it (string.rs:9-17): cell i is data[offsets[offset + i], offsets[offset + i + 1])
struct StrColView {
    const int32_t *offsets;
    const uint8_t *data;
    const uint8_t *validity;  // or nullptr
    uint64_t offset;
};

struct StrDictParams {
    unsigned long long *slots;
    uint64_t slot_mask;  // slots - 1
    uint64_t hash_mask;  // ~0, or the low bits option "string_hash_bits" leaves (collision tests)
    StrColView source;   // the column the dictionary was built from: the bytes behind every slot's row
    StrColView col;      // the column of this launch (insert: the source itself)
    uint64_t n;          // rows of `col`
    int64_t *ids;                     // encode: [n]
    unsigned long long *valid_count;  // encode: striped counter of the non-null rows (nullptr: the column has no bitmap)
    unsigned long long *distinct;     // insert: striped counter of the slots claimed
    uint32_t *error;                  // set when a chain walk exhausted the table
};

__device__ __forceinline__ bool str_cell(const StrColView &c, uint64_t i, const uint8_t *&p, uint64_t &len) {
    const uint64_t at = c.offset + i;
    if (c.validity && !((c.validity[at >> 3] >> (at & 7)) & 1)) return false;
    const int32_t b = c.offsets[at], e = c.offsets[at + 1];
    p = c.data + b;
    len = static_cast<uint64_t>(e - b);
    return true;
}

// does the string of source row `row` equal [p, p + len)?
__device__ __forceinline__ bool str_slot_equal(const StrColView &src, uint32_t row, const uint8_t *p, uint64_t len) {
    const uint64_t at = src.offset + row;
    const int32_t b = src.offsets[at], e = src.offsets[at + 1];
    return rvstr::string_equal(src.data + b, static_cast<uint64_t>(e - b), p, len);
}

// One lane per row: the row's string claims a free slot of its chain, or lowers the row of the slot that already holds it.
static __global__ __launch_bounds__(kStrDictThreads) void str_dict_insert(const StrDictParams q) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kStrDictThreads + threadIdx.x;
    bool claimed = false;
    const uint8_t *p = nullptr;
    uint64_t len = 0;
    if (i < q.n && str_cell(q.col, i, p, len)) {
        const uint64_t h = rvstr::string_hash(p, len) & q.hash_mask;
        const unsigned long long mine = (h & 0xFFFFFFFF00000000ull) | (i + 1);
        uint64_t s = h & q.slot_mask;
        bool placed = false;
        for (uint64_t step = 0; step <= q.slot_mask && !placed; ++step, s = (s + 1) & q.slot_mask) {
            // (an L1 line another CU's atomic has outdated only costs a failed compare-and-swap: its return value is current)
            unsigned long long e = __hip_atomic_load(&q.slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (e == 0) {
                e = atomicCAS(&q.slots[s], 0ull, mine);
                if (e == 0) {
                    claimed = placed = true;
                    break;
                }
                // lost the slot: another row of the SAME string may have taken it -- look at what it holds now
            }
            if ((e >> 32) == (mine >> 32) && str_slot_equal(q.source, static_cast<uint32_t>(e) - 1, p, len)) {
                if (mine < e) atomicMin(&q.slots[s], mine);
                placed = true;
            }
        }
        if (!placed) atomicOr(q.error, 1u);
    }
    const uint64_t m = ballot64(claimed);
    if (lane_id() == 0 && m) striped_add(q.distinct, __popcll(m));
}

// One lane per row: the id of the row's string (the first row that holds it in the source), -1 for a string the dictionary
// does not hold, 0 under a null (the bitmap is re-based by copy_bits_kernel).
static __global__ __launch_bounds__(kStrDictThreads) void str_dict_encode(const StrDictParams q) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kStrDictThreads + threadIdx.x;
    bool valid = false;
    if (i < q.n) {
        const uint8_t *p = nullptr;
        uint64_t len = 0;
        valid = str_cell(q.col, i, p, len);
        int64_t id = valid ? -1 : 0;
        if (valid) {
            const uint64_t h = rvstr::string_hash(p, len) & q.hash_mask;
            const uint32_t tag = static_cast<uint32_t>(h >> 32);
            uint64_t s = h & q.slot_mask;
            bool found = false;
            for (uint64_t step = 0; step <= q.slot_mask && !found; ++step, s = (s + 1) & q.slot_mask) {
                const unsigned long long e = q.slots[s];
                if (e == 0) {
                    found = true;  // the end of the chain: absent
                } else if (static_cast<uint32_t>(e >> 32) == tag && str_slot_equal(q.source, static_cast<uint32_t>(e) - 1, p, len)) {
                    id = static_cast<int64_t>(static_cast<uint32_t>(e)) - 1;
                    found = true;
                }
            }
            if (!found) atomicOr(q.error, 1u);
        }
        q.ids[i] = id;
    }
    if (q.valid_count) {
        const uint64_t m = ballot64(valid);
        if (lane_id() == 0 && m) striped_add(q.valid_count, __popcll(m));
    }
}

}  // namespace rvk
