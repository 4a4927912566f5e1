// The work list of segment_popcount_kernel (aux_kernels.hpp), written once for the kernel and the host: plain g++ compiles this
// header for the CPU test (tests/cpp/segment_items_tests.cpp), hipcc for the library.
//
// The kernel counts the set bits of an LSB-first bitmap inside nb bit ranges [bounds[k], bounds[k + 1]).  Every non-empty range
// is cut into chunks of chunk_words 64-bit words, counted from the word its first bit lies in; one item = one chunk = one wave.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/rivulus_gpu.h"

namespace rvk {

constexpr uint64_t kSegChunkWords = 4096;
struct SegItem {
    uint32_t segment, chunk;
};

// words a range touches (hi > lo)
inline uint64_t seg_range_words(uint64_t lo, uint64_t hi) { return ((hi - 1) >> 6) - (lo >> 6) + 1; }

// The items of bounds[nb + 1] for a device of `cus` compute units, and the chunk length they are cut by: about eight items per
// CU when the ranges are long, never chunks shorter than kSegChunkWords, a multiple of 64 words.  SegItem::segment is 32-bit:
// 2^32 ranges or more are refused (RV_ERR_UNSUPPORTED) before `bounds` is read.
inline rv_status segment_items(const uint64_t *bounds, uint64_t nb, uint64_t cus, std::vector<SegItem> &items, uint64_t &chunk_words) {
    items.clear();
    chunk_words = kSegChunkWords;
    if (nb >= (uint64_t{1} << 32)) return RV_ERR_UNSUPPORTED;
    uint64_t all_words = 0;
    for (uint64_t k = 0; k < nb; ++k)
        if (bounds[k + 1] > bounds[k]) all_words += seg_range_words(bounds[k], bounds[k + 1]);
    chunk_words = std::max<uint64_t>(kSegChunkWords, (all_words / (cus * 8) + 63) & ~63ull);
    for (uint64_t k = 0; k < nb; ++k) {
        if (bounds[k + 1] <= bounds[k]) continue;
        const uint64_t nwords = seg_range_words(bounds[k], bounds[k + 1]);
        for (uint64_t c = 0; c * chunk_words < nwords; ++c) items.push_back(SegItem{static_cast<uint32_t>(k), static_cast<uint32_t>(c)});
    }
    return RV_OK;
}

}  // namespace rvk
