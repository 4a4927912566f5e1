// The decisions of the top-k select (topk_kernel.hpp, topk.hip), written once for the device and the host: plain g++ compiles this header
// for the CPU test (tests/cpp/topk_rule_tests.cpp), hipcc for the kernels and the operator.  tests/topk_model.py restates it in numpy.
//   null_class    which rows the first k of the sort can come from, by the counts alone: m null rows, v non-null ones, nulls first or last
//   choose_bin    from a 256-bin histogram and the number r of values still owed: the smallest bin whose inclusive prefix count reaches r
//   high_above    the part of a working key above digit position `pos` -- position 7 has nothing above it, and a shift by 64 is not 0
//   refine_more   the stop rule
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RVTOPK_HD __host__ __device__ inline
#else
#define RVTOPK_HD inline
#endif

namespace rvtopk {

constexpr int kBins = 256;
constexpr int kPositions = 8;

enum : int {
    kNullsOnly = 0,  // nulls first and at least k of them: the candidates are the null rows alone
    kValues = 1,     // `r` of the first k are values: select among them (`nulls_taken`: every null row is a candidate too)
    kEveryRow = 2    // nulls last and fewer than k values: every row is a candidate
};
struct NullClass {
    int kind;
    uint64_t r;        // kValues: values owed, 1 <= r <= v
    bool nulls_taken;  // kValues: the null rows precede the values and are all candidates
};
// 0 < k < n = m + v
RVTOPK_HD NullClass null_class(uint64_t n, uint64_t v, uint64_t k, bool nulls_last) {
    const uint64_t m = n - v;
    if (!nulls_last) {
        if (m >= k) return {kNullsOnly, 0, false};
        return {kValues, k - m, m > 0};
    }
    if (v >= k) return {kValues, k, false};
    return {kEveryRow, 0, false};
}

struct BinChoice {
    uint32_t bin;
    uint64_t below;   // the count strictly below `bin`
    uint64_t in_bin;  // the count of `bin`: below < r <= below + in_bin
};
// 1 <= r <= the histogram's total.  (An r past the total ends at the last bin: nothing here reads out of bounds.)
RVTOPK_HD BinChoice choose_bin(const unsigned long long *hist, uint64_t r) {
    uint64_t below = 0;
    for (uint32_t b = 0; b + 1 < static_cast<uint32_t>(kBins); ++b) {
        const uint64_t c = hist[b];
        if (below + c >= r) return {b, below, c};
        below += c;
    }
    return {static_cast<uint32_t>(kBins - 1), below, static_cast<uint64_t>(hist[kBins - 1])};
}

// bits [8 x (pos + 1), 64) of the key, moved down; nothing lies above position 7
RVTOPK_HD uint64_t high_above(uint64_t key, uint32_t pos) { return pos >= static_cast<uint32_t>(kPositions - 1) ? 0 : key >> (8 * (pos + 1)); }
// bits [8 x pos, 64): what a candidate's key is compared by after the pass at `pos`
RVTOPK_HD uint64_t high_from(uint64_t key, uint32_t pos) { return key >> (8 * pos); }
RVTOPK_HD uint64_t with_digit(uint64_t prefix, uint32_t pos, uint32_t digit) {
    return (prefix & ~(0xFFull << (8 * pos))) | (static_cast<uint64_t>(digit) << (8 * pos));
}

// One more pass over the key column pays while the candidates it could shed cost more to sort than the pass costs to run: `remaining` is
// the mask of differing positions below the last one taken, `divisor` rvt::kTopKRefineDivisor (thresholds.hpp has the derivation).
RVTOPK_HD bool refine_more(uint64_t candidates, uint64_t n, uint64_t divisor, uint64_t remaining) { return remaining != 0 && candidates > n / divisor; }
// the highest set bit of a non-zero mask of positions
RVTOPK_HD uint32_t highest_position(uint64_t mask) {
    uint32_t p = 0;
    for (uint32_t q = 0; q < static_cast<uint32_t>(kPositions); ++q)
        if ((mask >> q) & 1) p = q;
    return p;
}

}  // namespace rvtopk
