// CPU test of the segmented bit count's work list (rivulus_amd/csrc/segment_items.hpp, shared by segment_popcount_kernel and
// its host driver): a stand-alone program, built with AddressSanitizer and UBSan by tests/test_segment_items_cpu.py.
//   - the items read the way the kernel reads them -- chunk c of range k is the words [w0 + c * chunk_words, min(.. + chunk_words
//     - 1, w1)], edge masks at w0 and w1 -- give every range's bit-by-bit count, and cover every word of every non-empty range
//     exactly once;
//   - chunk_words is a multiple of 64, never below kSegChunkWords;
//   - 2^32 ranges are refused before the bounds are read.
// Output: "ok <checks>" / "FAIL why"; exit status 0 iff all pass.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>

#include "../../rivulus_amd/csrc/segment_items.hpp"

namespace {
uint64_t g_checks = 0;
#define CHECK(cond) \
    do { \
        ++g_checks; \
        if (!(cond)) { \
            std::printf("FAIL %s:%d CHECK(%s)\n", __FILE__, __LINE__, #cond); \
            std::exit(1); \
        } \
    } while (0)

uint64_t low_mask(uint64_t n) { return n >= 64 ? ~0ull : (uint64_t{1} << n) - 1; }  // device_common.hpp's

void check_bounds(const std::vector<uint64_t> &bounds, uint64_t cus, std::mt19937_64 &rng, bool expect_long_range = false) {
    const uint64_t nb = bounds.size() - 1;
    std::vector<uint64_t> words((bounds.back() + 63) / 64 + 1);
    for (auto &w : words) w = rng();
    std::vector<rvk::SegItem> items;
    uint64_t chunk_words = 0;
    CHECK(rvk::segment_items(bounds.data(), nb, cus, items, chunk_words) == RV_OK);
    CHECK(chunk_words % 64 == 0 && chunk_words >= rvk::kSegChunkWords);
    std::vector<uint64_t> counts(nb, 0);
    std::map<std::pair<uint32_t, uint64_t>, int> covered;  // (range, word) -> times read
    uint32_t most_chunks = 0;
    for (const rvk::SegItem it : items) {  // segment_popcount_kernel's loop body, one lane
        CHECK(it.segment < nb);
        const uint64_t lo = bounds[it.segment], hi = bounds[it.segment + 1];
        CHECK(hi > lo);  // no item for an empty range
        const uint64_t w0 = lo >> 6, w1 = (hi - 1) >> 6;
        const uint64_t c0 = w0 + static_cast<uint64_t>(it.chunk) * chunk_words;
        const uint64_t c1 = c0 + chunk_words - 1 < w1 ? c0 + chunk_words - 1 : w1;
        CHECK(c0 <= w1);  // no item past its range
        for (uint64_t w = c0; w <= c1; ++w) {
            uint64_t x = words.at(w);
            if (w == w0) x &= ~low_mask(lo & 63);
            if (w == w1 && (hi & 63)) x &= low_mask(hi & 63);
            counts[it.segment] += static_cast<uint64_t>(__builtin_popcountll(x));
            ++covered[{it.segment, w}];
        }
        most_chunks = std::max(most_chunks, it.chunk + 1);
    }
    if (expect_long_range) CHECK(most_chunks >= 3);
    uint64_t range_words = 0;
    for (uint64_t k = 0; k < nb; ++k) {
        uint64_t bits = 0;
        for (uint64_t i = bounds[k]; i < bounds[k + 1]; ++i) bits += (words[i >> 6] >> (i & 63)) & 1;
        CHECK(counts[k] == bits);
        if (bounds[k + 1] > bounds[k]) range_words += rvk::seg_range_words(bounds[k], bounds[k + 1]);
    }
    CHECK(covered.size() == range_words);
    for (auto &kv : covered) CHECK(kv.second == 1);
}
}  // namespace

int main() {
    std::mt19937_64 rng(20240611);
    for (uint64_t cus : {uint64_t{1}, uint64_t{256}}) {
        // hand-made: empty ranges at both ends and in the middle, two ranges inside one word, boundaries on and off word edges
        check_bounds({0, 0, 5, 5, 37, 64, 64, 129, 4096, 4097, 4097}, cus, rng);
        check_bounds({0, 0}, cus, rng);
        check_bounds({0}, cus, rng);  // no range at all
        // one range longer than 2 * chunk_words among short ones: three chunks
        const uint64_t long_bits = 2 * 64 * rvk::kSegChunkWords + 131;
        check_bounds({3, 41, 41 + long_bits, 41 + long_bits + 1, 41 + long_bits + 1000}, cus, rng, true);
        // ... and where the chunks grow with the bitmap (one CU: an eighth of all words each)
        check_bounds({3, 41, 41 + 24 * long_bits, 41 + 24 * long_bits + 1000}, cus, rng, true);
        for (int round = 0; round < 40; ++round) {
            std::vector<uint64_t> b = {rng() % 130};
            const int nb = 1 + static_cast<int>(rng() % 12);
            for (int k = 0; k < nb; ++k) {
                const uint64_t kind = rng() % 5;
                const uint64_t len = kind == 0 ? 0 : kind == 1 ? rng() % 64 : kind == 2 ? 64 * (rng() % 5) : kind == 3 ? rng() % 5000 : rng() % 700000;
                b.push_back(b.back() + len);
            }
            check_bounds(b, cus, rng);
        }
    }
    // 2^32 ranges: refused before the bounds are read (there are none)
    std::vector<rvk::SegItem> items;
    uint64_t chunk_words = 0;
    CHECK(rvk::segment_items(nullptr, uint64_t{1} << 32, 256, items, chunk_words) == RV_ERR_UNSUPPORTED);
    CHECK(items.empty());
    std::printf("ok %llu\n", static_cast<unsigned long long>(g_checks));
    return 0;
}
