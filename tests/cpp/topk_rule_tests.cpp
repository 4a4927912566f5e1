// CPU test of the decisions of the top-k select (rivulus_amd/csrc/topk_rule.hpp): a stand-alone program, built with
// g++ -fsanitize=address,undefined by tests/test_topk_cpu.py and run as a program.
//
//   choose_bin    against a plain restatement (sort the values, look at the r-th) at r = 1, r = a bin's exact inclusive count (the cut is
//                 the last row of a bin), that + 1, r = the total; a histogram with one used bin; the used bins 0 and 255; random histograms
//   null_class    the four cases of the null class, on either side of m == k and v == k
//   high_above    position 7 has nothing above it (a shift by 64 would be undefined, and on the hardware is not 0)
//   refine_more   the stop rule on either side of n / divisor, with and without positions left
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../rivulus_amd/csrc/topk_rule.hpp"

static int failures = 0;
static long checks = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        ++checks;                                                         \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static uint64_t next_random(uint64_t &s) {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

// the bin of the r-th smallest digit (r from 1), by walking the digits one at a time -- not by prefix sums over the bins
static void check_choice(const std::vector<unsigned long long> &hist, uint64_t r) {
    std::vector<uint32_t> digits;
    for (uint32_t b = 0; b < 256; ++b)
        for (unsigned long long i = 0; i < hist[b]; ++i) digits.push_back(b);
    CHECK(r >= 1 && r <= digits.size());
    const uint32_t want = digits[r - 1];
    uint64_t below = 0;
    for (uint32_t d : digits) below += d < want;
    const rvtopk::BinChoice c = rvtopk::choose_bin(hist.data(), r);
    CHECK(c.bin == want);
    CHECK(c.below == below);
    CHECK(c.in_bin == hist[want]);
    CHECK(c.below < r && r <= c.below + c.in_bin);
}

static void check_edges(const std::vector<unsigned long long> &hist) {
    uint64_t total = 0, incl = 0;
    for (auto c : hist) total += c;
    if (total == 0) return;
    check_choice(hist, 1);
    check_choice(hist, total);
    for (uint32_t b = 0; b < 256; ++b) {
        if (!hist[b]) continue;
        incl += hist[b];
        check_choice(hist, incl);                       // the cut is the last row of a bin
        if (incl + 1 <= total) check_choice(hist, incl + 1);  // ... and the first row of the next used bin
        if (incl - hist[b] + 1 <= total) check_choice(hist, incl - hist[b] + 1);
    }
}

int main() {
    std::vector<unsigned long long> h(256, 0);
    // one used bin, at either end and in the middle
    for (uint32_t b : {0u, 255u, 17u}) {
        h.assign(256, 0);
        h[b] = 5;
        check_edges(h);
        for (uint64_t r = 1; r <= 5; ++r) CHECK(rvtopk::choose_bin(h.data(), r).bin == b && rvtopk::choose_bin(h.data(), r).below == 0);
    }
    // the used bins 0 and 255
    h.assign(256, 0);
    h[0] = 3;
    h[255] = 4;
    check_edges(h);
    CHECK(rvtopk::choose_bin(h.data(), 3).bin == 0);
    CHECK(rvtopk::choose_bin(h.data(), 4).bin == 255 && rvtopk::choose_bin(h.data(), 4).below == 3);
    CHECK(rvtopk::choose_bin(h.data(), 7).bin == 255 && rvtopk::choose_bin(h.data(), 7).in_bin == 4);
    // every bin used once
    h.assign(256, 1);
    check_edges(h);
    // counts past 2^32 stay 64-bit
    h.assign(256, 0);
    h[3] = 5000000000ull;
    h[200] = 7000000000ull;
    CHECK(rvtopk::choose_bin(h.data(), 5000000000ull).bin == 3);
    CHECK(rvtopk::choose_bin(h.data(), 5000000001ull).bin == 200 && rvtopk::choose_bin(h.data(), 5000000001ull).below == 5000000000ull);
    CHECK(rvtopk::choose_bin(h.data(), 12000000000ull).bin == 200);
    // random histograms: sparse and dense
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    for (int round = 0; round < 300; ++round) {
        h.assign(256, 0);
        const int used = 1 + static_cast<int>(next_random(seed) % (round % 2 ? 6 : 256));
        for (int i = 0; i < used; ++i) h[next_random(seed) % 256] += 1 + next_random(seed) % 9;
        check_edges(h);
        uint64_t total = 0;
        for (auto c : h) total += c;
        for (int i = 0; i < 8; ++i) check_choice(h, 1 + next_random(seed) % total);
    }

    // the null class: n = 10 rows
    using rvtopk::null_class;
    {   // nulls first
        rvtopk::NullClass c = null_class(10, 6, 4, false);  // m == k
        CHECK(c.kind == rvtopk::kNullsOnly);
        c = null_class(10, 6, 3, false);  // m > k
        CHECK(c.kind == rvtopk::kNullsOnly);
        c = null_class(10, 6, 5, false);  // m < k
        CHECK(c.kind == rvtopk::kValues && c.r == 1 && c.nulls_taken);
        c = null_class(10, 10, 5, false);  // no nulls
        CHECK(c.kind == rvtopk::kValues && c.r == 5 && !c.nulls_taken);
        c = null_class(10, 0, 5, false);  // only nulls
        CHECK(c.kind == rvtopk::kNullsOnly);
    }
    {   // nulls last
        rvtopk::NullClass c = null_class(10, 6, 6, true);  // v == k
        CHECK(c.kind == rvtopk::kValues && c.r == 6 && !c.nulls_taken);
        c = null_class(10, 6, 5, true);
        CHECK(c.kind == rvtopk::kValues && c.r == 5 && !c.nulls_taken);
        c = null_class(10, 6, 7, true);  // v < k
        CHECK(c.kind == rvtopk::kEveryRow);
        c = null_class(10, 0, 1, true);
        CHECK(c.kind == rvtopk::kEveryRow);
    }
    for (uint64_t n = 2; n < 40; ++n)
        for (uint64_t v = 0; v <= n; ++v)
            for (uint64_t k = 1; k < n; ++k)
                for (int last = 0; last < 2; ++last) {
                    const rvtopk::NullClass c = null_class(n, v, k, last != 0);
                    if (c.kind == rvtopk::kValues) CHECK(c.r >= 1 && c.r <= v && c.r + (c.nulls_taken ? n - v : 0) == k);
                    if (c.kind == rvtopk::kNullsOnly) CHECK(!last && n - v >= k);
                    if (c.kind == rvtopk::kEveryRow) CHECK(last && v < k);
                }

    // prefixes
    const uint64_t key = 0x0123456789ABCDEFull;
    CHECK(rvtopk::high_above(key, 7) == 0);
    CHECK(rvtopk::high_above(~0ull, 7) == 0);
    CHECK(rvtopk::high_above(key, 6) == 0x01);
    CHECK(rvtopk::high_above(key, 0) == 0x0123456789ABCDull);
    CHECK(rvtopk::high_from(key, 7) == 0x01 && rvtopk::high_from(key, 0) == key);
    for (uint32_t pos = 0; pos < 8; ++pos) {
        CHECK(rvtopk::high_from(rvtopk::with_digit(key, pos, 0x5A), pos) == ((rvtopk::high_above(key, pos) << 8) | 0x5A));
        CHECK(rvtopk::with_digit(rvtopk::with_digit(key, pos, 0), pos, (key >> (8 * pos)) & 0xFF) == key);
        CHECK(rvtopk::highest_position(1ull << pos) == pos && rvtopk::highest_position((1ull << pos) | 1) == pos);
    }

    // the stop rule
    CHECK(rvtopk::refine_more(33, 1024, 32, 0x0F));
    CHECK(!rvtopk::refine_more(32, 1024, 32, 0x0F));
    CHECK(!rvtopk::refine_more(1000, 1024, 32, 0));
    CHECK(rvtopk::refine_more(1, 8, 32, 1));    // 8 / 32 = 0 rows
    CHECK(!rvtopk::refine_more(8, 8, 1, 1));

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok %ld checks\n", checks);
    return 0;
}
