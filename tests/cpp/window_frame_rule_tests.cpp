// CPU test of csrc/window_frame_rule.hpp, the frame rule of rv_window_frames: a stand-alone program, built by plain g++ under
// -fsanitize=address,undefined and run directly (tests/test_window_frame_cpu.py).  For every partition length up to 40, every signed
// offset pair in [-45, 45] plus both unbounded ends and +-2^62 that the C ABI takes, and every position:
//   * lo / hi / empty against the header's sentence, computed in 128-bit arithmetic;
//   * the chosen case reproduces the brute-force SUM (wrapping) and MIN of random cells through block prefix / suffix arrays built by
//     sequential loops over the blocks the rule implies;
// and frame_ok against the sentence, NTILE's closed form against dealing the rows out one by one.
// Prints "ok <checks>" and exits 0, or the first failure and exits 1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../rivulus_amd/csrc/window_frame_rule.hpp"

using namespace rvframe;

namespace {

unsigned long long checks = 0;
std::mt19937_64 rng(12);

[[noreturn]] void fail(const char *what, long long len, long long p, long long f, long long pos) {
    std::printf("FAIL %s (len %lld, preceding %lld, following %lld, pos %lld)\n", what, len, p, f, pos);
    std::exit(1);
}

std::vector<int64_t> offsets() {
    std::vector<int64_t> v;
    for (int64_t k = -45; k <= 45; ++k) v.push_back(k);
    v.push_back(kUnbounded);
    v.push_back(kOffsetMost);
    v.push_back(-kOffsetMost);
    return v;
}

bool ok_by_the_sentence(int64_t p, int64_t f) {
    const __int128 most = static_cast<__int128>(1) << 62;
    const bool pu = p == kUnbounded, fu = f == kUnbounded;
    if (!pu && (p < -most || p > most)) return false;
    if (!fu && (f < -most || f > most)) return false;
    return pu || fu || static_cast<__int128>(p) + f >= 0;
}

void frames() {
    const std::vector<int64_t> offs = offsets();
    for (uint32_t len = 1; len <= 40; ++len) {
        std::vector<uint64_t> x(len + 1);
        for (uint64_t &c : x) c = rng() % 3 == 0 ? rng() % 5 : rng();
        for (int64_t p : offs)
            for (int64_t f : offs) {
                if (frame_ok(p, f) != ok_by_the_sentence(p, f)) fail("frame_ok", len, p, f, 0);
                ++checks;
                if (!frame_ok(p, f)) continue;
                const Frame fr = frame_of(p, f);
                // the blocks the rule implies: of fr.width positions, or the whole partition
                const uint32_t w = fr.width == 0 || fr.width >= len ? len : static_cast<uint32_t>(fr.width);
                std::vector<uint64_t> pre_sum(len + 1), suf_sum(len + 2), pre_min(len + 1), suf_min(len + 2);
                for (uint32_t i = 1; i <= len; ++i) {
                    const bool head = (i - 1) % w == 0;
                    pre_sum[i] = head ? x[i] : pre_sum[i - 1] + x[i];
                    pre_min[i] = head ? x[i] : (pre_min[i - 1] < x[i] ? pre_min[i - 1] : x[i]);
                }
                for (uint32_t i = len; i >= 1; --i) {
                    const bool tail = i == len || i % w == 0;
                    suf_sum[i] = tail ? x[i] : suf_sum[i + 1] + x[i];
                    suf_min[i] = tail ? x[i] : (suf_min[i + 1] < x[i] ? suf_min[i + 1] : x[i]);
                }
                for (uint32_t pos = 1; pos <= len; ++pos) {
                    const __int128 first = p == kUnbounded ? 1 : static_cast<__int128>(pos) - p, last = f == kUnbounded ? len : static_cast<__int128>(pos) + f;
                    const __int128 lo = first < 1 ? 1 : first, hi = last > len ? len : last;
                    const Pick k = frame_pick(fr, pos, len);
                    ++checks;
                    if ((lo > hi) != (k.which == FC_EMPTY)) fail("empty", len, p, f, pos);
                    if (lo > hi) continue;
                    if (k.lo != lo || k.hi != hi) fail("lo / hi", len, p, f, pos);
                    uint64_t sum = 0, min = ~0ull;
                    for (uint32_t i = k.lo; i <= k.hi; ++i) {
                        sum += x[i];
                        min = x[i] < min ? x[i] : min;
                    }
                    uint64_t got_sum, got_min;
                    if (k.which == FC_PREFIX) got_sum = pre_sum[k.hi], got_min = pre_min[k.hi];
                    else if (k.which == FC_SUFFIX) got_sum = suf_sum[k.lo], got_min = suf_min[k.lo];
                    else if (k.which == FC_BOTH) {
                        got_sum = suf_sum[k.lo] + pre_sum[k.hi];
                        got_min = suf_min[k.lo] < pre_min[k.hi] ? suf_min[k.lo] : pre_min[k.hi];
                    } else fail("an unknown case", len, p, f, pos);
                    if (got_sum != sum) fail("SUM through the chosen case", len, p, f, pos);
                    if (got_min != min) fail("MIN through the chosen case", len, p, f, pos);
                    // what the host relies on: an unbounded preceding side never asks for the suffix, an unbounded following side never for the prefix
                    if (fr.preceding_unbounded && k.which != FC_PREFIX) fail("unbounded preceding took the suffix", len, p, f, pos);
                    if (!fr.preceding_unbounded && fr.following_unbounded && k.which != FC_SUFFIX) fail("unbounded following took the prefix", len, p, f, pos);
                }
            }
    }
}

void ntile() {
    for (uint64_t len = 1; len <= 60; ++len)
        for (uint64_t n : {1ull, 2ull, 3ull, 4ull, 5ull, 7ull, 8ull, 16ull, 59ull, 60ull, 61ull, 1000ull, ~0ull}) {
            const uint64_t q = len / n, r = len % n;
            uint64_t bucket = 1, room = r >= 1 ? q + 1 : q;  // deal the rows out: the first r buckets take q + 1, the rest q
            for (uint64_t pos = 1; pos <= len; ++pos) {
                if (room == 0) {
                    ++bucket;
                    room = bucket <= r ? q + 1 : q;
                }
                --room;
                if (ntile_bucket(pos, len, n) != bucket) fail("NTILE", static_cast<long long>(len), static_cast<long long>(n), 0, static_cast<long long>(pos));
                ++checks;
            }
        }
}

}  // namespace

int main() {
    frames();
    ntile();
    std::printf("ok %llu\n", checks);
    return 0;
}
