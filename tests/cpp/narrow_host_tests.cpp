// Stand-alone CPU test of the host-side rule of the narrow companions (rivulus_amd/csrc/narrow_rule.hpp, what narrow.hip and the
// launch code decide by): range arithmetic at the ends of Int64, the code width on either side of 2^16 and 2^32, the code's round
// trip, the alignment a slice needs, which buffers qualify, and when a buffer counts as scanned.  Prints "ok <checks>" as its last line.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "../../rivulus_amd/csrc/narrow_rule.hpp"
#include "../../rivulus_amd/csrc/thresholds.hpp"

static long g_checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

int main() {
    constexpr int64_t kMin = std::numeric_limits<int64_t>::min(), kMax = std::numeric_limits<int64_t>::max();
    using namespace rvn;

    // ---- range arithmetic: an unsigned difference, no signed overflow anywhere in Int64 ----
    CHECK(value_range(0, 0) == 0);
    CHECK(value_range(-5, 65530) == 65535);
    CHECK(value_range(kMin, kMin + 65535) == 65535);
    CHECK(value_range(kMax - 65535, kMax) == 65535);
    CHECK(value_range(kMin, kMax) == ~uint64_t{0});
    CHECK(value_range(-1, 0) == 1);
    CHECK(value_range(kMin, 0) == (uint64_t{1} << 63));
    CHECK(value_range(0, kMax) == (uint64_t{1} << 63) - 1);

    // ---- width: both sides of each edge ----
    CHECK(code_bytes(0) == 2);
    CHECK(code_bytes(65535) == 2);
    CHECK(code_bytes(65536) == 4);
    CHECK(code_bytes((uint64_t{1} << 32) - 1) == 4);
    CHECK(code_bytes(uint64_t{1} << 32) == 0);
    CHECK(code_bytes(~uint64_t{0}) == 0);
    CHECK(code_bytes(value_range(kMin, kMax)) == 0);
    CHECK(code_bytes(value_range(kMin, kMin + 65535)) == 2);
    CHECK(code_bytes(value_range(kMax - (int64_t{1} << 32) + 1, kMax)) == 4);

    // ---- code round trip: every base position, both widths' extremes, a pseudo-random sweep ----
    const int64_t bases[] = {kMin, kMin + 1, -70000, -1, 0, 1, 41, kMax - 65535, kMax - 0xFFFFFFFFll};
    for (int64_t base : bases) {
        const uint64_t room = value_range(base, kMax);
        for (uint64_t off : {uint64_t{0}, uint64_t{1}, uint64_t{65535}, uint64_t{65536}, uint64_t{0xFFFFFFFFull}}) {
            if (off > room) continue;
            const int64_t v = static_cast<int64_t>(static_cast<uint64_t>(base) + off);
            CHECK(encode(v, base) == static_cast<uint32_t>(off));
            CHECK(decode(encode(v, base), base) == v);
        }
        uint64_t x = 0x9E3779B97F4A7C15ull ^ static_cast<uint64_t>(base);
        for (int i = 0; i < 2000; ++i) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            const uint64_t off = (x & 0xFFFFFFFFull) <= room ? (x & 0xFFFFFFFFull) : room;
            const int64_t v = static_cast<int64_t>(static_cast<uint64_t>(base) + off);
            CHECK(decode(encode(v, base), base) == v);
            CHECK(value_range(base, v) == off);
        }
    }

    // ---- alignment of a slice: the pair loads need an even first element ----
    CHECK(slice_aligned(0) && slice_aligned(2) && slice_aligned(1026) && slice_aligned(uint64_t{1} << 40));
    CHECK(!slice_aligned(1) && !slice_aligned(3) && !slice_aligned(1027));

    // ---- eligibility: pool blocks (id != 0) of Int64 values without a null bitmap ----
    CHECK(buffer_eligible(7, true, false));
    CHECK(!buffer_eligible(0, true, false));  // caller-owned memory (rv_wrap): the caller may write to it
    CHECK(!buffer_eligible(7, false, false)); // Float64 / Boolean
    CHECK(!buffer_eligible(7, true, true));   // nullable

    // ---- views the codes cover ----
    CHECK(view_covered(0, 100, 100) && view_covered(2, 98, 100) && view_covered(100, 0, 100));
    CHECK(!view_covered(2, 99, 100) && !view_covered(0, 101, 100));
    CHECK(!view_covered(~uint64_t{0}, 2, 100));  // wraps

    // ---- whole scans: one pass over the column, or windows in ascending order; a slice read again and again is none ----
    {
        ScanCover c;
        c.note_pass(0, 1000);
        CHECK(c.extent == 1000 && c.whole_scans == 1 && c.covered_to == 0);
        c.note_pass(0, 1000);
        CHECK(c.whole_scans == 2);
    }
    {
        ScanCover c;
        c.note_extent(1000);  // the parent of the slices
        for (int rep = 0; rep < 5; ++rep) c.note_pass(0, 500);
        CHECK(c.whole_scans == 0 && c.covered_to == 500);
        for (int rep = 0; rep < 5; ++rep) c.note_pass(600, 400);  // a gap before it
        CHECK(c.whole_scans == 0);
        c.note_pass(500, 100);
        CHECK(c.whole_scans == 0 && c.covered_to == 600);
        c.note_pass(600, 400);
        CHECK(c.whole_scans == 1 && c.covered_to == 0);
        c.note_pass(0, 256), c.note_pass(256, 256), c.note_pass(512, 256);
        CHECK(c.whole_scans == 1);
        c.note_pass(768, 232);
        CHECK(c.whole_scans == 2);
        c.note_pass(0, 2000);  // a longer view than any before: the extent grows with it
        CHECK(c.extent == 2000 && c.whole_scans == 3);
    }

    // ---- the trigger: both sides of each constant, and the option ----
    {
        const uint64_t after = rvt::kNarrowAfterWholeScans, floor = rvt::kNarrowFromRows;
        CHECK(after >= 1 && floor >= 1);
        ScanCover big;
        big.extent = floor;
        big.whole_scans = after - 1;
        CHECK(!worth_building(0, big, after, floor));
        big.whole_scans = after;
        CHECK(worth_building(0, big, after, floor));
        CHECK(!worth_building(-1, big, after, floor));
        ScanCover small = big;
        small.extent = floor - 1;
        small.whole_scans = after + 100;
        CHECK(!worth_building(0, small, after, floor));
        CHECK(worth_building(1, small, after, floor));  // option 1: the first whole scan, any size
        small.whole_scans = 0;
        CHECK(!worth_building(1, small, after, floor));
        ScanCover none;
        CHECK(!worth_building(1, none, after, floor) && !worth_building(0, none, after, floor));
    }

    std::printf("ok %ld\n", g_checks);
    return 0;
}
