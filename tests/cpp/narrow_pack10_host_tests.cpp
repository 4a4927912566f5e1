// Stand-alone CPU test of the packed layout of the narrow companions (rivulus_amd/csrc/narrow_rule.hpp: 10-bit codes, six per 8-byte
// word, super-groups of 384 elements) and of the rule that decides which layout is built and which launch reads which: the index
// arithmetic against a brute-force pack written from the layout's definition, the padding, the spare bits, the companion size, both
// sides of the width and alignment edges, the build / use decisions with the second cover, and the folded compare terms
// (narrow_term.hpp) over every 10-bit code.  Prints "ok <checks>" as its last line.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "../../rivulus_amd/csrc/narrow_rule.hpp"
#include "../../rivulus_amd/csrc/narrow_term.hpp"
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

// The layout as the design states it, written without narrow_rule.hpp's functions: super-group g is 64 words; word l holds elements
// 384 g + 128 s + 2 l + h; field k = 2 s + h lies in the low dword for k < 3, in the high dword otherwise, at bit 10 (k mod 3).
static std::vector<uint64_t> brute_pack(const std::vector<uint32_t> &codes) {
    const uint64_t n = codes.size(), groups = (n + 383) / 384;
    std::vector<uint64_t> words(groups * 64, 0);
    for (uint64_t g = 0; g < groups; ++g)
        for (uint64_t l = 0; l < 64; ++l) {
            uint32_t dw[2] = {0, 0};
            for (uint32_t s = 0; s < 3; ++s)
                for (uint32_t h = 0; h < 2; ++h) {
                    const uint64_t e = 384 * g + 128 * s + 2 * l + h;
                    const uint32_t k = 2 * s + h, code = e < n ? codes[e] : 0u;
                    dw[k >= 3] |= code << (10 * (k >= 3 ? k - 3 : k));
                }
            words[g * 64 + l] = static_cast<uint64_t>(dw[0]) | (static_cast<uint64_t>(dw[1]) << 32);
        }
    return words;
}

int main() {
    using namespace rvn;

    // ---- the layout: element -> (word, dword, shift), against the brute-force pack ----
    for (uint64_t n : {uint64_t{0}, uint64_t{1}, uint64_t{2}, uint64_t{127}, uint64_t{128}, uint64_t{129}, uint64_t{383}, uint64_t{384}, uint64_t{385}, uint64_t{767},
                       uint64_t{768}, uint64_t{769}, uint64_t{3071}, uint64_t{3072}, uint64_t{3073}}) {
        std::vector<uint32_t> codes(n);
        uint64_t x = 0x9E3779B97F4A7C15ull + n;
        for (uint64_t i = 0; i < n; ++i) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            codes[i] = static_cast<uint32_t>(x % 1024);
        }
        if (n >= 2) codes[0] = 1023, codes[n - 1] = 1023;  // all ten bits at both ends
        // companion size: whole super-groups of 512 bytes
        CHECK(packed_bytes(n) == (n + 383) / 384 * 512);
        CHECK(packed_bytes(n) % 512 == 0 && packed_bytes(n) * 6 >= n * 8);
        std::vector<uint64_t> mine(packed_bytes(n) / 8, 0);
        for (uint64_t i = 0; i < n; ++i) {
            const PackedAt a = packed_at(i);
            CHECK(a.word < mine.size() && a.dword < 2 && (a.shift == 0 || a.shift == 10 || a.shift == 20));
            packed_put(mine.data(), i, codes[i]);
        }
        const std::vector<uint64_t> want = brute_pack(codes);
        CHECK(mine.size() == want.size());
        for (size_t w = 0; w < want.size(); ++w) {
            CHECK(mine[w] == want[w]);
            CHECK((want[w] & 0xC0000000C0000000ull) == 0);  // bits 30 and 31 of both dwords
        }
        for (uint64_t i = 0; i < n; ++i) CHECK(packed_get(want.data(), i) == codes[i]);                   // every element is recovered
        for (uint64_t i = n; i < want.size() * 6; ++i) CHECK(packed_get(want.data(), i) == 0);            // the padding is code 0
        // lane l of a wave that reads word l of a super-group owns rows 2 l, 2 l + 1 of each of its three 128-row groups
        for (uint64_t i = 0; i < n; ++i) {
            const PackedAt a = packed_at(i);
            CHECK(a.word / 64 == i / 384 && a.word % 64 == (i % 128) / 2);
            CHECK(a.dword * 3 + a.shift / 10 == 2 * ((i % 384) / 128) + (i & 1));
        }
    }
    // (no two elements share a field: 384 distinct (word, dword, shift) per super-group -- implied by the round trip above, n = 3072)

    // ---- width and alignment: both sides of each edge ----
    CHECK(packed_width_ok(0) && packed_width_ok(999) && packed_width_ok(1023));
    CHECK(!packed_width_ok(1024) && !packed_width_ok(65535) && !packed_width_ok(~uint64_t{0}));
    CHECK(packed_view_aligned(0) && packed_view_aligned(384) && packed_view_aligned(768) && packed_view_aligned(uint64_t{384} << 20));
    CHECK(!packed_view_aligned(2) && !packed_view_aligned(128) && !packed_view_aligned(383) && !packed_view_aligned(385));
    CHECK(!packed_view_aligned(uint64_t{1} << 28));  // 2^28 is no multiple of 3: a stream's 2^28-row windows do not start on super-groups

    // ---- which layout is built ----
    const LaunchKind whole{0, false}, at384{384, false}, at2{2, false}, at128{128, false}, odd{3, false}, window{0, true}, window384{384, true};
    for (int64_t option : {int64_t{0}, int64_t{2}}) {
        CHECK(layout_to_build(option, 999, whole) == Layout::kPacked);
        CHECK(layout_to_build(option, 1023, whole) == Layout::kPacked);
        CHECK(layout_to_build(option, 1024, whole) == Layout::kPlain);  // 2-byte codes
        CHECK(layout_to_build(option, 1023, at384) == Layout::kPacked);
        CHECK(layout_to_build(option, 1023, at2) == Layout::kPlain);
        CHECK(layout_to_build(option, 1023, at128) == Layout::kPlain);
        CHECK(layout_to_build(option, 1023, window) == Layout::kPlain);  // a stream's windows keep getting 2-byte codes
        CHECK(layout_to_build(option, 1023, window384) == Layout::kPlain);
    }
    CHECK(layout_to_build(1, 999, whole) == Layout::kPlain);  // option 1 never builds the packed layout
    CHECK(layout_to_build(1, 0, at384) == Layout::kPlain);
    {   // options 1 and 2 share the trigger: the first whole scan, whatever the size
        ScanCover c;
        c.note_pass(0, 1000);
        CHECK(worth_building(1, c, rvt::kNarrowAfterWholeScans, rvt::kNarrowFromRows) && worth_building(2, c, rvt::kNarrowAfterWholeScans, rvt::kNarrowFromRows));
        CHECK(!worth_building(0, c, rvt::kNarrowAfterWholeScans, rvt::kNarrowFromRows) && !worth_building(-1, c, rvt::kNarrowAfterWholeScans, rvt::kNarrowFromRows));
    }

    // ---- which launch reads which ----
    bool found = false;
    CHECK(layout_to_read(whole, false, false, &found) == Layout::kPlain && !found);
    CHECK(layout_to_read(whole, false, true, &found) == Layout::kPacked && found);
    CHECK(layout_to_read(at384, false, true, &found) == Layout::kPacked && found);
    layout_to_read(at2, false, true, &found);
    CHECK(!found);
    layout_to_read(at128, false, true, &found);
    CHECK(!found);
    layout_to_read(window, false, true, &found);
    CHECK(!found);
    CHECK(layout_to_read(whole, true, false, &found) == Layout::kPlain && found);
    CHECK(layout_to_read(window, true, false, &found) == Layout::kPlain && found);
    CHECK(layout_to_read(at2, true, false, &found) == Layout::kPlain && found);
    layout_to_read(odd, true, false, &found);
    CHECK(!found);
    layout_to_read(odd, true, true, &found);
    CHECK(!found);
    CHECK(layout_to_read(whole, true, true, &found) == Layout::kPacked && found);  // both: each launch the one it can read
    CHECK(layout_to_read(window, true, true, &found) == Layout::kPlain && found);
    CHECK(layout_to_read(at128, true, true, &found) == Layout::kPlain && found);

    // ---- the second cover: launches that cannot use the companion the buffer has ----
    CHECK(count_pass_in(whole, false, false) == CountIn::kFirst && count_pass_in(window, false, false) == CountIn::kFirst);
    CHECK(count_pass_in(whole, false, true) == CountIn::kNowhere && count_pass_in(at384, false, true) == CountIn::kNowhere);
    CHECK(count_pass_in(window, false, true) == CountIn::kSecond && count_pass_in(at2, false, true) == CountIn::kSecond);
    CHECK(count_pass_in(whole, true, false) == CountIn::kNowhere && count_pass_in(window, true, false) == CountIn::kNowhere);
    CHECK(count_pass_in(odd, true, false) == CountIn::kSecond);
    CHECK(count_pass_in(window, true, true) == CountIn::kNowhere && count_pass_in(odd, true, true) == CountIn::kNowhere);
    bool build = false;
    CHECK(second_layout(0, 999, window, true, &build) == Layout::kPlain && build);    // streamed after whole scans: 2-byte codes beside the packed ones
    CHECK(second_layout(2, 999, at2, true, &build) == Layout::kPlain && build);
    second_layout(0, 999, odd, true, &build);
    CHECK(!build);
    second_layout(0, 999, odd, false, &build);                                        // odd slices of a buffer with 2-byte codes can read neither layout
    CHECK(!build);
    second_layout(1, 999, whole, false, &build);
    CHECK(!build);
    {   // a table scanned whole (packed), then streamed in windows with per-batch counts: the windows complete whole scans of their own
        const uint64_t n = uint64_t{1} << 26, win = uint64_t{1} << 24;
        ScanCover first, second;
        bool have_plain = false, have_packed = false;
        for (int scan = 0; scan < 2; ++scan) {
            CHECK(count_pass_in(whole, have_plain, have_packed) == CountIn::kFirst);
            first.note_pass(0, n);
        }
        CHECK(worth_building(0, first, rvt::kNarrowAfterWholeScans, rvt::kNarrowFromRows));
        CHECK(layout_to_build(0, 999, whole) == Layout::kPacked);
        have_packed = true;
        second.note_extent(first.extent);
        for (uint64_t scan = 0; scan < rvt::kNarrowAfterWholeScans; ++scan) {
            CHECK(!worth_building(0, second, rvt::kNarrowAfterWholeScans, rvt::kNarrowFromRows));
            for (uint64_t at = 0; at < n; at += win) {
                const LaunchKind k{at, true};
                CHECK(count_pass_in(k, have_plain, have_packed) == CountIn::kSecond);
                second.note_pass(at, win);
            }
        }
        CHECK(second.whole_scans == rvt::kNarrowAfterWholeScans && worth_building(0, second, rvt::kNarrowAfterWholeScans, rvt::kNarrowFromRows));
        CHECK(second_layout(0, 999, LaunchKind{n - win, true}, have_packed, &build) == Layout::kPlain && build);
        // whole-column launches in between are counted nowhere: they read the packed codes
        CHECK(count_pass_in(whole, have_plain, have_packed) == CountIn::kNowhere);
    }

    // ---- the folded compare terms over every 10-bit code (a pass over packed codes folds with code_bytes == 2) ----
    {
        bool ok = false;
        const CodeTerm empty = fold_negate(CodeTerm{0u, 0xFFFFFFFFu, true}, 2, &ok);
        CHECK(ok && !empty.negate && empty.lo == 0x10000u && empty.span == 0u);
        const CodeTerm full = fold_negate(CodeTerm{0u, 0xFFFFFFFFu, false}, 2, &ok);
        CHECK(ok && !full.negate);
        for (uint32_t c = 0; c <= 1023; ++c) {
            CHECK(!code_truth(empty, c));  // {0x10000, 0} lies above every 10-bit code as it lies above every 2-byte one
            CHECK(code_truth(full, c));
        }
        // every operator against literals below, at, inside, at the top of and above the codes: the folded interval agrees with the
        // comparison of the values, code for code
        const int64_t base = -17;
        for (int64_t lit : {base - 2, base - 1, base, base + 1, base + 511, base + 1022, base + 1023, base + 1024, base + 70000})
            for (int sel = 0; sel < 8; ++sel) {
                const bool lt = sel & 1, eq = sel & 2, gt = sel & 4;
                const CodeTerm t = fold_negate(lower_term(lt, eq, gt, lit, base), 2, &ok);
                CHECK(ok && !t.negate);
                for (uint32_t c = 0; c <= 1023; ++c) {
                    const int64_t v = decode(c, base);
                    CHECK(code_truth(t, c) == ((lt && v < lit) || (eq && v == lit) || (gt && v > lit)));
                }
            }
    }

    std::printf("ok %ld\n", g_checks);
    return 0;
}
