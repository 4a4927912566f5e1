// Stand-alone CPU test of the code-space lowering of the lean compare term (rivulus_amd/csrc/narrow_term.hpp, what launch_pass hands
// to a pass over narrow codes): for every subset of {<, ==, >}, both code widths, bases at both ends of Int64 and literals on and
// around every edge, truth(code) must equal the plain Int64 comparison of value = base + code with the literal.  Prints "ok <checks>"
// as its last line.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>
#include <vector>

#include "../../rivulus_amd/csrc/narrow_rule.hpp"
#include "../../rivulus_amd/csrc/narrow_term.hpp"

static long g_checks = 0;

static void fail(const char *what, int sel, int64_t base, int64_t lit, uint32_t code) {
    std::printf("FAILED %s: selectors %d base %" PRId64 " literal %" PRId64 " code %" PRIu32 "\n", what, sel, base, lit, code);
    std::exit(1);
}

int main() {
    constexpr int64_t kMin = std::numeric_limits<int64_t>::min(), kMax = std::numeric_limits<int64_t>::max();
    for (const int width : {2, 4}) {
        const uint64_t range = width == 2 ? 0xFFFFull : 0xFFFFFFFFull;  // the largest code of the width
        const int64_t top_base = static_cast<int64_t>(static_cast<uint64_t>(kMax) - range);
        for (const int64_t base : {kMin, int64_t{-5}, int64_t{0}, int64_t{41}, top_base}) {
            const int64_t max = rvn::decode(static_cast<uint32_t>(range), base);  // base + range: fits Int64 for every base above
            if (rvn::value_range(base, max) != range || rvn::code_bytes(range) != width) fail("setup", 0, base, max, 0);
            // literals on and around both ends of the values, in the middle and at the ends of Int64; base - 1 and max + 1 only
            // where Int64 has them (INT64_MIN / INT64_MAX themselves are in the list anyway)
            std::vector<int64_t> lits = {base, base + 1, base + static_cast<int64_t>(range / 2), max - 1, max, kMin, kMax};
            if (base > kMin) lits.push_back(base - 1);
            if (max < kMax) lits.push_back(max + 1);
            for (const int64_t lit : lits) {
                // the codes to try: every 2-byte code; for 4-byte codes the ends, the 2-byte edge and the literal's neighbourhood
                std::vector<uint32_t> codes;
                if (width == 2) {
                    for (uint32_t c = 0; c <= 0xFFFFu; ++c) codes.push_back(c);
                } else {
                    codes = {0u, 1u, 65535u, 65536u, 0xFFFFFFFEu, 0xFFFFFFFFu};
                    if (lit >= base && lit <= max) {
                        const uint32_t L = rvn::encode(lit, base);
                        codes.push_back(L);
                        if (L > 0) codes.push_back(L - 1);
                        if (L < 0xFFFFFFFFu) codes.push_back(L + 1);
                    }
                }
                for (int sel = 0; sel < 8; ++sel) {
                    const bool lt = sel & 1, eq = sel & 2, gt = sel & 4;
                    const rvn::CodeTerm t = rvn::lower_term(lt, eq, gt, lit, base);
                    for (const uint32_t code : codes) {
                        const int64_t value = rvn::decode(code, base);
                        const bool want = (lt && value < lit) || (eq && value == lit) || (gt && value > lit);
                        ++g_checks;
                        if (rvn::code_truth(t, code) != want) fail("truth", sel, base, lit, code);
                    }
                }
            }
        }
    }
    // the empty and the full set, and != as the complement of [L, L], in the form the kernel applies
    const rvn::CodeTerm none = rvn::lower_term(false, false, false, 7, 0), all = rvn::lower_term(true, true, true, 7, 0);
    const rvn::CodeTerm ne = rvn::lower_term(true, false, true, 7, 0);
    for (const uint32_t code : {0u, 6u, 7u, 8u, 0xFFFFu, 0xFFFFFFFFu}) {
        g_checks += 3;
        if (rvn::code_truth(none, code)) fail("empty set", 0, 0, 7, code);
        if (!rvn::code_truth(all, code)) fail("full set", 7, 0, 7, code);
        if (rvn::code_truth(ne, code) != (code != 7u)) fail("!=", 5, 0, 7, code);
    }
    if (!(ne.lo == 7u && ne.span == 0u && ne.negate)) fail("!= form", 5, 0, 7, 0);
    std::printf("ok %ld\n", g_checks);
    return 0;
}
