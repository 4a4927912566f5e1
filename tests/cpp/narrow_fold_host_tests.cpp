// Stand-alone CPU test of rvn::fold_negate (rivulus_amd/csrc/narrow_term.hpp): the term a pass over narrow codes is launched with is ONE
// interval of codes, so the kernel never flips a mask.  For every selector subset, bases at both ends of Int64, literals whose own code
// is on an edge of either code width, literals below the base and above the range -- and for raw terms on every edge of the 32-bit
// wrap-around -- the folded term must hold exactly where the unfolded one does: over EVERY 2-byte code, and over the 4-byte codes within
// +-2 of both ends of either interval, of 0 and of 2^32 - 1.  The only term without such a form is the empty set over 4-byte codes.
// Prints "ok <checks>" as its last line.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>
#include <vector>

#include "../../rivulus_amd/csrc/narrow_term.hpp"

static long g_checks = 0, g_unfoldable = 0;

static void fail(const char *what, const rvn::CodeTerm &t, int width, uint32_t code) {
    std::printf("FAILED %s: lo %" PRIu32 " span %" PRIu32 " negate %d, %d-byte codes, code %" PRIu32 "\n", what, t.lo, t.span, t.negate ? 1 : 0, width, code);
    std::exit(1);
}

static bool is_empty_set(const rvn::CodeTerm &t) { return t.negate && t.span == 0xFFFFFFFFu; }

// the folded form of `t` over codes of `width` bytes against `t` itself
static void check_term(const rvn::CodeTerm &t, int width) {
    bool ok = false;
    const rvn::CodeTerm f = rvn::fold_negate(t, width, &ok);
    ++g_checks;
    if (ok != !(width == 4 && is_empty_set(t))) fail("which terms fold", t, width, 0);
    if (!ok) {  // handed back as it came: the caller reads the 8-byte values
        ++g_unfoldable;
        if (f.lo != t.lo || f.span != t.span || f.negate != t.negate) fail("an unfoldable term changed", t, width, 0);
        return;
    }
    if (f.negate) fail("still negated", t, width, 0);
    if (!t.negate && (f.lo != t.lo || f.span != t.span)) fail("a plain interval changed", t, width, 0);
    if (width == 2) {
        for (uint32_t c = 0; c <= 0xFFFFu; ++c) {
            ++g_checks;
            if (rvn::code_truth(f, c) != rvn::code_truth(t, c)) fail("truth", t, width, c);
        }
        return;
    }
    for (const uint32_t at : {t.lo, t.lo + t.span, f.lo, f.lo + f.span, 0u, 0xFFFFFFFFu})
        for (int d = -2; d <= 2; ++d) {
            const uint32_t c = at + static_cast<uint32_t>(d);  // wraps, like the codes' own arithmetic
            ++g_checks;
            if (rvn::code_truth(f, c) != rvn::code_truth(t, c)) fail("truth", t, width, c);
        }
}

int main() {
    constexpr int64_t kMin = std::numeric_limits<int64_t>::min(), kMax = std::numeric_limits<int64_t>::max();
    const std::vector<uint32_t> edges = {0u, 1u, 0xFFFEu, 0xFFFFu, 0x10000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    // ---- terms as lower_term makes them ----------------------------------------------------------------------------------
    const std::vector<int64_t> bases = {kMin, kMin + 1, -5, 0, 41, kMax - int64_t{0xFFFFFFFF}, kMax - 0xFFFF, kMax};
    for (const int64_t base : bases) {
        std::vector<int64_t> lits = {kMin, kMax};
        for (const uint32_t L : edges)  // the literal whose own code is L, where Int64 has it
            if (static_cast<uint64_t>(kMax) - static_cast<uint64_t>(base) >= L) lits.push_back(static_cast<int64_t>(static_cast<uint64_t>(base) + L));
        if (base > kMin) lits.push_back(base - 1);                                                               // below the base
        if (base > kMin + 1) lits.push_back(base - 2);
        if (static_cast<uint64_t>(kMax) - static_cast<uint64_t>(base) >= 0x100000001ull)                       // above every code
            lits.push_back(static_cast<int64_t>(static_cast<uint64_t>(base) + 0x100000000ull)), lits.push_back(static_cast<int64_t>(static_cast<uint64_t>(base) + 0x100000001ull));
        for (const int64_t lit : lits)
            for (int sel = 0; sel < 8; ++sel) {
                const rvn::CodeTerm t = rvn::lower_term(sel & 1, sel & 2, sel & 4, lit, base);
                check_term(t, 2);
                check_term(t, 4);
            }
    }
    // ---- every interval and complement on the edges of the wrap-around, whoever made it ------------------------------------------
    for (const uint32_t lo : edges)
        for (const uint32_t span : edges)
            for (const bool negate : {false, true}) {
                check_term(rvn::CodeTerm{lo, span, negate}, 2);
                check_term(rvn::CodeTerm{lo, span, negate}, 4);
            }
    // ---- the forms the launch relies on ---------------------------------------------------------------------------------------------
    bool ok = false;
    const rvn::CodeTerm none2 = rvn::fold_negate(rvn::lower_term(false, false, false, 7, 0), 2, &ok);
    if (!ok || none2.lo != 0x10000u || none2.span != 0u || none2.negate) fail("the empty set over 2-byte codes", none2, 2, 0);
    const rvn::CodeTerm all = rvn::fold_negate(rvn::lower_term(true, true, true, 7, 0), 4, &ok);
    if (!ok || all.lo != 0u || all.span != 0xFFFFFFFFu || all.negate) fail("the full set", all, 4, 0);
    const rvn::CodeTerm gt = rvn::fold_negate(rvn::lower_term(false, false, true, 899, 0), 2, &ok);  // x > 899: codes [900, 2^32 - 1]
    if (!ok || gt.lo != 900u || gt.span != 0xFFFFFFFFu - 900u || gt.negate) fail("x > 899", gt, 2, 0);
    const rvn::CodeTerm ne = rvn::fold_negate(rvn::lower_term(true, false, true, 7, 0), 4, &ok);  // x != 7: [8, 6] around the wrap
    if (!ok || ne.lo != 8u || ne.span != 0xFFFFFFFEu || ne.negate) fail("x != 7", ne, 4, 0);
    rvn::fold_negate(rvn::lower_term(false, false, false, 7, 0), 4, &ok);
    if (ok) fail("the empty set over 4-byte codes has no interval", none2, 4, 0);
    if (g_unfoldable == 0) fail("no unfoldable term was met", none2, 4, 0);
    std::printf("ok %ld\n", g_checks);
    return 0;
}
