// Stand-alone CPU test of the one-sided classifier of a pass over packed codes (rivulus_amd/csrc/narrow_sides.hpp, what launch_pass hands
// the kernel beside the folded interval): for every companion range up to 64, every subset of {<, ==, >}, bases at both ends of Int64
// and every literal from two below the column minimum to two above its maximum (and the ends of Int64), the term is lowered and folded
// as the launch does it, classified, and the class's own test -- `code >= lo`, `code <= span`, or the interval's subtract-and-compare --
// must equal the interval's for EVERY code 0 .. range.  A wrapped interval must come out as "both"; a single `<`, `<=`, `>`, `>=` with
// the literal inside the column's range must come out one-sided (else the classifier could say "both" always and pass).  Prints
// "ok <checks>" as its last line.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>
#include <vector>

#include "../../rivulus_amd/csrc/narrow_rule.hpp"
#include "../../rivulus_amd/csrc/narrow_sides.hpp"
#include "../../rivulus_amd/csrc/narrow_term.hpp"

static long g_checks = 0;

static void fail(const char *what, int sel, uint64_t range, int64_t base, int64_t lit, uint32_t code) {
    std::printf("FAILED %s: selectors %d range %" PRIu64 " base %" PRId64 " literal %" PRId64 " code %" PRIu32 "\n", what, sel, range, base, lit, code);
    std::exit(1);
}

int main() {
    constexpr int64_t kMin = std::numeric_limits<int64_t>::min(), kMax = std::numeric_limits<int64_t>::max();
    long one_sided = 0, both = 0, wrapped = 0;
    for (uint64_t range = 0; range <= 64; ++range) {
        for (const int64_t base : {kMin, int64_t{-5}, int64_t{0}, int64_t{41}, static_cast<int64_t>(static_cast<uint64_t>(kMax) - range)}) {
            const int64_t max = rvn::decode(static_cast<uint32_t>(range), base);
            if (rvn::value_range(base, max) != range) fail("setup", 0, range, base, max, 0);
            std::vector<int64_t> lits = {kMin, kMax};
            for (int64_t d = -2; d <= static_cast<int64_t>(range) + 2; ++d) {
                if (d < 0 && base < kMin - d) continue;                           // Int64 has no such literal
                if (d > 0 && base > kMax - d) continue;
                lits.push_back(base + d);
            }
            for (const int64_t lit : lits) {
                for (int sel = 0; sel < 8; ++sel) {
                    const bool lt = sel & 1, eq = sel & 2, gt = sel & 4;
                    const rvn::CodeTerm raw = rvn::lower_term(lt, eq, gt, lit, base);
                    for (const int width : {2, 4}) {
                        bool ok = false;
                        const rvn::CodeTerm t = rvn::fold_negate(raw, width, &ok);
                        if (!ok) continue;  // (the empty set over 4-byte codes: handed on negated, never classified)
                        if (t.negate) fail("fold left a negate", sel, range, base, lit, 0);
                        const rvn::CodeSides sides = rvn::classify_sides(t.lo, t.span, range);
                        const bool wraps = static_cast<uint64_t>(t.lo) + t.span > 0xFFFFFFFFull;
                        if (wraps) {
                            ++wrapped;
                            if (sides != rvn::kSidesBoth) fail("a wrapped interval is two-sided", sel, range, base, lit, t.lo);
                        }
                        for (uint32_t code = 0; code <= range; ++code) {
                            ++g_checks;
                            const bool want = rvn::code_truth(t, code);
                            if (rvn::sided_truth(sides, t.lo, t.span, code) != want) fail("classified test", sel, range, base, lit, code);
                            // ... and both against the comparison of the values themselves
                            const int64_t value = rvn::decode(code, base);
                            if (want != ((lt && value < lit) || (eq && value == lit) || (gt && value > lit))) fail("truth", sel, range, base, lit, code);
                        }
                        // the four single compares are one-sided wherever the literal lies: [0, k] or [k, range and beyond]
                        if (sel == 1 || sel == 3 || sel == 4 || sel == 6) {
                            if (sides == rvn::kSidesBoth) fail("a single compare is one-sided", sel, range, base, lit, t.lo);
                            ++one_sided;
                        } else if (sides == rvn::kSidesBoth) {
                            ++both;
                        }
                    }
                }
            }
        }
    }
    // the forms by hand: x > 899 over codes 0 .. 999 (the flagship query), its complement, ==, != and the empty set over 2-byte codes
    bool ok = false;
    const rvn::CodeTerm gt = rvn::fold_negate(rvn::lower_term(false, false, true, 899, 0), 2, &ok);
    if (!(gt.lo == 900u && rvn::classify_sides(gt.lo, gt.span, 999) == rvn::kSidesLowerOnly)) fail("x > 899", 4, 999, 0, 899, gt.lo);
    const rvn::CodeTerm le = rvn::fold_negate(rvn::lower_term(true, true, false, 899, 0), 2, &ok);
    if (!(le.lo == 0u && le.span == 899u && rvn::classify_sides(le.lo, le.span, 999) == rvn::kSidesUpperOnly)) fail("x <= 899", 3, 999, 0, 899, le.span);
    const rvn::CodeTerm eq = rvn::fold_negate(rvn::lower_term(false, true, false, 500, 0), 2, &ok);
    if (rvn::classify_sides(eq.lo, eq.span, 999) != rvn::kSidesBoth) fail("x == 500", 2, 999, 0, 500, eq.lo);
    const rvn::CodeTerm ne = rvn::fold_negate(rvn::lower_term(true, false, true, 500, 0), 2, &ok);
    if (rvn::classify_sides(ne.lo, ne.span, 999) != rvn::kSidesBoth) fail("x != 500", 5, 999, 0, 500, ne.lo);
    const rvn::CodeTerm none = rvn::fold_negate(rvn::lower_term(false, false, false, 7, 0), 2, &ok);
    if (!(none.lo == 0x10000u && rvn::classify_sides(none.lo, none.span, 999) == rvn::kSidesLowerOnly)) fail("the empty set", 0, 999, 0, 7, none.lo);
    g_checks += 5;
    if (one_sided == 0 || both == 0 || wrapped == 0) fail("every class and a wrapped interval are among the cases", 0, 0, 0, 0, 0);
    std::printf("classes: %ld one-sided, %ld two-sided, %ld wrapped\nok %ld\n", one_sided, both, wrapped, g_checks);
    return 0;
}
