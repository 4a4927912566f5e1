// The lean compare term of a pass over narrow codes, lowered to CODE SPACE on the host (fused_launch.hip, launch_pass): with
// value = base + code (narrow_rule.hpp, decode), every subset of {<, ==, >} against an Int64 literal is an interval of codes or the
// complement of one, so the kernel needs one 32-bit subtract and one unsigned compare per row instead of a 64-bit addition and two
// 64-bit compares.  Plain C++ without the runtime: tests/cpp/narrow_term_host_tests.cpp builds it on the CPU.
#pragma once
#include <cstdint>

namespace rvn {

// truth(code) = ((code - lo) as uint32 <= span) != negate.  A 2-byte code is zero-extended to 32 bits first, so one form serves both
// code widths: the lowering never needs to know the width (a literal above the largest code of a 2-byte companion is simply an
// interval end no code reaches).
struct CodeTerm {
    uint32_t lo, span;
    bool negate;
};
inline bool code_truth(const CodeTerm &t, uint32_t code) { return (static_cast<uint32_t>(code - t.lo) <= t.span) != t.negate; }

// `sel_lt` / `sel_eq` / `sel_gt`: the term holds where value < / == / > lit (device_common.hpp, DevTerm: `!=` selects lt and gt, `<=`
// lt and eq, ...).  Exact for every literal and base: lit - base does not fit 64 signed bits with bases at the ends of Int64, so the
// literal is first placed below / inside / above the codes by a signed comparison and only then subtracted, unsigned (as
// narrow_rule.hpp's value_range does).
inline CodeTerm lower_term(bool sel_lt, bool sel_eq, bool sel_gt, int64_t lit, int64_t base) {
    const CodeTerm full{0u, 0xFFFFFFFFu, false}, empty{0u, 0xFFFFFFFFu, true};
    if (lit < base) return sel_gt ? full : empty;  // every value lies above the literal
    const uint64_t d = static_cast<uint64_t>(lit) - static_cast<uint64_t>(base);
    if (d > 0xFFFFFFFFull) return sel_lt ? full : empty;  // every value lies below it
    const uint32_t L = static_cast<uint32_t>(d);          // the literal's own code
    // codes below L: [0, L - 1] (none when L == 0); codes above L: the complement of [0, L]
    const int sel = (sel_lt ? 1 : 0) | (sel_eq ? 2 : 0) | (sel_gt ? 4 : 0);
    switch (sel) {
        case 0: return empty;
        case 1: return L == 0 ? empty : CodeTerm{0u, L - 1, false};  // <
        case 2: return CodeTerm{L, 0u, false};                       // ==
        case 3: return CodeTerm{0u, L, false};                       // <=
        case 4: return CodeTerm{0u, L, true};                        // >
        case 5: return CodeTerm{L, 0u, true};                        // !=: the complement of [L, L]
        case 6: return L == 0 ? full : CodeTerm{0u, L - 1, true};    // >=
        default: return full;
    }
}

// The same term without `negate`, wherever one exists: in 32-bit wrap-around arithmetic the complement of the cyclic interval
// [lo, lo + span] is the cyclic interval [lo + span + 1, lo - 1], so the kernel tests one interval and never flips a mask.  The one
// complement that is no interval is the EMPTY set (the complement of all 2^32 codes).  Over 2-byte codes, which reach the compare
// zero-extended, an interval above them stands for it; over 4-byte codes nothing does: `*ok` comes back false, the term unchanged,
// `negate` still set, and the launch hands it on as it is (fused_launch.hip, launch_pass): the kernel tests the flag once per tile
// and runs such a launch through the form of its loop that still flips the masks (fused_kernel.hpp).
// A pass over PACKED codes (10 bits each, narrow_rule.hpp) calls this with code_bytes == 2, like the 2-byte cells it stages: its
// codes reach the compare zero-extended from 10 bits, so the interval {0x10000, 0} lies above every one of them as well, and every
// other folded interval is exact over 0..1023 because it is exact over 0..65535.
inline CodeTerm fold_negate(const CodeTerm &t, int code_bytes, bool *ok) {
    *ok = true;
    if (!t.negate) return t;
    if (t.span != 0xFFFFFFFFu) return CodeTerm{t.lo + t.span + 1u, 0xFFFFFFFEu - t.span, false};
    if (code_bytes == 2) return CodeTerm{0x10000u, 0u, false};
    *ok = false;
    return t;
}

}  // namespace rvn
