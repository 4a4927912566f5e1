// Which ends of a pass over narrow codes' ONE interval (narrow_term.hpp: truth(code) = (code - lo) as uint32 <= span, a complement
// already folded in) a code of the companion can fall outside of.  The companion's codes are 0 .. range (narrow_rule.hpp, value_range:
// max - min of the column), so a single compare against a literal -- `<`, `<=`, `>`, `>=` -- is one-sided in code space: [0, k] or
// [k, range and beyond].  For those the subtraction in front of the compare tests nothing a code can fail:
//   lower only   lo + span >= range: no code lies above the interval        truth(code) = code >= lo
//   upper only   lo == 0:            no code lies below it                  truth(code) = code <= span
//   both         everything else: `==`, `!=` (a wrapped interval) and literals strictly inside on both ends
// A wrapped interval (lo + span passes 2^32: the fold of a complement whose own interval does not start at 0) is always "both": its
// two ends are the two ends of a gap, not of the codes.  The full set {0, 2^32 - 1} is "lower only" with lo = 0; the interval above
// every 2-byte code that stands for the empty set, {0x10000, 0}, is "lower only" with a bound no code reaches.
// The class holds for the codes 0 .. range only -- real rows.  Padding and bytes past a packed companion read as code 0, which lies in
// that range, so it is classified like a row's code and the kernel's rule for it (whole tiles hold no padding) is untouched.
// Plain C++ without the runtime: tests/cpp/narrow_sides_host_tests.cpp builds it on the CPU.
#pragma once
#include <cstdint>

namespace rvn {

enum CodeSides : uint32_t { kSidesBoth = 0, kSidesLowerOnly = 1, kSidesUpperOnly = 2 };

// (lo, span): a folded term, `negate` clear.  range: the companion's largest code.
inline CodeSides classify_sides(uint32_t lo, uint32_t span, uint64_t range) {
    const uint64_t last = static_cast<uint64_t>(lo) + span;  // the interval's last code, before any wrap
    if (last > 0xFFFFFFFFull) return kSidesBoth;             // wrapped
    if (last >= range) return kSidesLowerOnly;
    if (lo == 0) return kSidesUpperOnly;
    return kSidesBoth;
}

// the test a kernel runs for a class, as the CPU test checks it against the interval's own
inline bool sided_truth(CodeSides sides, uint32_t lo, uint32_t span, uint32_t code) {
    switch (sides) {
        case kSidesLowerOnly: return code >= lo;
        case kSidesUpperOnly: return code <= span;
        default: return static_cast<uint32_t>(code - lo) <= span;
    }
}

}  // namespace rvn
