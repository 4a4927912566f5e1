// The combine of the window operator's segmented scan (window_kernel.hpp), written once for the device and the host: plain g++
// compiles this header for the CPU test (tests/cpp/window_combine_tests.cpp), hipcc for the kernels.
//
// An element of the scan is a triple (flag, value, count) over a run of sorted positions:
//   flag   the run holds a partition head;
//   value  the operator applied to the cells of the run FROM ITS LAST PARTITION HEAD ON (the whole run when it has none);
//   count  the non-null cells (or whatever else rides along) of the same stretch.
// a (+) b for a run a directly before a run b: b alone when b holds a head -- nothing before a head reaches past it -- and otherwise
// (a.flag, op(a.value, b.value), a.count + b.count).  That is associative for every associative op (the test brackets random triples
// every way), NOT commutative, and has the identity (0, identity(op), 0) on both sides.
//   WC_ADD_I64  two's complement wrap          WC_ADD_F64  one IEEE-754 addition of the two bit patterns (not associative in general:
//   WC_MIN_U64 / WC_MAX_U64  unsigned          the scan fixes the bracketing, window_kernel.hpp states it)
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RVWIN_HD __host__ __device__ inline
#else
#define RVWIN_HD inline
#endif

namespace rvwin {

enum : uint32_t { WC_ADD_I64 = 0, WC_ADD_F64 = 1, WC_MIN_U64 = 2, WC_MAX_U64 = 3 };

struct Triple {
    uint64_t value;
    uint64_t count;
    uint32_t flag;
    uint32_t pad;
};

RVWIN_HD double bits_to_double(uint64_t b) {
    double d;
    __builtin_memcpy(&d, &b, 8);
    return d;
}
RVWIN_HD uint64_t double_to_bits(double d) {
    uint64_t b;
    __builtin_memcpy(&b, &d, 8);
    return b;
}

template <uint32_t OP>
RVWIN_HD uint64_t identity() {
    return OP == WC_MIN_U64 ? ~0ull : 0ull;  // 0 is also the bit pattern of +0.0
}
template <uint32_t OP>
RVWIN_HD uint64_t apply(uint64_t a, uint64_t b) {
    if (OP == WC_ADD_F64) return double_to_bits(bits_to_double(a) + bits_to_double(b));
    if (OP == WC_MIN_U64) return a < b ? a : b;
    if (OP == WC_MAX_U64) return a > b ? a : b;
    return a + b;
}
template <uint32_t OP>
RVWIN_HD Triple identity_triple() {
    return Triple{identity<OP>(), 0, 0, 0};
}
// a directly before b
template <uint32_t OP>
RVWIN_HD Triple combine(const Triple &a, const Triple &b) {
    if (b.flag) return b;
    return Triple{apply<OP>(a.value, b.value), a.count + b.count, a.flag, 0};
}

}  // namespace rvwin
