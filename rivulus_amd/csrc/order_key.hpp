// The order-preserving map of a cell's 64 bits onto an unsigned integer, written once for the device and the host: plain g++
// compiles this header for the CPU test (tests/cpp/sort_key_tests.cpp), hipcc for the kernels -- the grouped MIN / MAX
// (group_agg_kernel.hpp, agg_order_key) and the sort (sort_kernel.hpp).
//   Int64    the sign bit flipped: the numeric order.
//   Float64  sign bit set: every bit flipped; otherwise the sign bit set.  Over the non-NaN cells that is the total order
//            -inf < ... < -0.0 < +0.0 < ... < +inf, and the map is injective there.  A NaN (either sign, any payload) has no place of its
//            own in it: order_key_is_nan says so and the caller decides -- the sort puts every NaN at ~0, above +inf and equal to every
//            other NaN (sort_key); MIN / MAX move it to the end that wins.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RVORDER_HD __host__ __device__ inline
#else
#define RVORDER_HD inline
#endif

namespace rvorder {

constexpr uint64_t kSignBit = 0x8000000000000000ull;

RVORDER_HD bool order_key_is_nan(uint64_t bits) { return (bits & ~kSignBit) > 0x7FF0000000000000ull; }
// the map itself (a NaN's bits go through like any other: see above)
RVORDER_HD uint64_t order_key(uint64_t bits, bool is_float) {
    if (!is_float) return bits ^ kSignBit;
    return (bits >> 63) ? ~bits : bits | kSignBit;
}
// ... and back
RVORDER_HD uint64_t order_value(uint64_t key, bool is_float) {
    if (!is_float) return key ^ kSignBit;
    return (key >> 63) ? key & ~kSignBit : ~key;
}
// what the sort orders a non-null cell by: ascending keys are ascending cells, every NaN the one largest key
RVORDER_HD uint64_t sort_key(uint64_t bits, bool is_float) {
    if (is_float && order_key_is_nan(bits)) return ~0ull;
    return order_key(bits, is_float);
}

}  // namespace rvorder
