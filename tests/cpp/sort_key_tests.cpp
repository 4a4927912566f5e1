// CPU test of the order map the sort and the grouped MIN / MAX share (rivulus_amd/csrc/order_key.hpp): a stand-alone program, built
// with g++ -fsanitize=address,undefined by tests/test_sort_cpu.py and run as a program.
//
// Over Int64 and Float64 edge values and 10^5 random bit patterns, every pair (a random pattern against each edge value and against its
// neighbour in the list):
//   - the map is monotone with respect to the stated order: a < b in the numeric order (Int64) / in -inf < .. < -0.0 < +0.0 < .. < +inf
//     (Float64, non-NaN) exactly when key(a) < key(b);
//   - it is injective on non-NaN values (different bits, different keys) and order_value undoes it;
//   - all NaNs collapse to the maximum: sort_key is ~0 for every NaN, of either sign and any payload, and above the key of +inf.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rivulus_amd/csrc/order_key.hpp"

static int failures = 0;
static long checks = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        ++checks;                                                         \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static uint64_t next_random(uint64_t &s) {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

static double as_double(uint64_t bits) {
    double d;
    std::memcpy(&d, &bits, 8);
    return d;
}
static uint64_t bits_of(double d) {
    uint64_t b;
    std::memcpy(&b, &d, 8);
    return b;
}

// the stated Float64 order of two non-NaN cells, from the numbers and the sign of zero -- not from the map under test
static int float_order(uint64_t a, uint64_t b) {
    const double x = as_double(a), y = as_double(b);
    if (x < y) return -1;
    if (x > y) return 1;
    const int sx = std::signbit(x) ? 0 : 1, sy = std::signbit(y) ? 0 : 1;  // x == y: only -0.0 against +0.0 differ
    return sx < sy ? -1 : sx > sy ? 1 : 0;
}

static void check_float_pair(uint64_t a, uint64_t b) {
    const bool na = rvorder::order_key_is_nan(a), nb = rvorder::order_key_is_nan(b);
    CHECK(na == std::isnan(as_double(a)));
    const uint64_t ka = rvorder::sort_key(a, true), kb = rvorder::sort_key(b, true);
    if (na) CHECK(ka == ~0ull);
    if (na && nb) CHECK(ka == kb);
    if (na && !nb) CHECK(kb < ka);
    if (na || nb) return;
    const int want = float_order(a, b);
    CHECK((ka < kb) == (want < 0));
    CHECK((ka > kb) == (want > 0));
    CHECK((ka == kb) == (a == b));  // injective
    CHECK(rvorder::order_value(ka, true) == a);
    CHECK(ka < ~0ull);  // below every NaN
}

static void check_int_pair(uint64_t a, uint64_t b) {
    const uint64_t ka = rvorder::sort_key(a, false), kb = rvorder::sort_key(b, false);
    const int64_t x = static_cast<int64_t>(a), y = static_cast<int64_t>(b);
    CHECK((ka < kb) == (x < y));
    CHECK((ka == kb) == (x == y));
    CHECK(rvorder::order_value(ka, false) == a);
}

int main() {
    const double inf = INFINITY;
    std::vector<uint64_t> fedges = {bits_of(-inf), bits_of(-1.7976931348623157e308), bits_of(-1.0), bits_of(-2.2250738585072014e-308), bits_of(-5e-324),
                                    bits_of(-0.0), bits_of(0.0), bits_of(5e-324), bits_of(2.2250738585072014e-308), bits_of(1.0),
                                    bits_of(1.7976931348623157e308), bits_of(inf),
                                    0x7FF8000000000000ull, 0xFFF8000000000000ull, 0x7FF0000000000001ull, 0xFFF0000000000001ull, 0x7FFFFFFFFFFFFFFFull,
                                    0xFFFFFFFFFFFFFFFFull};
    std::vector<uint64_t> iedges = {0x8000000000000000ull, 0x8000000000000001ull, ~0ull, 0, 1, 0x7FFFFFFFFFFFFFFEull, 0x7FFFFFFFFFFFFFFFull};
    for (uint64_t a : fedges)
        for (uint64_t b : fedges) check_float_pair(a, b);
    for (uint64_t a : iedges)
        for (uint64_t b : iedges) check_int_pair(a, b);
    // the edge list is written in ascending order up to +inf: the keys must be strictly ascending too
    for (size_t i = 0; i + 1 < 12; ++i) CHECK(rvorder::sort_key(fedges[i], true) < rvorder::sort_key(fedges[i + 1], true));
    for (size_t i = 0; i + 1 < iedges.size(); ++i) CHECK(rvorder::sort_key(iedges[i], false) < rvorder::sort_key(iedges[i + 1], false));

    uint64_t seed = 0x9E3779B97F4A7C15ull, prev = 0;
    for (int i = 0; i < 100000; ++i) {
        uint64_t r = next_random(seed);
        if (i % 4 == 1) r = (r & 0x800FFFFFFFFFFFFFull) | 0x7FF0000000000000ull;  // NaNs and infinities: the random exponents rarely hit them
        if (i % 4 == 2) r &= 0x800FFFFFFFFFFFFFull;                              // denormals and zeros
        for (uint64_t e : fedges) check_float_pair(r, e);
        for (uint64_t e : iedges) check_int_pair(r, e);
        check_float_pair(r, prev);
        check_int_pair(r, prev);
        check_float_pair(r, r ^ 1);  // a neighbouring bit pattern
        prev = r;
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok %ld checks\n", checks);
    return 0;
}
