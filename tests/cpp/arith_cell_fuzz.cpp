// CPU run of the arithmetic cell functions (rivulus_amd/csrc/arith_cell.hpp, the header the device kernel evaluates cells with):
// plain g++ compiles the header, and this program writes what its functions give over edge and random cells for
// tests/test_arith_cpu.py to compare, bit for bit, with tests/arith_model.py.
//   arith_cell_fuzz types              the result-dtype table: one "left right result" line per pair of dtype codes 0 .. 4
//   arith_cell_fuzz cells N out.bin    for each type pair (ii, ff, if, fi) and each operator (+ - * /), in that order: N records of
//                                      four little-endian u64 {a, b, result, ok} -- a / b the raw input cells (Int64 or Float64
//                                      bits as the pair says), result the output bits, ok 0 for a null result.
// The first records of every block are all pairs of the edge cells; the rest come from splitmix64.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../rivulus_amd/csrc/arith_cell.hpp"

namespace {

uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

std::vector<uint64_t> int_edges() {
    const int64_t p53 = int64_t{1} << 53, p54 = int64_t{1} << 54;
    const int64_t mx = std::numeric_limits<int64_t>::max(), mn = std::numeric_limits<int64_t>::min();
    const int64_t v[] = {0, 1, -1, mn, mx, int64_t{1} << 31, -(int64_t{1} << 31), int64_t{1} << 32, -(int64_t{1} << 32), p53 + 1, p53 - 1, -(p53 + 1), -(p53 - 1),
                         // halfway cases of the conversion to Float64: ties go to the even neighbour
                         p53 + 3, p54 + 2, p54 + 6, -(p54 + 2), mx - 511, mx - 512, mn + 512, mn + 1536, 2, -2, 3, 7, -7, 10};
    std::vector<uint64_t> out;
    for (int64_t x : v) out.push_back(static_cast<uint64_t>(x));
    return out;
}

std::vector<uint64_t> float_edges() {
    const double inf = std::numeric_limits<double>::infinity();
    const double v[] = {0.0, -0.0, inf, -inf, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::denorm_min(), -std::numeric_limits<double>::denorm_min(),
                        2.2250738585072009e-308 /* the largest subnormal */, std::numeric_limits<double>::min(), std::numeric_limits<double>::max(), -std::numeric_limits<double>::max(),
                        1.0, -1.0, 1.0 + 0x1p-30, 1.0 - 0x1p-30, 0.5, 2.0, 3.0, 1e-200, 1e-120, 1e200, 9007199254740992.0, 9007199254740993.0 /* rounds on the way in */,
                        0.1, 1.5, -7.0, 0x1p-1022 * 1.5, 0x1p-537};
    std::vector<uint64_t> out;
    for (double x : v) out.push_back(rvarith::f64_bits(x));
    return out;
}

// a random cell: every fourth a small number, every fourth a raw 64-bit pattern (for Float64: NaNs, subnormals, huge exponents), the
// rest mid-sized values whose products and sums round
uint64_t random_cell(bool is_float, uint64_t &s) {
    const uint64_t r = splitmix64(s), kind = r & 3;
    const uint64_t x = splitmix64(s);
    if (!is_float) {
        if (kind == 0) return static_cast<uint64_t>(static_cast<int64_t>(x % 41) - 20);
        if (kind == 1) return x;
        if (kind == 2) return static_cast<uint64_t>(static_cast<int64_t>(x >> 10) - (int64_t{1} << 53));  // round 2^53: conversions round
        return static_cast<uint64_t>(static_cast<int64_t>(x >> 32) - (int64_t{1} << 31));
    }
    if (kind == 0) return rvarith::f64_bits(static_cast<double>(static_cast<int64_t>(x % 41) - 20));
    if (kind == 1) return x;
    if (kind == 2) return (x & 0x800FFFFFFFFFFFFFull) | (uint64_t{(x >> 52) % 64} << 52);  // subnormals and the smallest normals
    return rvarith::f64_bits((static_cast<double>(x >> 11) * 0x1p-53 - 0.5) * 1e6);
}

int run_types() {
    for (int l = 0; l <= 4; ++l)
        for (int r = 0; r <= 4; ++r) std::printf("%d %d %d\n", l, r, rvarith::result_dtype(l, r));
    return 0;
}

int run_cells(uint64_t n, const char *path) {
    FILE *f = std::fopen(path, "wb");
    if (!f) {
        std::perror(path);
        return 2;
    }
    const std::vector<uint64_t> ie = int_edges(), fe = float_edges();
    uint64_t seed = 20240611, written = 0;
    for (int pair = 0; pair < 4; ++pair) {  // ii, ff, if, fi
        const bool af = pair == 1 || pair == 3, bf = pair == 1 || pair == 2;
        const std::vector<uint64_t> &ea = af ? fe : ie, &eb = bf ? fe : ie;
        for (uint32_t op = 0; op < 4; ++op) {
            std::vector<uint64_t> rec;
            rec.reserve(n * 4);
            for (uint64_t k = 0; k < n; ++k) {
                uint64_t a, b;
                if (k < ea.size() * eb.size()) {
                    a = ea[k / eb.size()];
                    b = eb[k % eb.size()];
                } else {
                    a = random_cell(af, seed);
                    b = random_cell(bf, seed);
                }
                uint64_t x = a, y = b;
                const bool flt = af || bf;
                if (flt && !af) x = rvarith::f64_bits(rvarith::i64_to_f64(static_cast<int64_t>(a)));
                if (flt && !bf) y = rvarith::f64_bits(rvarith::i64_to_f64(static_cast<int64_t>(b)));
                bool ok = true;
                const uint64_t r = rvarith::apply((flt ? rvarith::S_ADD_F64 : rvarith::S_ADD_I64) + op, x, y, &ok);
                rec.insert(rec.end(), {a, b, r, static_cast<uint64_t>(ok)});
            }
            if (std::fwrite(rec.data(), 8, rec.size(), f) != rec.size()) return 2;
            written += n;
        }
    }
    std::fclose(f);
    std::printf("ok %llu\n", static_cast<unsigned long long>(written));
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "types") return run_types();
    if (argc == 4 && std::string(argv[1]) == "cells") return run_cells(std::strtoull(argv[2], nullptr, 10), argv[3]);
    std::fprintf(stderr, "usage: arith_cell_fuzz types | cells N out.bin\n");
    return 2;
}
