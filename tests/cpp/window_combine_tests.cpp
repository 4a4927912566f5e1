// CPU test of csrc/window_combine.hpp, the combine of the window operator's segmented scan: a stand-alone program, built by plain g++
// under -fsanitize=address,undefined and run directly (tests/test_window_cpu.py).
//   * (a (+) b) (+) c == a (+) (b (+) c) on random triples for every operator (Float64 over integer-valued cells, where every partial sum
//     is exact; in general a Float64 addition is not associative and the kernels fix the bracketing instead);
//   * the identity is neutral on both sides;
//   * a tree reduction of a random sequence in ANY bracketing -- and the scan that goes with it: every prefix -- equals the sequential loop
//     "reset at a head, else accumulate", for Int64 and for Float64 on integer-valued data.
// Prints "ok <checks>" and exits 0, or the first failure and exits 1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../rivulus_amd/csrc/window_combine.hpp"

using namespace rvwin;

namespace {

unsigned long long checks = 0;
std::mt19937_64 rng(12);

[[noreturn]] void fail(const char *what, unsigned op) {
    std::printf("FAIL %s (operator %u)\n", what, op);
    std::exit(1);
}

bool same(const Triple &a, const Triple &b) { return a.value == b.value && a.count == b.count && a.flag == b.flag; }

// a random element: Float64 cells are integers below 2^20 in magnitude, never -0.0 (the kernels let a zero in as +0.0)
template <uint32_t OP>
Triple random_triple(int head_one_in) {
    Triple t{};
    t.flag = rng() % static_cast<unsigned>(head_one_in) == 0;
    t.count = rng() % 3;
    if (OP == WC_ADD_F64) {
        const long long k = static_cast<long long>(rng() % (1u << 21)) - (1 << 20);
        t.value = double_to_bits(k == 0 ? 0.0 : static_cast<double>(k));
    } else {
        t.value = rng() % 5 == 0 ? rng() % 7 : rng();  // small values too, so that MIN / MAX meet ties
    }
    return t;
}

// the fold of v[b, e) in a random bracketing
template <uint32_t OP>
Triple tree(const std::vector<Triple> &v, size_t b, size_t e) {
    if (e - b == 1) return v[b];
    const size_t m = b + 1 + rng() % (e - b - 1);
    const Triple left = tree<OP>(v, b, m), right = tree<OP>(v, m, e);
    return combine<OP>(left, right);
}

template <uint32_t OP>
void run() {
    const Triple id = identity_triple<OP>();
    for (int round = 0; round < 4000; ++round) {
        const Triple a = random_triple<OP>(3), b = random_triple<OP>(3), c = random_triple<OP>(3);
        if (!same(combine<OP>(combine<OP>(a, b), c), combine<OP>(a, combine<OP>(b, c)))) fail("associativity", OP);
        if (!same(combine<OP>(id, a), a) || !same(combine<OP>(a, id), a)) fail("identity", OP);
        checks += 3;
    }
    for (int round = 0; round < 300; ++round) {
        const size_t n = 1 + rng() % 200;
        std::vector<Triple> v(n);
        for (Triple &t : v) t = random_triple<OP>(1 + static_cast<int>(rng() % 40));
        // the sequential loop: what the operator means
        Triple acc = id;
        for (size_t i = 0; i < n; ++i) {
            if (v[i].flag) acc = v[i];
            else {
                acc.value = apply<OP>(acc.value, v[i].value);
                acc.count += v[i].count;
            }
            const Triple got = tree<OP>(v, 0, i + 1);
            if (got.value != acc.value || got.count != acc.count) fail("a bracketing of a prefix differs from the sequential loop", OP);
            ++checks;
        }
    }
}

}  // namespace

int main() {
    run<WC_ADD_I64>();
    run<WC_ADD_F64>();
    run<WC_MIN_U64>();
    run<WC_MAX_U64>();
    std::printf("ok %llu\n", checks);
    return 0;
}
