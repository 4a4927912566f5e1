// CPU test of the string dictionary's shared hash header (rivulus_amd/csrc/string_hash.hpp): a stand-alone program, built
// with g++ -fsanitize=address,undefined by tests/test_string_dict_cpu.py and run as a program.
//
//   - byte strings of length 0-40 and one of 4 KiB hash the same from every start alignment 0-7 inside a padded buffer,
//     and the same as a byte-at-a-time restatement of the hash;
//   - no read past the end: every string is also hashed where it ENDS flush with the end of a heap block and where it STARTS at
//     the block's first byte (the aligned loads may touch the up to 7 bytes around the cell inside its own 8-byte words, never
//     another word: AddressSanitizer faults on the first byte outside the block);
//   - the length is mixed in: "a" != "a\0", "" != "\0";
//   - string_equal is byte equality at every pair of alignments, a difference in the last byte or only in the length included.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rivulus_amd/csrc/string_hash.hpp"

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                              \
        }                                                            \
    } while (0)

// the same hash, bytes assembled one at a time: what StrWords must hand out
static uint64_t hash_by_bytes(const uint8_t *p, uint64_t len) {
    const uint64_t m = 0xc6a4a7935bd1e995ull;
    uint64_t h = 0x9e3779b97f4a7c15ull ^ (len * m);
    for (uint64_t at = 0; at < len; at += 8) {
        uint64_t k = 0;
        for (uint64_t j = 0; j < 8 && at + j < len; ++j) k |= static_cast<uint64_t>(p[at + j]) << (8 * j);
        k *= m;
        k ^= k >> 47;
        k *= m;
        h ^= k;
        h *= m;
    }
    return rvstr::fmix64(h);
}

static uint64_t next_random(uint64_t &s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

// `bytes` copied to offset `at` of a heap block of exactly `block` bytes (operator new[]: aligned to 16 at least)
struct Placed {
    uint8_t *block;
    const uint8_t *p;
    Placed(const std::vector<uint8_t> &bytes, size_t at, size_t block_bytes, uint8_t fill) {
        block = new uint8_t[block_bytes];
        std::memset(block, fill, block_bytes);
        if (!bytes.empty()) std::memcpy(block + at, bytes.data(), bytes.size());
        p = block + at;
    }
    ~Placed() { delete[] block; }
    Placed(const Placed &) = delete;
    Placed &operator=(const Placed &) = delete;
};

static size_t round8(size_t x) { return (x + 7) & ~static_cast<size_t>(7); }

int main() {
    uint64_t seed = 12345;
    std::vector<size_t> lengths;
    for (size_t l = 0; l <= 40; ++l) lengths.push_back(l);
    lengths.push_back(4096);
    uint64_t cases = 0;
    for (size_t len : lengths) {
        std::vector<uint8_t> bytes(len);
        for (auto &b : bytes) b = static_cast<uint8_t>(next_random(seed));
        const uint64_t want = hash_by_bytes(bytes.data(), len);
        {  // the cell ends exactly where the block ends (its start alignment follows from the length: 0-40 cover all eight)
            const size_t block = round8(len) + 8;
            Placed flush(bytes, block - len, block, 0xCD);
            CHECK(rvstr::string_hash(flush.p, len) == want);
            ++cases;
        }
        for (size_t align = 0; align < 8; ++align) {
            // inside a padded buffer, two different paddings: the bytes around the cell must not matter
            for (uint8_t fill : {uint8_t{0x00}, uint8_t{0xFF}}) {
                Placed mid(bytes, 16 + align, round8(16 + align + len) + 16, fill);
                CHECK(rvstr::string_hash(mid.p, len) == want);
                ++cases;
            }
            // the cell's first aligned word is the block's first, and its last aligned word the block's last
            Placed tight(bytes, align, std::max<size_t>(round8(align + len), 8), 0xAB);
            CHECK(rvstr::string_hash(tight.p, len) == want);
            cases += 1;
        }
    }

    // the length is mixed in
    const uint8_t a[8] = {'a', 0, 0, 0, 0, 0, 0, 0};
    CHECK(rvstr::string_hash(a, 1) != rvstr::string_hash(a, 2));
    CHECK(rvstr::string_hash(a + 1, 0) != rvstr::string_hash(a + 1, 1));
    CHECK(rvstr::string_hash(a, 0) == rvstr::string_hash(a + 3, 0));  // "" hashes alike wherever it lies, and reads nothing
    CHECK(rvstr::string_hash(nullptr, 0) == rvstr::string_hash(a, 0));

    // string_equal: byte equality at every pair of alignments
    for (size_t len : {size_t{0}, size_t{1}, size_t{7}, size_t{8}, size_t{9}, size_t{16}, size_t{17}, size_t{33}, size_t{4096}}) {
        std::vector<uint8_t> x(len);
        for (auto &b : x) b = static_cast<uint8_t>(next_random(seed));
        for (size_t ax = 0; ax < 8; ++ax)
            for (size_t ay = 0; ay < 8; ++ay) {
                Placed px(x, ax, std::max<size_t>(round8(ax + len), 8), 0x11), py(x, ay, std::max<size_t>(round8(ay + len), 8), 0x22);
                CHECK(rvstr::string_equal(px.p, len, py.p, len));
                if (len) {
                    std::vector<uint8_t> y = x;
                    y[len - 1] ^= 0x80;  // differs in the last byte only
                    Placed pz(y, ay, std::max<size_t>(round8(ay + len), 8), 0x11);
                    CHECK(!rvstr::string_equal(px.p, len, pz.p, len));
                    CHECK(!rvstr::string_equal(px.p, len, py.p, len - 1));  // differs only in length
                    y = x;
                    y[0] ^= 1;
                    Placed pw(y, ay, std::max<size_t>(round8(ay + len), 8), 0x11);
                    CHECK(!rvstr::string_equal(px.p, len, pw.p, len));
                }
                cases += 1;
            }
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ok %llu\n", static_cast<unsigned long long>(cases));
    return 0;
}
