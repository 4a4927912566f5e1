// The string hash and the byte comparison of the device string dictionary (string_dict_kernel.hpp), written once for the
// device and the host: plain g++ compiles this header for the CPU test (tests/cpp/string_hash_tests.cpp), hipcc for the kernels.
//
// A cell's bytes start at any address.  They are fetched as ALIGNED 8-byte words and funnel-shifted into the cell's own 8-byte
// groups (StrWords): one load per 8 bytes instead of eight byte loads, and never a word that holds no byte of the cell -- the
// first word starts at most 7 bytes before the cell, the last ends at most 7 bytes behind it.  What this asks of the buffer:
// its base is 8-byte aligned and its allocation a whole number of 8-byte words (every String values buffer of the library is
// a pool block: 256-byte multiples).  Bytes outside the cell are shifted or masked away before anything looks at them.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RVSTR_HD __host__ __device__ inline
#else
#define RVSTR_HD inline
#endif

namespace rvstr {

// the 8-byte groups of the bytes [p, p + len), little-endian, the last one zero-filled behind the cell
struct StrWords {
    const uint64_t *next_word;  // the aligned word behind `cur`
    const uint64_t *last_word;  // the aligned word that holds the cell's last byte
    uint64_t cur;               // the aligned word the next group starts in
    uint64_t left;              // bytes not handed out yet
    unsigned shift;             // bits the cell starts into its first aligned word: 0, 8, .. 56

    RVSTR_HD StrWords(const uint8_t *p, uint64_t len) : next_word(nullptr), last_word(nullptr), cur(0), left(len), shift(0) {
        if (len == 0) return;  // nothing is read, whatever p is
        const uintptr_t at = reinterpret_cast<uintptr_t>(p);
        shift = static_cast<unsigned>(at & 7) * 8;
        const uint64_t *first = reinterpret_cast<const uint64_t *>(at & ~static_cast<uintptr_t>(7));
        last_word = reinterpret_cast<const uint64_t *>((at + len - 1) & ~static_cast<uintptr_t>(7));
        cur = *first;
        next_word = first + 1;
    }
    RVSTR_HD bool done() const { return left == 0; }
    // the next 8 bytes (fewer at the end: the rest of the group is zero); call only while !done()
    RVSTR_HD uint64_t next() {
        const uint64_t following = next_word <= last_word ? *next_word : 0;
        uint64_t w = shift ? (cur >> shift) | (following << (64 - shift)) : cur;
        cur = following;
        ++next_word;
        if (left < 8) {
            w &= (uint64_t{1} << (8 * left)) - 1;
            left = 0;
        } else {
            left -= 8;
        }
        return w;
    }
};

// murmur3's 64-bit finaliser (the join's join_hash): every bit reaches the low bits the slot index is taken from
RVSTR_HD uint64_t fmix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// 64-bit hash of the bytes [p, p + len): murmur2-64A's word step over the 8-byte groups, the length mixed into the seed (the
// zero fill of the last group alone would hash "a" and "a\0" alike), then the finaliser.  The same value from every alignment.
RVSTR_HD uint64_t string_hash(const uint8_t *p, uint64_t len) {
    const uint64_t m = 0xc6a4a7935bd1e995ull;
    uint64_t h = 0x9e3779b97f4a7c15ull ^ (len * m);
    for (StrWords w(p, len); !w.done();) {
        uint64_t k = w.next();
        k *= m;
        k ^= k >> 47;
        k *= m;
        h ^= k;
        h *= m;
    }
    return fmix64(h);
}

// byte equality of [a, a + la) and [b, b + lb): AnyValue::String's PartialEq -- no normalisation, NUL bytes count
RVSTR_HD bool string_equal(const uint8_t *a, uint64_t la, const uint8_t *b, uint64_t lb) {
    if (la != lb) return false;
    StrWords x(a, la), y(b, lb);
    while (!x.done())
        if (x.next() != y.next()) return false;
    return true;
}

}  // namespace rvstr
