// The kernels that build a narrow companion of an Int64 values buffer (runtime.hpp, NarrowCodes; narrow.hip): the column's
// minimum and maximum, then codes[i] = uint(value[i] - min) in 2 or 4 bytes, or packed at 10 bits (narrow_pack10_kernel).  All are
// plain streaming passes over the 8-byte values (ordinary vector loads and stores, every index checked against `count`), run once per
// buffer and layout.
#pragma once

#include <type_traits>

#include "device_common.hpp"
#include "narrow_rule.hpp"

namespace rvk {

typedef long long rv_i64x2 __attribute__((ext_vector_type(2)));

// out[0] = min, out[1] = max over values[0, count); the host sets out = {INT64_MAX, INT64_MIN} first
__global__ __launch_bounds__(256) void narrow_minmax_kernel(const long long *values, uint64_t count, long long *out) {
    long long lo = 0x7FFFFFFFFFFFFFFFll, hi = -0x7FFFFFFFFFFFFFFFll - 1;
    const uint64_t npairs = count / 2;  // 16-byte loads (pool blocks are 256-byte aligned)
    const rv_i64x2 *pairs = reinterpret_cast<const rv_i64x2 *>(values);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < npairs; i += stride) {
        const rv_i64x2 t = __builtin_nontemporal_load(&pairs[i]);
        lo = t.x < lo ? t.x : lo, hi = t.x > hi ? t.x : hi;
        lo = t.y < lo ? t.y : lo, hi = t.y > hi ? t.y : hi;
    }
    if ((count & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const long long t = values[count - 1];
        lo = t < lo ? t : lo, hi = t > hi ? t : hi;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const long long l2 = static_cast<long long>(shfl64(static_cast<uint64_t>(lo), lane_id() ^ s));
        const long long h2 = static_cast<long long>(shfl64(static_cast<uint64_t>(hi), lane_id() ^ s));
        lo = l2 < lo ? l2 : lo, hi = h2 > hi ? h2 : hi;
    }
    // one pair of atomics per workgroup (atomics on one address are served one at a time: device_common.hpp, striped_add)
    __shared__ long long s_lo[4], s_hi[4];
    const uint32_t wave = threadIdx.x >> 6;
    if (lane_id() == 0) s_lo[wave] = lo, s_hi[wave] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < (blockDim.x >> 6) && w < 4; ++w) lo = s_lo[w] < lo ? s_lo[w] : lo, hi = s_hi[w] > hi ? s_hi[w] : hi;
        atomicMin(&out[0], lo);
        atomicMax(&out[1], hi);
    }
}

// codes[i] = uint(values[i] - base), i < count; BYTES per code.  A thread packs four consecutive elements per step: two 16-byte
// loads, one 8-byte (2-byte codes) or 16-byte (4-byte codes) store.  The codes buffer holds at least count x BYTES bytes.
template <int BYTES>
__global__ __launch_bounds__(256) void narrow_pack_kernel(const long long *values, uint64_t count, long long base, void *codes) {
    static_assert(BYTES == 2 || BYTES == 4, "code width");
    using Code = std::conditional_t<BYTES == 2, uint16_t, uint32_t>;
    const uint64_t nquads = count / 4;
    const rv_i64x2 *pairs = reinterpret_cast<const rv_i64x2 *>(values);
    const uint64_t ub = static_cast<uint64_t>(base);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const uint64_t me = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (uint64_t q = me; q < nquads; q += stride) {
        const rv_i64x2 a = __builtin_nontemporal_load(&pairs[2 * q]), b = __builtin_nontemporal_load(&pairs[2 * q + 1]);
        const uint32_t c0 = static_cast<uint32_t>(static_cast<uint64_t>(a.x) - ub), c1 = static_cast<uint32_t>(static_cast<uint64_t>(a.y) - ub);
        const uint32_t c2 = static_cast<uint32_t>(static_cast<uint64_t>(b.x) - ub), c3 = static_cast<uint32_t>(static_cast<uint64_t>(b.y) - ub);
        if constexpr (BYTES == 2) {
            static_cast<rv_u32x2 *>(codes)[q] = rv_u32x2{(c0 & 0xFFFFu) | (c1 << 16), (c2 & 0xFFFFu) | (c3 << 16)};
        } else {
            static_cast<rv_u32x4 *>(codes)[q] = rv_u32x4{c0, c1, c2, c3};
        }
    }
    const uint64_t tail = nquads * 4 + me;  // the last count % 4 elements
    if (me < 4 && tail < count) static_cast<Code *>(codes)[tail] = static_cast<Code>(static_cast<uint64_t>(values[tail]) - ub);
}

// The packed layout (narrow_rule.hpp: 10-bit codes, six per 8-byte word, super-groups of 384 elements in 64 words).  One thread per
// output word: word l of super-group g takes elements 384 g + 128 s + 2 l + {0, 1}, s = 0, 1, 2 -- three 16-byte loads, each
// coalesced over the 64 threads of a super-group like a pass's pair loads -- and stores one 8-byte word.  `words` = 64 x the
// super-groups of `count`; an element past `count` packs as code 0 (the tail super-group is padded).  The codes buffer holds at
// least words x 8 bytes.
__global__ __launch_bounds__(256) void narrow_pack10_kernel(const long long *values, uint64_t count, long long base, uint64_t words, rv_u32x2 *codes) {
    const rv_i64x2 *pairs = reinterpret_cast<const rv_i64x2 *>(values);
    const uint64_t ub = static_cast<uint64_t>(base);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; w < words; w += stride) {
        const uint64_t first = (w >> 6) * rvn::kPackGroup + 2 * (w & 63);  // the word's first element
        uint32_t c[6];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const uint64_t e = first + 128u * s;
            long long a = base, b = base;  // (code 0)
            if (e + 1 < count) {
                const rv_i64x2 t = __builtin_nontemporal_load(&pairs[e >> 1]);
                a = t.x, b = t.y;
            } else if (e < count) {
                a = values[e];
            }
            c[2 * s] = static_cast<uint32_t>(static_cast<uint64_t>(a) - ub) & rvn::kPackMask;
            c[2 * s + 1] = static_cast<uint32_t>(static_cast<uint64_t>(b) - ub) & rvn::kPackMask;
        }
        codes[w] = rv_u32x2{c[0] | (c[1] << 10) | (c[2] << 20), c[3] | (c[4] << 10) | (c[5] << 20)};
    }
}

}  // namespace rvk
