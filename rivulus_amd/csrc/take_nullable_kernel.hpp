// The gathers over a NULLABLE index list (rv_take_device_nullable, the outer joins' gathers): a null index gives a null cell -- value
// 0 / false / length 0, validity bit clear.  Kernels of their own, in a unit of their own (take_nullable.hip), so that take_kernel,
// take_bounds_kernel and str_gather_lengths -- the gathers of every filter, sort and inner join -- and the units that hold them stay
// the code they were.
#pragma once

#include "aux_kernels.hpp"
#include "string_kernels.hpp"

namespace rvk {

// validity != nullptr: the index list's own bitmap, read at bit `offset` + i; nullptr: an all-ones index is the null (what the join's
// probe leaves in its index buffers, kJoinNone)
struct TakeNulls {
    const uint8_t *validity;
    uint64_t offset;
};
__device__ __forceinline__ bool take_index_is_null(const TakeNulls &z, uint64_t i, uint64_t index) {
    if (!z.validity) return index == ~0ull;
    const uint64_t at = z.offset + i;
    return !((z.validity[at >> 3] >> (at & 7)) & 1);
}

// take_kernel over a nullable index list; out_validity is always there
static __global__ __launch_bounds__(256) void take_nullable_kernel(const TakeParams p, const TakeNulls z) {
    const int lane = lane_id();
    const uint64_t nchunks = (p.n + 63) / 64;
    const uint64_t wave0 = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = (static_cast<uint64_t>(gridDim.x) * blockDim.x) >> 6;
    unsigned long long pop = 0;
    for (uint64_t c = wave0; c < nchunks; c += nwaves) {
        const uint64_t i = c * 64 + lane;
        const bool in = i < p.n;
        const uint64_t index = in ? p.indices[i] : 0;
        const bool live = in && !take_index_is_null(z, i, index);  // the row has a source cell
        const uint64_t src = live ? index + p.col.offset : 0;
        bool valid = live;
        if (live && p.col.validity) valid = (p.col.validity[src >> 3] >> (src & 7)) & 1;
        if (p.col.dtype == DT_BOOLEAN) {
            const uint8_t *vals = static_cast<const uint8_t *>(p.col.values);
            const bool bit = valid && ((vals[src >> 3] >> (src & 7)) & 1);
            const uint64_t m = ballot64(bit);
            if (lane == 0) p.out_values[c] = m;
        } else if (in) {
            p.out_values[i] = valid ? static_cast<const uint64_t *>(p.col.values)[src] : 0;
        }
        const uint64_t m = ballot64(valid);
        if (lane == 0) {
            p.out_validity[c] = m;
            pop += static_cast<unsigned long long>(__popcll(m));
        }
    }
    if (lane == 0 && pop) striped_add(p.out_valid_pop, pop);
}

// take_bounds_kernel over a nullable index list: a null index is in bounds whatever lies under it
static __global__ __launch_bounds__(256) void take_bounds_nullable_kernel(const uint64_t *indices, TakeNulls z, uint64_t n, uint64_t rows, unsigned long long *first_bad) {
    unsigned long long bad = ~0ull;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t index = indices[i];
        if (!take_index_is_null(z, i, index) && index >= rows && i < bad) bad = i;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = (static_cast<unsigned long long>(__shfl_xor(static_cast<uint32_t>(bad >> 32), s, 64)) << 32) |
                                     __shfl_xor(static_cast<uint32_t>(bad), s, 64);
        bad = o < bad ? o : bad;
    }
    if (lane_id() == 0 && bad != ~0ull) atomicMin(first_bad, bad);
}

// str_gather_lengths over a nullable index list: a null index gives length 0 and a clear validity bit; out_validity is always there
static __global__ __launch_bounds__(256) void str_gather_lengths_nullable(const StrGather p, const TakeNulls z) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    bool valid = false;
    uint32_t len = 0;
    if (j < p.n) {
        const uint64_t idx = p.indices[j];
        if (take_index_is_null(z, j, idx)) {
            p.starts[j] = 0;
        } else if (idx >= p.src_length) {
            atomicExch(p.err, 1u);
        } else {
            const uint64_t e = p.offset + idx;
            valid = !p.validity || ((p.validity[e >> 3] >> (e & 7)) & 1);
            const int32_t b0 = p.offsets[e];
            if (valid) len = static_cast<uint32_t>(p.offsets[e + 1] - b0);
            p.starts[j] = b0;
        }
        p.lengths[j] = len;
    }
    __shared__ uint32_t s_valid[4];
    const uint64_t word = ballot64(valid);  // 64 consecutive j per wave (blockDim is a multiple of 64)
    if ((threadIdx.x & 63) == 0) {
        if (j < p.n) p.out_validity[j >> 6] = word;
        s_valid[threadIdx.x >> 6] = static_cast<uint32_t>(__popcll(word));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = static_cast<unsigned long long>(s_valid[0]) + s_valid[1] + s_valid[2] + s_valid[3];
        if (t) striped_add_wg(p.valid_pop, t);
    }
}

}  // namespace rvk
