// The frame rule of rv_window_frames (window_frame.hip), written once for the device and the host: plain g++ compiles this header for the
// CPU test (tests/cpp/window_frame_rule_tests.cpp), hipcc for the kernels.
//
// A row stands at the 1-based position `pos` of a partition of `len` rows.  Its frame is the positions
// [max(1, pos - preceding), min(len, pos + following)], an unbounded side being the partition's edge; it is empty when that interval is.
// For a frame of the finite width w = preceding + following + 1 the partition is cut into BLOCKS of w positions anchored at its head (the
// last one cut short by the partition's end); with an unbounded side, and whenever w >= len, the one block is the partition.  Given the
// inclusive aggregate of every position's block up to it (prefix) and from it on (suffix), a non-empty frame [lo, hi] is exactly one of
//   FC_PREFIX  lo starts a block and hi lies in it:                            prefix[hi]
//   FC_SUFFIX  hi ends a block (or the partition) and lo lies in it:           suffix[lo]
//   FC_BOTH    lo and hi lie in adjacent blocks:                               suffix[lo] (+) prefix[hi]
// (van Herk / Gil-Werman).  An unclipped frame is w positions wide, so it never spans more than two blocks; one clipped by the partition's
// head starts at position 1, a block start, and one clipped by its end stops at len, which ends the last block.
//
// Offsets are clamped to +-2^33 before anything is added: positions are below 2^32, so an offset of a larger magnitude reaches the same
// rows, and no sum or difference here leaves the Int64 range for any offset the C ABI takes (magnitude <= 2^62).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RVFRAME_HD __host__ __device__ inline
#else
#define RVFRAME_HD inline
#endif

namespace rvframe {

constexpr int64_t kUnbounded = INT64_MAX;           // RV_FRAME_UNBOUNDED
constexpr int64_t kOffsetMost = int64_t{1} << 62;   // the largest magnitude of a finite offset
constexpr int64_t kOffsetClamp = int64_t{1} << 33;

enum : uint32_t { FC_EMPTY = 0, FC_PREFIX = 1, FC_SUFFIX = 2, FC_BOTH = 3 };

// what the C ABI takes: finite offsets of magnitude <= 2^62, and preceding + following >= 0 when both are finite
RVFRAME_HD bool frame_ok(int64_t preceding, int64_t following) {
    const bool pu = preceding == kUnbounded, fu = following == kUnbounded;
    if (!pu && (preceding < -kOffsetMost || preceding > kOffsetMost)) return false;
    if (!fu && (following < -kOffsetMost || following > kOffsetMost)) return false;
    return pu || fu || preceding >= -following;
}

struct Frame {
    int64_t preceding, following;  // clamped; 0 on an unbounded side
    uint64_t width;                // preceding + following + 1 of the clamped offsets; 0 with an unbounded side
    uint32_t preceding_unbounded, following_unbounded;
};

RVFRAME_HD int64_t clamp_offset(int64_t v) { return v < -kOffsetClamp ? -kOffsetClamp : v > kOffsetClamp ? kOffsetClamp : v; }

// of offsets that passed frame_ok
RVFRAME_HD Frame frame_of(int64_t preceding, int64_t following) {
    Frame f{};
    f.preceding_unbounded = preceding == kUnbounded;
    f.following_unbounded = following == kUnbounded;
    f.preceding = f.preceding_unbounded ? 0 : clamp_offset(preceding);
    f.following = f.following_unbounded ? 0 : clamp_offset(following);
    f.width = f.preceding_unbounded || f.following_unbounded ? 0 : static_cast<uint64_t>(f.preceding + f.following + 1);
    return f;
}

struct Pick {
    uint32_t which;   // FC_*
    uint32_t lo, hi;  // 1-based positions in the partition; unspecified when which == FC_EMPTY
};

// 1 <= pos <= len < 2^32
RVFRAME_HD Pick frame_pick(const Frame &f, uint32_t pos, uint32_t len) {
    const int64_t p = pos, n = len;
    const int64_t first = f.preceding_unbounded ? 1 : p - f.preceding, last = f.following_unbounded ? n : p + f.following;
    const int64_t lo = first < 1 ? 1 : first, hi = last > n ? n : last;
    if (lo > hi) return Pick{FC_EMPTY, 0, 0};
    Pick r{FC_BOTH, static_cast<uint32_t>(lo), static_cast<uint32_t>(hi)};
    if (f.preceding_unbounded) r.which = FC_PREFIX;
    else if (f.following_unbounded) r.which = FC_SUFFIX;
    else if (f.width >= len) r.which = lo == 1 ? FC_PREFIX : FC_SUFFIX;  // one block: a frame that starts after the head was cut by the end
    else {
        const uint32_t w = static_cast<uint32_t>(f.width);
        if ((r.lo - 1) / w == (r.hi - 1) / w) r.which = (r.lo - 1) % w == 0 ? FC_PREFIX : FC_SUFFIX;
    }
    return r;
}

// the block heads of a finite width below 2^32: the partition's position pos0 (0-based) starts a block
RVFRAME_HD bool block_head(uint32_t pos0, uint32_t width) { return pos0 % width == 0; }

// NTILE(n): with q = len / n and r = len % n the first r buckets hold q + 1 rows, the rest q; the 1-based bucket of position pos.  n >= 1.
RVFRAME_HD uint64_t ntile_bucket(uint64_t pos, uint64_t len, uint64_t n) {
    const uint64_t q = len / n, r = len % n, big = r * (q + 1);  // big <= len: the rows of the larger buckets
    if (pos <= big) return (pos - 1) / (q + 1) + 1;
    return r + (pos - 1 - big) / q + 1;  // q >= 1 here: q == 0 means r == len and every position is within `big`
}

}  // namespace rvframe
