// The per-tile arithmetic of the staged pass (fused_kernel.hpp), written once for the device and the host: plain g++ compiles this
// header for the CPU test (tests/cpp/tile_addr_tests.cpp, which holds it to the per-tile expressions it replaced), hipcc for the kernel
// and for the launch (fused_launch.hip, which fills a TileWalk per launch).
//
// A launch of n rows runs tiles of `tile_rows` = waves x 64 x rows-per-lane rows; wave w of tile t owns rows [t tile_rows + w wave_rows,
// + wave_rows).  What the tile loop asked per tile with 64-bit multiplies, a division by 384 and 64-bit compares is linear in t and w:
//   whole tile?         t tile_rows + tile_rows <= n          ==  t < first_ragged_tile      (one 32-bit compare)
//   rows of the wave    clamp(n - (t tile_rows + w wave_rows)) ==  clamp(ragged_rows - w wave_rows) in the one ragged tile
//   byte of its codes   (offset + row) / 384 * 512, or (offset + row) * 2 | 4
//                                                              ==  view_byte0 + t tile_bytes + w wave_bytes
// because the view starts on a super-group (packed codes; narrow_rule.hpp, packed_view_aligned) and a tile and a wave range of the
// packed geometries are whole super-groups (rows per lane a multiple of 6); 2- and 4-byte codes are linear as they stand.
// The passes over packed codes are the ones that ask it today (fused_kernel.hpp, kLeanTile: the other forms measured no gain or a loss
// with the cut and keep their per-tile expressions); the 2- and 4-byte widths are here, and tested, for the day they do.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RVTILE_HD __host__ __device__ inline
#else
#define RVTILE_HD inline
#endif

namespace rvtile {

constexpr uint64_t kPackGroup = 384, kPackGroupBytes = 512;  // the packed layout's super-group (narrow_rule.hpp)
constexpr int kPackedCodes = 0;                              // `code_bytes` of a packed companion; 2 and 4: plain codes

// code bytes of `rows` consecutive elements from an element that starts a super-group (packed) or a pair
RVTILE_HD uint64_t code_bytes_of(uint64_t rows, int code_bytes) {
    return code_bytes == kPackedCodes ? rows / kPackGroup * kPackGroupBytes : rows * static_cast<uint64_t>(code_bytes);
}

// The launch's constants.  The code fields are zero in a launch that reads the 8-byte values.
struct TileWalk {
    uint64_t view_byte0;         // byte of the companion that holds the view's first code
    uint64_t bytes;              // readable bytes of the companion
    uint32_t tile_bytes;         // code bytes of a tile
    uint32_t wave_bytes;         // ... of a wave range
    uint32_t first_ragged_tile;  // tiles below it are whole: n / tile_rows
    uint32_t ragged_rows;        // rows of that tile inside the launch: n % tile_rows (0: every tile is whole)
};

// `n` rows in tiles of `waves` wave ranges of 64 x `rows_per_lane` rows; n / tile_rows must fit 32 bits (the launch checks its tile count)
RVTILE_HD TileWalk rows_walk(uint64_t n, int rows_per_lane, int waves) {
    const uint64_t tile_rows = 64ull * static_cast<uint64_t>(rows_per_lane) * static_cast<uint64_t>(waves);
    TileWalk w{};
    w.first_ragged_tile = static_cast<uint32_t>(n / tile_rows);
    w.ragged_rows = static_cast<uint32_t>(n % tile_rows);
    return w;
}
// ... reading codes of `code_bytes` (kPackedCodes, 2, 4) from a companion of `bytes` readable bytes, the view starting at element `offset`
// of the values buffer (a multiple of 384 for packed codes, even otherwise)
RVTILE_HD TileWalk codes_walk(uint64_t n, int rows_per_lane, int waves, uint64_t offset, uint64_t bytes, int code_bytes) {
    TileWalk w = rows_walk(n, rows_per_lane, waves);
    const uint64_t wave_rows = 64ull * static_cast<uint64_t>(rows_per_lane);
    w.view_byte0 = code_bytes_of(offset, code_bytes);
    w.bytes = bytes;
    w.wave_bytes = static_cast<uint32_t>(code_bytes_of(wave_rows, code_bytes));
    w.tile_bytes = w.wave_bytes * static_cast<uint32_t>(waves);
    return w;
}

// every row of tile `tile` lies inside the launch
RVTILE_HD bool tile_full(const TileWalk &w, uint32_t tile) { return tile < w.first_ragged_tile; }

// rows of wave `wave`'s range inside the launch, for a tile that is not whole (the ragged one, or an id past the last tile: none)
RVTILE_HD int32_t wave_rows_left(const TileWalk &w, uint32_t tile, uint32_t wave, uint32_t wave_rows) {
    if (tile != w.first_ragged_tile) return 0;
    const uint32_t before = wave * wave_rows;
    return before < w.ragged_rows ? static_cast<int32_t>(w.ragged_rows - before) : 0;
}

// byte of the companion where the codes of wave `wave` of tile `tile` start: one 32 x 32 -> 64 multiply and two additions
RVTILE_HD uint64_t wave_byte_at(const TileWalk &w, uint32_t tile, uint32_t wave) {
    return w.view_byte0 + static_cast<uint64_t>(tile) * w.tile_bytes + static_cast<uint64_t>(wave * w.wave_bytes);
}
// readable bytes of that wave range (the buffer descriptor's size): what the companion has left there, at most a wave range's
RVTILE_HD uint32_t wave_bytes_left(const TileWalk &w, uint64_t at) {
    const uint64_t left = w.bytes > at ? w.bytes - at : 0;
    return static_cast<uint32_t>(left < w.wave_bytes ? left : w.wave_bytes);
}

}  // namespace rvtile
