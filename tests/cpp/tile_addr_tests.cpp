// CPU test of the staged pass's per-tile arithmetic (rivulus_amd/csrc/tile_addr.hpp): a stand-alone program, built with g++ (plain and
// with -fsanitize=address,undefined) by tests/test_tile_addr_cpu.py.  The specification is the code the header replaced, as it stood in
// the tile loop of fused_kernel.hpp and in load_rows_packed / load_rows_narrow of scan_frontend.hpp (`ref` below): a wave range's first
// element `first` = offset + tile * TILE + wave * ROWS_PER_WAVE, its codes at byte first / 384 * 512 (packed) or first * BYTES, the
// descriptor's size clamped to the companion's bytes left, `full` = tile_base + TILE <= n, and the ragged tile's `left` clamps.
// Every geometry of the narrow table x code width x view offset x n x companion size x tile id x wave is compared, nothing is skipped,
// and the number of comparisons is printed: the Python side works the same number out from the lists it knows.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../rivulus_amd/csrc/tile_addr.hpp"

namespace ref {
struct Wave {
    uint64_t at;      // byte of the companion where the wave's codes start
    uint32_t nbytes;  // the buffer descriptor's size
    bool full;
    int32_t rem;  // rows of the wave inside the launch (read when !full only)
};
// code_bytes 0: packed
static Wave wave_of(uint64_t offset, uint64_t n, uint64_t bytes, int r, int waves, int code_bytes, uint32_t tile, uint32_t wave) {
    const uint64_t ROWS_PER_WAVE = 64u * static_cast<uint64_t>(r), TILE = ROWS_PER_WAVE * static_cast<uint64_t>(waves);
    Wave w{};
    const uint64_t first = offset + static_cast<uint64_t>(tile) * TILE + static_cast<uint64_t>(wave) * ROWS_PER_WAVE;
    const uint64_t WAVE_BYTES = code_bytes == 0 ? 512u * (static_cast<uint64_t>(r) / 6) : 64u * static_cast<uint64_t>(r) * static_cast<uint64_t>(code_bytes);
    w.at = code_bytes == 0 ? first / 384u * 512u : first * static_cast<uint64_t>(code_bytes);
    const uint64_t left = bytes > w.at ? bytes - w.at : 0;
    w.nbytes = static_cast<uint32_t>(left < WAVE_BYTES ? left : WAVE_BYTES);
    const uint64_t tile_base = static_cast<uint64_t>(tile) * TILE;
    const uint64_t wave_base = tile_base + static_cast<uint64_t>(wave) * ROWS_PER_WAVE;
    w.full = tile_base + TILE <= n;
    w.rem = 0;
    if (!w.full) {
        const int64_t l = static_cast<int64_t>(n) - static_cast<int64_t>(wave_base);
        w.rem = static_cast<int32_t>(l < 0 ? 0 : (l > (1 << 30) ? (1 << 30) : l));
    }
    return w;
}
}  // namespace ref

static uint64_t compared = 0, failed = 0;

static void check(uint64_t offset, uint64_t n, uint64_t bytes, int r, int waves, int code_bytes, uint32_t tile, uint32_t wave) {
    const ref::Wave want = ref::wave_of(offset, n, bytes, r, waves, code_bytes, tile, wave);
    const rvtile::TileWalk w = rvtile::codes_walk(n, r, waves, offset, bytes, code_bytes);
    const uint64_t at = rvtile::wave_byte_at(w, tile, wave);
    // the kernel's form: the walk moved to this wave's codes of tile 0 before the loop, tiles counted from there
    rvtile::TileWalk mine = w;
    mine.view_byte0 = rvtile::wave_byte_at(w, 0u, wave);
    const uint64_t at_loop = rvtile::wave_byte_at(mine, tile, 0u);
    const uint32_t nbytes = rvtile::wave_bytes_left(w, at);
    const bool full = rvtile::tile_full(w, tile);
    const int32_t rem = full ? 0 : rvtile::wave_rows_left(w, tile, wave, 64u * static_cast<uint32_t>(r));
    // a launch that reads the 8-byte values fills the row part alone: the same answers
    const rvtile::TileWalk rows = rvtile::rows_walk(n, r, waves);
    const bool same_rows = rvtile::tile_full(rows, tile) == full && (full || rvtile::wave_rows_left(rows, tile, wave, 64u * static_cast<uint32_t>(r)) == rem);
    compared += 1;
    if (at != want.at || at_loop != want.at || nbytes != want.nbytes || full != want.full || rem != want.rem || !same_rows) {
        if (failed++ < 20)
            std::printf("MISMATCH r %d code_bytes %d offset %" PRIu64 " n %" PRIu64 " bytes %" PRIu64 " tile %u wave %u: at %" PRIu64 " / %" PRIu64 " / %" PRIu64
                        " nbytes %u / %u full %d / %d rem %d / %d rows-only %d\n",
                        r, code_bytes, offset, n, bytes, tile, wave, at, at_loop, want.at, nbytes, want.nbytes, full, want.full, rem, want.rem, same_rows);
    }
}

int main() {
    const int kWaves = 16;
    const int geometries[] = {48, 24, 12, 32, 16, 8, 4};  // rows per lane of the narrow table (fused_narrow.hip)
    const int widths[] = {0, 2, 4};                       // packed, 2- and 4-byte codes
    // view offsets: the first super-groups, one whose packed byte offset needs 34 bits, and two that put every width's byte offset past
    // 2^32 and past 2^40
    const uint64_t offsets[] = {0, 384, 768, 384ull * ((1ull << 24) + 1), 384ull * ((1ull << 23) + 3), 384ull * ((1ull << 31) + 5)};
    for (int r : geometries) {
        const uint64_t wave_rows = 64u * static_cast<uint64_t>(r), tile_rows = wave_rows * kWaves;
        // n on both sides of a tile, of a wave range and of a super-group; short launches; the GPU tests' 3 tiles + 77 rows
        const uint64_t ns[] = {1, 17, tile_rows - 1, tile_rows, tile_rows + 1, 3 * tile_rows + 5 * wave_rows - 1, 3 * tile_rows + 5 * wave_rows, 3 * tile_rows + 5 * wave_rows + 1,
                               2 * tile_rows + 384 * 2 - 1, 2 * tile_rows + 384 * 2, 2 * tile_rows + 384 * 2 + 1, 3 * tile_rows + 77};
        for (int cb : widths) {
            if (cb == 0 && r % 6 != 0) continue;  // packed geometries: whole super-groups per wave range
            for (uint64_t offset : offsets)
                for (uint64_t n : ns) {
                    const uint64_t ntiles = (n + tile_rows - 1) / tile_rows;
                    const uint32_t tiles[] = {0u, 1u, static_cast<uint32_t>(ntiles - 1), static_cast<uint32_t>(ntiles), 0xFFFFFFFFu};
                    // the companion ends with the view (its last super-group padded), or goes on behind it
                    for (uint64_t count : {offset + n, offset + n + 5000}) {
                        const uint64_t bytes = cb == 0 ? (count + 383) / 384 * 512 : count * static_cast<uint64_t>(cb);
                        for (uint32_t tile : tiles)
                            for (uint32_t wave = 0; wave < static_cast<uint32_t>(kWaves); ++wave) check(offset, n, bytes, r, kWaves, cb, tile, wave);
                    }
                }
        }
    }
    std::printf("compared %" PRIu64 "\nfailed %" PRIu64 "\n", compared, failed);
    return failed ? 1 : 0;
}
