#include "fused_table.hpp"
namespace rvk {
// The lean Int64 form (one column, no null bitmap, one compare term) reading the column's narrow companion: 2-byte (FF_NARROW16) or
// 4-byte (FF_NARROW32) frame-of-reference codes instead of the 8-byte rows (scan_frontend.hpp, load_rows_narrow).  What these
// instantiations do differently from the plain form (fused_kernel.hpp, the `kNarrow != 0` branches):
//   - a lane holds the tile as raw code pairs (one register per pair of 2-byte codes), requested one tile ahead like the plain form's rows;
//   - the compare term runs in code space: the host lowers it to ONE interval of codes (narrow_term.hpp: a complement is folded into the
//     interval it is in wrap-around arithmetic; the empty set over 4-byte codes, which is none, keeps its negate flag, tested once per
//     tile), a row costs one 32-bit subtract and one unsigned compare;
//   - the staging loop of a whole tile carries nothing that is the same for every row of it: no negate flag, no `full` / `project`
//     test, ranks formed as LDS addresses from a scalar base and CLAMPED to the slot's last cell instead of compared with its capacity
//     (a wave that outgrows its slot goes to the redo kernel anyway), and branch-free stores -- a lane without a survivor writes to
//     its cell of the wave's dump area.  24 instructions per pair of rows (15 vector, 2 LDS, 6 scalar, one wait; no branch, no exec
//     write) where the form before had 35; the ragged last tile, a launch that projects nothing and the one negated term run a second form with the tests and the flip;
//   - survivors are staged as codes and widened (value = base + code) where they are written out; the slots hold the same ROWS as the
//     plain form's (fused_launch.hip, size_staged), in a quarter or half of the LDS bytes.
// Same values, same order, same counts and redo list as the plain form, bit for bit.
// The pass is bound by the vector instructions of its waves, not by HBM latency (tools/narrow_stamp.py, profiles/narrow2_stamps_*.txt:
// a wave waits ~50 of 11 000-15 000 cycles per tile for its codes; evaluating them and waiting at the barrier for the other waves on the
// SIMD to evaluate theirs is 80-87 %).  Tried on top of the above and taken out again: THREE sets of pairs per lane, the tile two
// ahead requested at the top of an iteration (ids drawn four ahead, loop unrolled by three) -- 128 VGPRs, and the headline kernel
// took 0.612 ms against 0.576 ms with one set (1e9 rows, same box, alternating processes; profiles/narrow2_steps.txt).  The two kept
// steps one by one: compare in code space 0.772 -> 0.603 ms, codes in the slots 0.603 -> 0.564 ms.  The staging loop above:
// 0.564 -> 0.478 ms with the branch-free stores, 0.495 ms with stores under an exec mask (two vector instructions fewer per pair, four
// exec writes more: taken out; profiles/narrow3_steps.txt).  At 0.478 ms the pass moves its 2.93 GB at 6.1 TB/s: what a streaming
// kernel reaches on this part.
// The first entry of a flags class is the default geometry; kNarrowTallRows rows per lane is what a launch without per-batch counts
// takes (fused_launch.hip): a tile's codes are a quarter or half of its rows' bytes, so twice the rows per lane put twice the bytes
// on their way per request and halve the per-tile costs (barrier, ticket, descriptor) per row.  The geometries with fewer rows per lane
// are the ones the plain lean form walks down through for denser selections.
const FusedEntry *fused_entries_narrow(size_t *n) {
    static const FusedEntry t[] = {
        RV_FUSED(1, 16, 2, 16, FF_ONE_I64 | FF_NARROW16), RV_FUSED(1, 32, 2, 16, FF_ONE_I64 | FF_NARROW16),
        RV_FUSED(1, 8, 2, 16, FF_ONE_I64 | FF_NARROW16),  RV_FUSED(1, 4, 2, 16, FF_ONE_I64 | FF_NARROW16),
        // (4-byte codes: no tall geometry yet.  32 rows per lane compile to 108 VGPRs without scratch in this form -- the parent's widened
        //  form spilled -- but the geometry has not been measured, and the class keeps what has been)
        RV_FUSED(1, 16, 2, 16, FF_ONE_I64 | FF_NARROW32), RV_FUSED(1, 8, 2, 16, FF_ONE_I64 | FF_NARROW32), RV_FUSED(1, 4, 2, 16, FF_ONE_I64 | FF_NARROW32),
        // diagnostic (options "stamp" / "debug": phase cycle sums and the ablations of a pass over 2-byte codes, tools/narrow_stamp.py)
        RV_FUSED(1, 16, 2, 16, FF_STAMP | FF_ONE_I64 | FF_NARROW16), RV_FUSED(1, 32, 2, 16, FF_STAMP | FF_ONE_I64 | FF_NARROW16),
    };
    *n = sizeof(t) / sizeof(t[0]);
    return t;
}
// The plain lean Int64 instantiation of a narrow geometry the lean table (fused_lean1.hip) does not hold: what re-runs a pass over
// codes after an output overflow, over the 8-byte values.  (Its 64 value registers per lane spill at 128 VGPRs: a rare second pass,
// never the launch a query is sized for.)
FusedEntry narrow_tall_plain() { return RV_FUSED(1, kNarrowTallRows, 2, 16, FF_ONE_I64); }
}  // namespace rvk
