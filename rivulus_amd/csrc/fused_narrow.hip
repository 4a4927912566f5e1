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
// PACKED codes (FF_PACK10 beside FF_NARROW16; narrow_rule.hpp): a column whose values need 10 bits keeps them six per 8-byte word, in a
// layout whose word l of a 384-element super-group holds rows 2l, 2l + 1 of its three 128-row groups -- the pair loads' row-to-lane
// mapping, so ranks, masks, write-out order, wave totals and the redo list are the 2-byte form's.  A lane loads one 8-byte word per
// three pairs (scan_frontend.hpp, load_rows_packed) and unpacks a row with one bit-field extract where the 2-byte form has an `and` or a
// shift; everything behind the unpack is the same instruction stream, the cells staged in LDS are 2-byte codes.  48 rows per lane
// occupy the 16 code registers per lane that 32 rows of 2-byte codes do: the pass reads 1.33 GB instead of 2.00 GB per 1e9 rows and
// pays a tile's fixed part once per 49 152 rows.  Measured (profiles/narrow4_*): 0.470 -> 0.438 ms; 12 040 cycles per 48-row tile of
// wave 1 against 9 085 per 32-row tile (8 027 per 32 rows, -12 %), which is what the per-tile cost model predicted (11 460) and far
// from what the byte model did (0.353 ms): the pass stands at the instruction issue of its waves, not at HBM.  It needs THREE stages
// of slots: with two (what the plain form's LDS rule gives 3072-row wave ranges) the look-back is exposed, 15 280 cycles per tile and
// 0.57 ms -- so its slots are sized as the plain form sizes two stages, and its plain re-run runs two-staged (fused_launch.hip,
// size_staged).
// Their whole tiles are staged a raw word (three pairs) at a time, by one of three forms chosen per tile from the class of the code
// interval (narrow_sides.hpp: `code >= lo`, `code <= hi`, or subtract-and-compare), with one clamp per pair and a spare cell behind every
// slot, and written out in whole 128-byte lines (fused_kernel.hpp, kPack10): 21 listed instructions per pair where the form above has 25,
// 0.396 -> 0.369 ms for the headline kernel (profiles/narrow6_steps.txt).
// The pass is bound by the vector instructions of its waves, not by HBM latency (tools/narrow_stamp.py, profiles/narrow2_stamps_*.txt:
// a wave waits ~50 of 11 000-15 000 cycles per tile for its codes; evaluating them and waiting at the barrier for the other waves on the
// SIMD to evaluate theirs is 80-87 %).  Tried on top of the above and taken out again: THREE sets of pairs per lane, the tile two
// ahead requested at the top of an iteration (ids drawn four ahead, loop unrolled by three) -- 128 VGPRs, and the headline kernel
// took 0.612 ms against 0.576 ms with one set (1e9 rows, same box, alternating processes; profiles/narrow2_steps.txt).  The two kept
// steps one by one: compare in code space 0.772 -> 0.603 ms, codes in the slots 0.603 -> 0.564 ms.  The staging loop above:
// 0.564 -> 0.478 ms with the branch-free stores, 0.495 ms with stores under an exec mask (two vector instructions fewer per pair, four
// exec writes more: taken out; profiles/narrow3_steps.txt).  At 0.478 ms the pass moves its 2.93 GB at 6.1 TB/s: what a streaming
// kernel reaches on this part.
// An entry carries its PLAIN TWIN, the lean Int64 instantiation of its geometry over the 8-byte values (RV_NARROW below names both, so a
// geometry without one cannot be listed): what re-runs a pass over codes after an output overflow.  16, 8, 4 and 24 rows per lane are
// geometries of the lean table (fused_lean1.hip instantiates them: declared here, not built a second time); 32, 48 and 12 are built in
// this unit only -- 64 and 96 value registers per lane at 32 and 48 rows spill at 128 VGPRs (profiles/narrow4_resources.txt has their
// scratch): a rare second pass, never the launch a query is sized for.
// The first entry of a flags class is the default geometry; kNarrowTallRows rows per lane is what a launch without per-batch counts
// takes (fused_launch.hip): a tile's codes are a quarter or half of its rows' bytes, so twice the rows per lane put twice the bytes
// on their way per request and halve the per-tile costs (barrier, ticket, descriptor) per row.  The geometries with fewer rows per lane
// are the ones the plain lean form walks down through for denser selections.
#define RV_NARROW(R, FLAGS) ::rvk::FusedEntry{1, R, 2, 16, FLAGS, &::rvk::fused_filter_compact<1, R, 2, 16, FLAGS>, &::rvk::fused_filter_compact<1, R, 2, 16, ::rvk::FF_ONE_I64>}
extern template __global__ void fused_filter_compact<1, 16, 2, 16, FF_ONE_I64>(const FusedParams);
extern template __global__ void fused_filter_compact<1, 8, 2, 16, FF_ONE_I64>(const FusedParams);
extern template __global__ void fused_filter_compact<1, 4, 2, 16, FF_ONE_I64>(const FusedParams);
extern template __global__ void fused_filter_compact<1, 24, 2, 16, FF_ONE_I64>(const FusedParams);
const FusedEntry *fused_entries_narrow(size_t *n) {
    static const FusedEntry t[] = {
        RV_NARROW(16, FF_ONE_I64 | FF_NARROW16), RV_NARROW(32, FF_ONE_I64 | FF_NARROW16),
        RV_NARROW(8, FF_ONE_I64 | FF_NARROW16),  RV_NARROW(4, FF_ONE_I64 | FF_NARROW16),
        // (4-byte codes: no tall geometry yet.  32 rows per lane compile to 108 VGPRs without scratch in this form -- the parent's widened
        //  form spilled -- but the geometry has not been measured, and the class keeps what has been)
        RV_NARROW(16, FF_ONE_I64 | FF_NARROW32), RV_NARROW(8, FF_ONE_I64 | FF_NARROW32), RV_NARROW(4, FF_ONE_I64 | FF_NARROW32),
        // diagnostic (options "stamp" / "debug": phase cycle sums and the ablations of a pass over 2-byte codes, tools/narrow_stamp.py)
        RV_NARROW(16, FF_STAMP | FF_ONE_I64 | FF_NARROW16), RV_NARROW(32, FF_STAMP | FF_ONE_I64 | FF_NARROW16),
        // packed codes (FF_PACK10, always with FF_NARROW16: the cells staged in LDS stay 2-byte codes): kPackedTallRows rows per lane
        // first, then the geometries the walk down at denser selections takes; a selection denser than the 12-row one admits reads the
        // 8-byte values through the plain lean pass (fused_launch.hip, choose_launch)
        // (1e9 rows, x > 899, kernel ms by events, same box, alternating processes: 48 rows per lane 0.438, 36 0.489, 24 0.589, against
        //  0.470 of the 2-byte codes at 32; 36 was instantiated for the experiment only: profiles/narrow4_steps.txt)
        RV_NARROW(48, FF_ONE_I64 | FF_NARROW16 | FF_PACK10), RV_NARROW(24, FF_ONE_I64 | FF_NARROW16 | FF_PACK10),
        RV_NARROW(12, FF_ONE_I64 | FF_NARROW16 | FF_PACK10),
        RV_NARROW(48, FF_STAMP | FF_ONE_I64 | FF_NARROW16 | FF_PACK10), RV_NARROW(24, FF_STAMP | FF_ONE_I64 | FF_NARROW16 | FF_PACK10),
    };
    *n = sizeof(t) / sizeof(t[0]);
    return t;
}
}  // namespace rvk
