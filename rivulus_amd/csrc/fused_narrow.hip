#include "fused_table.hpp"
namespace rvk {
// The lean Int64 form (one column, no null bitmap, one compare term) reading the column's narrow companion: 2-byte (FF_NARROW16) or
// 4-byte (FF_NARROW32) frame-of-reference codes instead of the 8-byte rows (scan_frontend.hpp, load_rows_narrow).
// The first entry of a flags class is the default geometry; kNarrowTallRows rows per lane is what a launch without per-batch counts
// takes (fused_launch.hip): a tile's codes are a quarter or half of its rows' bytes, and a workgroup that keeps ONE tile of 16 rows per
// lane in flight has too few bytes on their way to cover HBM's latency -- twice the rows per lane, twice the bytes.  The geometries
// with fewer rows per lane are the ones the plain lean form walks down through for denser selections.
const FusedEntry *fused_entries_narrow(size_t *n) {
    static const FusedEntry t[] = {
        RV_FUSED(1, 16, 2, 16, FF_ONE_I64 | FF_NARROW16), RV_FUSED(1, 32, 2, 16, FF_ONE_I64 | FF_NARROW16),
        RV_FUSED(1, 8, 2, 16, FF_ONE_I64 | FF_NARROW16),  RV_FUSED(1, 4, 2, 16, FF_ONE_I64 | FF_NARROW16),
        // (4-byte codes: 32 rows per lane do not fit 128 VGPRs without spills; the class has no tall geometry)
        RV_FUSED(1, 16, 2, 16, FF_ONE_I64 | FF_NARROW32), RV_FUSED(1, 8, 2, 16, FF_ONE_I64 | FF_NARROW32), RV_FUSED(1, 4, 2, 16, FF_ONE_I64 | FF_NARROW32),
    };
    *n = sizeof(t) / sizeof(t[0]);
    return t;
}
// The plain lean Int64 instantiation of a narrow geometry the lean table (fused_lean1.hip) does not hold: what re-runs a pass over
// codes after an output overflow, over the 8-byte values.  (Its 64 value registers per lane spill at 128 VGPRs: a rare second pass,
// never the launch a query is sized for.)
FusedEntry narrow_tall_plain() { return RV_FUSED(1, kNarrowTallRows, 2, 16, FF_ONE_I64); }
}  // namespace rvk
