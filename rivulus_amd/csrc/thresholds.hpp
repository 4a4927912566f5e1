// EVERY switch between the kernels / paths of the backend, in one place: the value, what it decides, and the measurement that set it
// (files under profiles/, tools that re-measure it).  The launch code (fused_launch.hip, query.hip, strings.hip) reads these constants
// and nothing else; tests/test_paths_gpu.py asserts the path taken on either side of every row.  Boxes differ by +- 4 % and several
// crossovers were measured inside that noise: the values are the middle of the measured band, not a sharp edge.
#pragma once
#include <cstdint>

namespace rvt {
// ---- which kernel runs the pass (fused_launch.hip, fused_begin) -----------------------------------------------------------------
// A predicate nobody has run over these buffers is SAMPLED before its first launch is sized (1024 blocks of 1024 rows, ~10 us):
// below this many rows a mis-sized pass costs less than the sample.                     profiles/README.md "the first call", tools/dense_one.py
constexpr uint64_t kSampleFromRows = uint64_t{1} << 25;
// The direct (register-staged) kernel instead of the staged pass, from this selectivity on, by what the launch loads / projects:
//                                                              profiles/r04_dense_sweep.txt, r05d_dense_sweep.txt, tools/dense_sweep.py
constexpr double kDirectFromOneColumn = 0.52;            // one loaded column (r05d: 1.80 / 2.01 against the staged 1.77 / 2.03 ms at 30 / 50 %, 2.22 against 3.06 at 70 %)
constexpr double kDirectFromOneProjectedOfSeveral = 0.60;  // several loaded, one projected (the staged slots hold every survivor there)
constexpr double kDirectFromTwoProjected = 0.22;
constexpr double kDirectFromThreeProjected = 0.15;       // three or four
constexpr double kDirectFromTwoProjectedNullable = 0.35;   // columns that keep nulls carry a validity byte through the LDS slot: later
constexpr double kDirectFromThreeProjectedNullable = 0.22; //                                         tools/dense_nullable.py
// ... with ONE loaded column, 16 rows per lane (8192-row tiles) instead of 12 while fewer than this survive: 1e9 rows at 30 / 50 / 70 /
// 84 % kept: 1.80 / 2.01 / 2.30 / 2.43 ms against 2.18 / 2.20 / 2.22 / 2.33      tools/dense_sweep.py, tools/direct_geometry.py, profiles/r05d_dense_sweep.txt, r05d_direct_geometry.txt
constexpr double kDirectTallBelow = 0.62;
// Staged geometries: a wave whose expected survivors x 1.1 + 3 sigma (binomial) pass its LDS slot walks down to geometries whose
// slots hold a larger share of a wave's rows.                                            tools/roomy_ab.py, profiles/README.md
constexpr double kCrowdedMargin = 1.1, kCrowdedSigmas = 3.0;
// Survivors that come in RUNS (sorted / clustered tables): the redo kernel costs ~kRedoMsPerShare ms per 1e9 rows x the share of wave
// ranges it re-reads; the direct kernel costs kDirectPenaltyAt0 - kDirectPenaltySlope x selectivity ms more than the staged pass.  The
// direct kernel runs when the first exceeds the second (never below kDirectPenaltyFloor).   profiles/r05_skew_sweep.txt, tools/skew_sweep.py
// (Both sides got cheaper since -- the redo kernel's whole-line stores: ~2.2-2.8 ms per share; the direct kernel's 16-row tiles: 0.46 /
// 0.27 / 0.02 ms more than the staged pass at 10 / 20 / 30 % -- by about the same factor: the rule still picks the faster launch on
// either side of its crossover at ~15 % kept.                                   profiles/r05d_skew_rule_check.txt, tools/skew_rule_check.py)
constexpr double kRedoMsPerShare = 3.5, kDirectPenaltyAt0 = 0.9, kDirectPenaltySlope = 1.3, kDirectPenaltyFloor = 0.1;
// ... a measured redo share is trusted while the selectivity stayed within this of what it was then, and for slots no roomier than
// this much of a wave's rows beyond the slots it was measured with
constexpr double kRedoMemorySelectivityBand = 0.15, kRedoMemorySlotBand = 0.05;
// Output buffers from the predicate's known selectivity x kOutSizingFactor + kOutSizingSlack of the rows, for tables this big (the
// sample's 1024 blocks are off by 1 % of the rows, one sigma, over runs of 1e5 rows); smaller tables: every row.   tests/test_skew_gpu.py
constexpr uint64_t kOutSizingFromRows = uint64_t{1} << 25;
constexpr double kOutSizingFactor = 1.2, kOutSizingSlack = 0.02;
// A table whose survivors sit in a few LONG STRETCHES (sorted on the predicate's column) is cut at the edges the sample's profile shows
// (its 1024 blocks in table order) and filtered stretch by stretch, each with the kernel its own density asks for (run_segmented_pass):
// a block counts as sparse up to / dense from these shares of its 1024 sampled rows; a plan is at most kStretchesMost stretches of at
// least kStretchLeastBlocks blocks (every stretch costs a launch and a ~30 us read-back: runs of 1e7 rows in 1e9 are 100 stretches), all
// sparse or dense; a selectivity counted by a later pass outranks a profile that promised something else by more than kStretchKnownBand.
//                                                                                       profiles/r05c_skew_sweep.txt, tools/skew_sweep.py
constexpr double kStretchSparseUpTo = 0.30, kStretchDenseFrom = 0.55, kStretchKnownBand = 0.05;
constexpr int kStretchLeastBlocks = 24, kStretchesMost = 4;
// ... for tables this big: a stretch more costs a launch and a read-back, ~55 us per query over one pass -- 4e7 / 1.3e8 / 2.7e8 / 5e8 sorted
// rows at 10 % kept: 0.156 / 0.249 / 0.461 / 0.763 ms against 0.106 / 0.246 / 0.458 / 0.786 as one pass (50 %: 0.170 / 0.344 / 0.604 /
// 1.046 against 0.128 / 0.326 / 0.629 / 1.140)                                             profiles/r05d_stretches_by_rows.txt, tools/stretch_rows.py
constexpr uint64_t kStretchFromRows = uint64_t{1} << 28;

// ---- narrow companions of resident Int64 columns (narrow.hip, narrow_rule.hpp) ------------------------------------------------------
// A values buffer the lean one-column pass has read from end to end this many times gets 2- or 4-byte frame-of-reference codes, and the
// lean passes after that read those.  The build is a min/max pass and a pack pass over the 8-byte values (1.27 + 1.85 ms of kernels per
// 1e9 rows, 4.4 ms on the calls around it), the pass over codes saves 0.53 ms of 1.33 per scan -- break-even after ~8 further scans (~6
// at 2^28 rows, ~11 at 2^25): the first scan alone says nothing about a second one (a one-shot collect() must
// not pay for codes nobody reads), the second one does.  Buffers below kNarrowFromRows elements are left alone: a pass over them is
// launch and read-back time, not bytes (plain / codes, ms per call: 2^20 0.032 / 0.036, 2^22 0.041 / 0.038, 2^24 0.054 / 0.047, 2^25 0.077 /
// 0.058, 2^28 0.388 / 0.235; the size below which a first call is not sampled either).  Option "narrow_codes": 1 packs at
// the first whole scan whatever the size (tests), -1 never.                      tests/test_narrow_codes_gpu.py, profiles/narrow_costs.json
constexpr uint64_t kNarrowAfterWholeScans = 2;
constexpr uint64_t kNarrowFromRows = uint64_t{1} << 25;

// ---- which columns the pass carries (query.hip, filter_by_groups) ---------------------------------------------------------------
// Columns compacted AFTER the pass at its wave offsets (compact_ranges_kernel) instead of inside it, for tables this big:
constexpr uint64_t kRangesFromRows = uint64_t{1} << 24;
// plain columns the predicate does not read, while the predicate keeps at most this share (10-15 % faster at 10 and 20 % kept, a
// wash from 30 % on; nullable ones always: a pass with output bitmaps is the weakest launch there is)       profiles/r04d_*, tools/wide_ab.py
constexpr double kDeferPlainUpTo = 0.25;
// the column groups beyond the first of a wide projection, while at most this share survives (past it the direct kernel's whole-line
// stores are 5 % ahead for plain columns): rows x 20 <= length x 11                                           tools/wide_ab.py
constexpr uint64_t kRangesSparseNum = 11, kRangesSparseDen = 20;
// RecordBatch::filter by a BooleanArray without a chained pass (mask_select_kernel + scan + compact_ranges_kernel): plain columns of a
// selection denser than this go back to the direct kernel's pass                                              profiles/r04_bool_x_*, r05_batch_bool*
constexpr double kMaskPathPlainUpTo = 0.55;
// ... its outputs sized from the predicate's last selectivity (the compaction queued behind the scan, no host round trip) up to:
constexpr double kMaskPathAssumeUpTo = 0.5;

// ---- windows of RecordBatches (query.hip) ------------------------------------------------------------------------------------------
constexpr uint32_t kSpeculateFromBatches = 4096;   // the query runs on the assumed (regular) window while the walk validates it
constexpr uint32_t kWalkThreadsFromBatches = 16384;  // the handle walk is split over host threads            profiles/r04_batch_sweep.json
constexpr uint32_t kWalkThreads = 8;               // (16 measured slower: profiles/r05_batch_sweep.txt)

// ---- String / Boolean columns behind the pass (strings.hip) -------------------------------------------------------------------------
constexpr double kStrTilesFrom = 0.50;             // source-tile order instead of (start, length) lists            tools/str_sweep.py, profiles/r04c_*
constexpr double kBoolCapFactor = 1.25;            // Boolean outputs sized for the expected survivors x this + kBoolCapSlack rows
constexpr uint64_t kBoolCapSlack = 65536;

// ---- inner hash join (join.hip, probe_table) -----------------------------------------------------------------------------------------
// A probe row's match list of up to this many build rows is written by its own lane (join_probe_emit<1>); a table with longer lists
// probes with join_probe_emit<2>, which hands those lists to the whole workgroup.  (A table whose lists all hold one row takes
// join_probe_emit<0>, the plain compaction: no threshold.)  Set by reasoning -- a lane writing 32 pairs costs about what handing
// them to the workgroup costs -- NOT by a sweep; profiles/r06_join_bench.jsonl times 8 rows per key on the lane path (tools/join_bench.py).
constexpr uint32_t kJoinLaneListMost = 32;
// rv_hash_join_chunked's count pass: batches of exactly this many probe rows (the reference's 1024, streaming_planner.rs:32; a quarter of
// a 4096-row probe tile) are counted from per-lane partial sums (join_probe_count_batched<true>: no atomics, no LDS counters); every
// other batch size takes the general pass (join_probe_count_batched<false>: a wave scan per step, LDS counters, integer atomics for
// batches that span tiles).  Not a crossover: the fast form exists for this one size only.   tests/test_stream_join_gpu.py
constexpr uint64_t kJoinFastBatchRows = 1024;

// ---- string dictionary (string_dict.hip, rv_string_dict_build) ----------------------------------------------------------------------
// Slots per non-null row of the source column, rounded up to a power of two: 2 keeps the table at most half full, the load the join's
// table has (join.hip).  Not a crossover and not swept: with linear probing the expected chain at 50 % is 1.5 slots for a hit and 2.5
// for a miss, and every slot is one 8-byte word -- 16 bytes per row at most, next to the strings themselves.   tools/string_key_bench.py
constexpr uint64_t kStrDictSlotsPerRow = 2;

// ---- arithmetic expressions (arith.hip) -----------------------------------------------------------------------------------------------
// Workgroups of 256 lanes one arith_kernel launch takes at most: eight per CU of a 256-CU part, what the other one-lane-per-row kernels
// take (grid_for_words); longer columns are grid-strided.  Not a crossover and not swept.              tools/arith_bench.py
constexpr uint64_t kArithGridMost = 2048;

// ---- grouped aggregation (group_agg.hip) -------------------------------------------------------------------------------------------------
// Up to this many groups every workgroup of the accumulate kernel keeps its own accumulators in LDS (group_accumulate<lds>: LDS integer
// atomics per run of equal ids, one global integer atomic per group, accumulator and workgroup at the end); more groups take global
// integer atomics per run (group_accumulate<global>).  The value is what 128 KiB of a CU's 160 KiB of LDS hold of ONE accumulator (8 bytes per group): a
// launch takes as many accumulators as fit that budget (4 up to a quarter of this many groups, 1 from half on), so more aggregates
// cost more passes over the ids, never the global form.  Not a crossover but
// the LDS's capacity: the sweep of G at 2^28 rows, SUM + COUNT_ROWS, shows the LDS form ahead wherever it fits -- accumulate stage 0.98 /
// 2.9 / 4.1 / 7.7 ms at G = 1024 / 4096 / 8193 / 16384 against 22.5 ms for the global form at G = 16385 and 22.6 at 65536 (the global
// form runs at the rate of scattered 8-byte atomics whatever G is).          profiles/group_agg_bench.txt, tools/group_agg_bench.py --sweep
constexpr uint64_t kGroupAggLdsGroupsMost = 16384;
// Float64 SUM (group_f64_sum): a group's list of up to this many rows is summed by one wave (16 strided additions per lane, then the
// butterfly), a longer one by the four waves of the workgroup.  Part of what fixes the order of the additions: changing it changes the
// bits of inexact sums.  Set by reasoning, not by a sweep (the path's speed is not tuned).
constexpr uint32_t kGroupAggWaveListMost = 1024;
// rv_hash_aggregate / rv_group_ids refuse more distinct keys than this unless option "agg_max_groups" says otherwise: 2^27 slots of
// 8 bytes bound the group table at 1 GiB.  A limit, not a crossover.
constexpr uint64_t kGroupAggGroupsMostDefault = uint64_t{1} << 26;

// ---- sort (sort.hip) ------------------------------------------------------------------------------------------------------------------------
// Rows per lane of a tile of the radix passes (sort_tile_hist, sort_scatter: one workgroup of 256 lanes per tile, so 2048 rows).  It
// decides what a tile stages in LDS (12 bytes per row + 1 for the digit, with the counters 32 KiB: four workgroups per CU) and how many per-tile digit counts
// a pass scans (256 per 2048 rows: 1 byte per row through the scan against the 32 a pass moves).  Not a crossover; set by that reasoning,
// NOT by a sweep -- 16 rows per lane would halve the counts and leave two workgroups per CU.                       tools/sort_bench.py
constexpr uint32_t kSortRowsPerLane = 8;

// ---- top-k (topk.hip) -------------------------------------------------------------------------------------------------------------------------
// The radix select refines its cut by one more pass over the key column while differing digit positions remain and the candidates
// number more than rows / kTopKRefineDivisor.  By bytes: a refine pass reads 8 bytes per ROW of the table; it saves at most the sort of
// the candidates it sheds, about 296 derived bytes per CANDIDATE -- so a pass pays while candidates > rows x 8 /
// 296 = rows / 37, rounded to the power of two below.  The value is that reasoning.  The sweep over {8, 32, 128} at 2^28 rows agrees with it
// where the candidates are full-width (3.1 % of the rows, six bytes left to sort: 3.75 ms unrefined against 3.72 refined -- the break-even)
// and shows it conservative where they differ in one byte only, whose sort is one pass (8.5 % of the rows: 2.82 ms unrefined against
// 2.88; 2.1 %: 2.33 against 2.75).  32 is within 2.5 % of the best divisor on every shape at k = 100 (DESIGN.md section 4 K11 has the
// table).  Option "top_k_refine_divisor" overrides it (tests).
//                                                                                tools/topk_bench.py --sweep, profiles/topk_bench.txt
constexpr uint64_t kTopKRefineDivisor = 32;
// Below this many rows rv_top_k_indices / rv_top_k sort the whole column and keep the first k: the select is a dozen launches and two or
// three read-backs whatever the size, the sort of a short column a few more launches and one read-back.  A launch-bound crossover: k = 100
// over random Int64, select / sort 2^19 0.366 / 0.348 ms, 2^20 0.393 / 0.382, 2^21 0.395 / 0.459, 2^22 0.411 / 0.626 (below 2^12 rows the
// select refines to the last digit and is 2.4 x behind).  Option "top_k_select_from_rows" overrides it (tests).
//                                                                                tools/topk_bench.py --sweep, profiles/topk_bench.txt
constexpr uint64_t kTopKSelectFromRows = uint64_t{1} << 21;
// Rows per lane of a tile of the collect (topk_tile_count, topk_collect: one workgroup of 256 lanes per tile, so 2048 rows): one count per
// tile goes through the scan, 4 bytes per 2048 rows, and a wave keeps one ballot per step in registers.  Not a crossover; the sort's tile,
// by the sort's reasoning, NOT a sweep.
constexpr uint32_t kTopKCollectRowsPerLane = 8;
}  // namespace rvt
