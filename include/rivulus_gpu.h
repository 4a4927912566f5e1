/*
 * rivulus_gpu.h -- C ABI of the MI355X (gfx950) execution backend for the
 * Rivulus filter / project / scan hot path.
 *
 * This header is the drop-in boundary.  The reference (CleConor/rivulus, pure
 * Rust) has no FFI of its own, so every entry point below names the reference
 * seam it stands behind (paths relative to the reference checkout):
 *
 *   S1  trait DataStream::next_batch            src/execution/stream.rs:25-28
 *       FilterStream / SelectStream             src/execution/stream.rs:116-213
 *   S2  RecordBatch::{filter,take,concat,slice} src/execution/record_batch.rs:92-342
 *   S3  PhysicalPlan::{Filter,Select}::execute  src/physical_plan/plan.rs:65-150
 *
 * Conventions
 *   - every function returns rv_status (0 == RV_OK); no exception crosses the ABI;
 *   - rv_last_error() returns a thread-local NUL-terminated message; where the
 *     reference defines the failure text, the text is the reference's;
 *   - plain pointers and sizes only; host pointers are borrowed for the duration
 *     of the call; device objects are opaque handles released with rv_free();
 *   - bit buffers are LSB-first (bit i lives in byte i/8, bit i%8), exactly the
 *     reference BitMap layout (src/execution/array/bitmap.rs:48-52,61-68);
 *     validity bit 1 == valid (src/execution/array/primitive.rs:31-33,53-57);
 *   - one rv_ctx == one device + one HIP stream, not thread-safe (mirrors the
 *     `&mut self` of DataStream::next_batch); different contexts are independent.
 */
#ifndef RIVULUS_GPU_H
#define RIVULUS_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RV_ABI_VERSION 4

typedef enum rv_status {
    RV_OK = 0,
    RV_ERR_INVALID_ARG = 1,
    RV_ERR_LENGTH_MISMATCH = 2, /* record_batch.rs:222-228 */
    RV_ERR_TYPE_MISMATCH = 3,   /* record_batch.rs:230-233, stream.rs:147-154 */
    RV_ERR_OUT_OF_BOUNDS = 4,   /* record_batch.rs:109-116, :93 */
    RV_ERR_UNSUPPORTED = 5,
    RV_ERR_DEVICE = 6,
    RV_ERR_OOM = 7,
    RV_ERR_INTERNAL = 8,
    RV_ERR_PARSE = 9            /* file_stream.rs:43-122: a CSV cell or line the schema does not accept */
} rv_status;

/* execution::schema::DataType, src/execution/schema.rs:1-8 */
typedef enum rv_dtype {
    RV_NULL = 0,
    RV_BOOLEAN = 1,
    RV_INT64 = 2,
    RV_FLOAT64 = 3,
    RV_STRING = 4
} rv_dtype;

/* the six compare operators of expressions::BinaryOperator, src/expressions/expr.rs:21-26.
 * RV_IS_TRUE is the predicate form the reference streaming path accepts today: a bare
 * Boolean column kept where value(i) == Some(true) (stream.rs:139-158, record_batch.rs:235-240). */
typedef enum rv_cmp {
    RV_EQ = 0,
    RV_NE = 1,
    RV_LT = 2,
    RV_GT = 3,
    RV_LE = 4,
    RV_GE = 5,
    RV_IS_TRUE = 6
} rv_cmp;

/* How a null cell behaves inside a compare term.
 *   RV_NULL_DROPS    streaming composition: a compare over a null cell is null and
 *                    RecordBatch::filter keeps only Some(true) (record_batch.rs:237,
 *                    boolean.rs:120-135) => the row is dropped.
 *   RV_NULL_IS_LEAST eager path: AnyValue ordering, Null == Null and Null < everything
 *                    (src/datatypes/series.rs:87-117), so <, <=, != keep null rows. */
typedef enum rv_null_policy {
    RV_NULL_DROPS = 0,
    RV_NULL_IS_LEAST = 1
} rv_null_policy;

/* Field-for-field view of PrimitiveArray<i64|f64> (primitive.rs:20-28) or BooleanArray
 * (boolean.rs:9-16).  Used for host memory (rv_upload / rv_download) and for
 * caller-owned device memory (rv_wrap). */
typedef struct rv_column {
    rv_dtype dtype;
    const void *values;      /* int64_t[] / double[]; RV_BOOLEAN: LSB-first bit buffer;
                                RV_STRING: the UTF-8 bytes (StringArray::data)            */
    const uint8_t *validity; /* NULL == no null bitmap; LSB-first, bit 1 == valid        */
    uint64_t offset;         /* element offset into values AND bit offset into bitmaps   */
    uint64_t length;         /* logical number of elements                               */
    /* RV_STRING only (string.rs:9-15): element i of the buffer spans
     * values[offsets[i] .. offsets[i+1]); offset + length + 1 entries are read.  A null element
     * spans zero bytes, as StringArray::new builds it (string.rs:34-38). */
    const int32_t *offsets;
    uint64_t data_bytes;     /* bytes in `values` (RV_STRING)                            */
} rv_column;

/* One `Column <op> Literal` term (planner.rs:134-189).  lit_type == RV_NULL is
 * Literal(AnyValue::Null); RV_BOOLEAN literals carry 0/1 in lit.i. */
typedef struct rv_term {
    uint32_t column; /* index into the cols[] array handed to the call */
    rv_cmp op;
    rv_dtype lit_type;
    union {
        int64_t i;
        double f;
        struct {            /* lit_type == RV_STRING: AnyValue::String literal (UTF-8, not NUL-terminated); */
            const char *ptr; /* String cells order byte-wise like Rust's str (series.rs:100-117)             */
            uint64_t len;
        } s;
    } lit;
} rv_term;

/* A predicate over compare terms.  expr == NULL: the AND of all terms (BinaryOperator::And, expr.rs:27).
 * Otherwise expr[0 .. n_expr) is the predicate in postfix order over
 *   0x00 .. 0x7F  push the truth of terms[code]
 *   RV_EXPR_AND   pop two, push a AND b      BinaryOperator::And (expr.rs:27), BooleanArray::and (boolean.rs:120-135)
 *   RV_EXPR_OR    pop two, push a OR b       BinaryOperator::Or  (expr.rs:28), BooleanArray::or  (boolean.rs:137-152)
 *   RV_EXPR_NOT   pop one, push NOT a        BooleanArray::not   (boolean.rs:154-165)
 * and must leave exactly one value.  Null semantics per policy:
 *   RV_NULL_DROPS     every term is a nullable BooleanArray (null where its cell is null), AND / OR / NOT are the
 *                     reference's strict operators (null if an operand is null, `false AND null = null`), and
 *                     RecordBatch::filter keeps Some(true): a row survives iff every cell the expression reads is
 *                     valid and the expression is true;
 *   RV_NULL_IS_LEAST  every term is the eager mask of plan.rs:112-130 (a definite bool per row, nulls ordered
 *                     lowest); AND = chained filters, OR / NOT the same algebra on those masks.
 * n_terms >= 1, at most 16 terms.  Expressions whose conjunctive normal form (or that of their negation) has at
 * most 16 literals run inside the single fused pass; larger ones are composed from per-term BooleanArrays. */
#define RV_EXPR_AND 0x80
#define RV_EXPR_OR 0x81
#define RV_EXPR_NOT 0x82
typedef struct rv_predicate {
    const rv_term *terms;
    uint32_t n_terms;
    rv_null_policy nulls;
    const uint8_t *expr; /* NULL: AND of all terms */
    uint32_t n_expr;
} rv_predicate;

/* On-device synthetic column, bit-identical to the CPU generator in oracle/
 * (SURVEY.md section 8d):  splitmix64(z): z += 0x9E3779B97F4A7C15;
 *   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *   return z ^ (z >> 31).
 * Row g = first_row + i (global index, so row-range shards agree):
 *   RV_INT64   value = (int64)(splitmix64(seed + g) % modulus)
 *   RV_FLOAT64 value = (double)(splitmix64(seed + g) >> 11) * 2^-53
 *   RV_BOOLEAN value = splitmix64(seed + g) % 100 < true_percent
 *   validity   bit   = splitmix64(validity_seed + g) % 100 >= null_percent
 * Under a null slot the generated value is kept as is (a null slot may hold anything).
 * `pattern` (ABI 4) replaces the hash h = splitmix64(seed + g) the values are made of -- the reference filters whatever
 * order its source has (plan.rs:112-147, file_stream.rs:122-198: file order), and ids / timestamps come sorted or in runs:
 *   RV_SYNTH_IID          h as above (independent rows: a tile's selectivity is the table's)
 *   RV_SYNTH_CLUSTERED    h = splitmix64(seed + g / run_rows): runs of run_rows equal cells
 *   RV_SYNTH_SORTED_ASC   q = g * ((2^64 - 1) / table_rows), a 64-bit fraction that grows with g:
 *                         RV_INT64 value = (q * modulus) >> 64, RV_FLOAT64 value = (double)(q >> 11) * 2^-53,
 *                         RV_BOOLEAN value = ((q * 100) >> 64) < true_percent   (table_rows 0: first_row + length)
 *   RV_SYNTH_SORTED_DESC  the same with q = (table_rows - 1 - g) * ((2^64 - 1) / table_rows)
 * The validity bits stay independent per row under every pattern. */
typedef enum rv_synth_pattern { RV_SYNTH_IID = 0, RV_SYNTH_CLUSTERED = 1, RV_SYNTH_SORTED_ASC = 2, RV_SYNTH_SORTED_DESC = 3 } rv_synth_pattern;
typedef struct rv_synth_spec {
    rv_dtype dtype;
    uint64_t seed;
    uint64_t first_row;
    uint64_t length;
    uint64_t modulus;      /* RV_INT64 only, > 0                                   */
    uint32_t true_percent; /* RV_BOOLEAN only                                      */
    int32_t with_validity; /* 0: no null bitmap                                    */
    uint64_t validity_seed;
    uint32_t null_percent;
    uint32_t pattern;      /* rv_synth_pattern; 0 = independent rows                */
    uint64_t run_rows;     /* RV_SYNTH_CLUSTERED: rows per run, > 0                 */
    uint64_t table_rows;   /* RV_SYNTH_SORTED_*: rows of the whole table (shards agree) */
} rv_synth_spec;

typedef struct rv_column_info {
    rv_dtype dtype;
    uint64_t length;
    uint64_t offset;
    int32_t has_validity; /* a null bitmap is attached                              */
    int64_t null_count;   /* -1 when not yet known                                  */
    uint64_t data_bytes;  /* RV_STRING: bytes of the logical elements, else 0       */
} rv_column_info;

typedef struct rv_ctx rv_ctx;         /* one device + one stream + scratch arena     */
typedef struct rv_dcolumn rv_dcolumn; /* device-resident array (values + validity)   */
typedef struct rv_comm rv_comm;       /* RCCL communicator, one rank per process     */
typedef struct rv_pending rv_pending; /* a fused launch queued by rv_filter_project_begin */
typedef struct rv_csv_reader rv_csv_reader; /* a CSV file parsed on the device, batch by batch */

/* ---- library / context ------------------------------------------------- */
uint32_t rv_abi_version(void);
const char *rv_last_error(void);
const char *rv_status_name(rv_status s);

/* number of HIP devices this process sees (0 without a GPU; never an error: the library reports, it does not fall back) */
int rv_device_count(void);
rv_status rv_ctx_create(int device, rv_ctx **out);
rv_status rv_ctx_destroy(rv_ctx *ctx);
rv_status rv_ctx_synchronize(rv_ctx *ctx);
/* hipStream_t of the context, for callers that interleave their own work. */
void *rv_ctx_stream(rv_ctx *ctx);
/* number of compute units of the context's device (grid sizing, reporting). */
rv_status rv_ctx_device_info(rv_ctx *ctx, int *compute_units, uint64_t *hbm_bytes, char *name,
                             size_t name_len);
/* Tuning / diagnostics.  Keys: "rows_per_lane" (R | waves << 8: geometry of the fused
 * kernel; 0 = default), "vec" (0 auto, 1 force 8-byte loads, 2 force 16-byte loads),
 * "cap_rows" (rows of a wave's LDS slot, 0 = as many as fit), "depth" (iterations between a
 * tile's aggregate and its write-out: 0 auto, 1, 2), "roomy" (1: size the LDS slots as for a dense selection -- one
 * workgroup per CU, two stages; 0 = decided per launch from the selectivity the context last saw with the same predicate:
 * a selectivity the default geometry's slots would not hold takes geometries with fewer rows per lane, results unchanged),
 * "direct" (the register-staged kernel for dense selections, direct_kernel.hpp: 0 = from a selectivity of 52 % (one loaded
 * column) / 60 % (one projected of several) / 22 % (two projected) / 15 % (three, four) known for the predicate, for value columns
 * without an output bitmap, 1 = whenever the launch is eligible, -1 = never; "direct_r" / "direct_waves": diagnostic, a named
 * geometry of it), "sample" (a predicate the context has not run over this data gets its selectivity from a strided sample before
 * its first launch is sized: 0 = for tables of 2^25 rows and more, k > 0 = from k rows on, -1 = never),
 * "skew" (survivors that come in RUNS -- a table sorted or clustered on the predicate's column -- fill some waves' LDS slots while
 * others stay empty; a wave range that outgrows its slot is re-read by the redo kernel at its reserved output offset.  0 = when the
 * share of such ranges the predicate is known to leave (the last staged pass, or the sample's histogram of 1024-row blocks on a first
 * call) would cost more than the direct kernel's slower scan, the direct kernel runs instead; -1 = never: staged pass + redo kernel),
 * "segments" (a table whose survivors sit in a few long STRETCHES -- sorted on the predicate's column: the first call's sample shows its
 * 1024 blocks in table order -- is cut at those edges and filtered stretch by stretch, each with the kernel its own density asks for, all
 * into one set of outputs; 8-byte value columns, queries of one pass.  0 = tables of 2^28 rows and more in which the sample shows two
 * to four such stretches (a stretch more costs a launch and a read-back: below that one pass is ahead); k > 0 = from k rows on; -1 = never.
 * Same rows in the same order either way),
 * "str_tiles_from" (String columns of a filter are copied tile by tile of 512 SOURCE rows, without the survivors' (start, length)
 * lists, when the pass expects at least this share of the rows to survive: 0 = from 50 %, k > 1 = from k %, 1 = always, -1 = never),
 * "groups_by_ranges" (plain 8-byte columns can be compacted AFTER the pass at its wave offsets, by a kernel without a chain between
 * its waves: 0 = the column groups beyond the first four of a wide projection while up to 55 % of the rows survive, and every plain
 * column the predicate does not read when the predicate kept at most a quarter of the rows the last time -- a nullable one at
 * every selectivity; 1 = always; -1 = never),
 * "speculative_batches" (rv_filter_project_batches launches the pass of a window that looks regular before its handles are
 * validated and validates meanwhile: 0 = from 4096 batches on, -1 = never), "wgs_per_cu" (0 = occupancy query),
 * "grid_limit" (tests: a staged pass launches at most k worker workgroups next to its scanner workgroup, so that a small table makes one
 * workgroup walk many tiles; 0 = as many as the device keeps resident.  Tiles are handed out by a ticket counter: a speed matter only),
 * "agg_grid" (rv_filter_agg: workgroups per CU striding over the tiles; 0 = 8192 workgroups whatever the CU count, -1 = one workgroup per tile),
 * "profile_kernels" (0/1), "out_sizing" (capacity of the output buffers: 0, the default = a table of 2^25 rows and more gets outputs
 * for what its predicate is known to keep -- its last pass over these buffers, or the first call's sample -- x 1.2 + 2 % of the rows,
 * smaller tables and unknown predicates outputs for every row; -1 = every row may survive, always: 2x the input in HBM;
 * 1 = the context's last observed selectivity x 1.5 + 1 %; k >= 2 = a caller-given bound of k rows per
 * million.  A launch whose survivors do not fit still counts exactly and is re-run once with outputs of the exact size, so
 * the bound is a hint, never a correctness matter), "bools_in_pass" (1: projected Boolean columns are compacted inside the fused pass instead
 * of by the bit-compaction kernel after it; measured slower, kept selectable), "narrow_codes" (narrow companions of resident Int64
 * columns: a values buffer of 2^25 elements and more that the lean one-column filter pass -- one compare term, no null bitmap -- has
 * read from end to end twice gets frame-of-reference codes, code = value - column minimum in 2 bytes, or 4 when the value range needs
 * them, and the lean passes after that, over the column or any slice of it that starts at an even element, read the codes instead of
 * the 8-byte values; same rows, same order, same bits.  MEMORY: + 25 % of the column for 2-byte codes, + 50 % for 4-byte codes, held
 * until the column's buffer is freed; a range of 2^32 and more, or no memory for the codes, means no companion and never a failed
 * query.  Only buffers the library allocated qualify -- columns are immutable once their handle is out; rv_wrap memory is the caller's
 * to write and is never packed.  A column whose value range is 1023 and less, and whose triggering scan was a launch over the whole
 * column -- no per-batch counts, first element a multiple of 384 -- gets its codes PACKED instead: 10 bits each, six per 8-byte word,
 * + 16.7 % of the column; launches without per-batch counts over views that start at a multiple of 384 read them, every other launch
 * over the buffer reads the 8-byte values, and when such launches complete two whole scans of their own the 2-byte codes are built
 * beside the packed ones (+ 25 % more; likewise the packed ones beside 2-byte codes that whole-column launches cannot read).
 * 0 = as described, -1 = never, 1 = at the first whole scan whatever the size and never the packed layout (tests), 2 = at the first
 * whole scan whatever the size, packed where the rule above allows, else as 1 (tests, tools/narrow_stamp.py) -- and only with 1 or 2
 * does a launch with a
 * forced "rows_per_lane" geometry or the "stamp" / "debug" diagnostics read the codes, and only where exactly that instantiation exists
 * over codes (the forced geometry; for the diagnostics 2-byte codes at 32 or 16 rows per lane, packed codes at 48 or 24): every other
 * such launch reads the 8-byte values at the geometry asked for, a 4-byte companion under the diagnostics included; read-only
 * counters "narrow_builds", "narrow_passes", "narrow_bytes").  Diagnostics only, never for results: "stamp" (per-phase cycle
 * counters, printed to stderr) and "debug" (bit 0 skip the value stores, bit 1 skip the
 * output-offset lookup -- both make the output WRONG, timing shares only -- bit 2 print
 * scanner / fallback look-back counts, bit 3 run without the scanner wave: results stay correct, bit 4 fault injection: tile 1 never
 * publishes its count, so the bounded waits behind it give up and the call returns RV_ERR_DEVICE) select the separate FF_STAMP
 * instantiations of the kernel, which exist for three shapes; the production instantiations contain none of it.  "spin_limit": polls a
 * wait for another workgroup's descriptor may take before it gives up (0 = default, 4 Mi polls = seconds).
 * "inject_failure" = k: the next k query calls on this context (rv_filter_project*, rv_filter_agg) return RV_ERR_DEVICE
 * before anything is launched -- fault injection for the failure handling of rv_group_* (tests/test_group_gpu.py).
 * "bool_cap" = k > 0: Boolean columns compacted behind the pass get output bitmaps of at most k rows (they are sized for the expected
 * survivors + 25 %; more survivors than that and the column takes the scan path after the pass: this forces that fallback in tests).
 * "csv_slow_cap" = k > 0: a CSV chunk's first list of Float64 cells left to the exact slow kernel holds at most k cells (default:
 * rows x Float64 columns, at most 2^20); more such cells and the chunk is parsed again with a list of the exact size (forces
 * that path in tests).
 * "agg_max_groups" = k > 0: rv_hash_aggregate / rv_group_ids refuse more than k groups (0: the default, 2^26) and size the group
 * table by min(rows, k); "agg_hash_bits" = b (tests): the key hash of group tables truncated to b low bits (see rv_hash_aggregate).
 * "sort_engine": 0, the default = rv_sort_indices runs its own radix passes; 1 (measurements and tests, never chosen by the library) = the
 * pair sort goes through rocprim::radix_sort_pairs over all 64 bits, everything around it unchanged (see rv_sort_indices).  The read-only
 * "sort_last_passes" is the number of scatter passes the last sort call of the context ran.
 * "top_k_select_from_rows" = k > 0 (tests): rv_top_k_indices / rv_top_k run their radix select from k rows on (0: the built-in
 * crossover); "top_k_refine_divisor" = d > 0 (tests): the select takes one more pass while its candidates number more than rows / d
 * (0: the built-in 32).  The read-only "top_k_last_passes" is the number of passes over the key column the select of the last top-k
 * call ran (0: it sorted the whole column), "top_k_last_candidates" the rows that call sorted (see rv_top_k_indices). */
rv_status rv_ctx_set_option(rv_ctx *ctx, const char *key, int64_t value);
/* current value of an option, or of the read-only counters "overflow_reruns" (launches re-run because speculatively sized
 * outputs were too small), "last_selectivity_ppm" (survivors per million rows of the last fused launch, -1: none yet),
 * "last_redo_ppm" (wave ranges -- 64 x rows-per-lane rows -- per million of that launch whose survivors did not fit the wave's LDS slot and were re-read by the redo kernel) and
 * "batch_counts_in_pass" (rv_filter_project_chunked / _batches calls whose per-batch survivor counts came out of the fused
 * pass itself rather than from a second read of the selection bitmap), "fused_rows_scanned" (input rows of every fused
 * filter launch of the context so far: what a pushed-down Limit keeps small), "samples_taken" (selectivity samples so far),
 * "speculative_batch_passes", "last_rows_in" / "last_rows_out" (rows / survivors of the last fused pass), "hbm_free_bytes"
 * (what the device reports free right now), "segmented_passes" (queries that ran stretch by stretch, option "segments") and
 * "segment_fallbacks" (... that started so and ran as one pass after all: more survivors than the sample's profile promised),
 * "csv_slow_cells" (Float64 cells of CSV scans on this context that only the exact slow kernel could round) and
 * "csv_slow_reparses" (CSV chunks parsed a second time because those cells outgrew the first list). */
rv_status rv_ctx_get_option(rv_ctx *ctx, const char *key, int64_t *value);

/* Device time of the hot-path kernel launches (fused filter+compact, filter+aggregate)
 * since the last reset, measured with HIP events recorded on the context stream directly
 * around each launch.  Collected only while option "profile_kernels" is 1. */
rv_status rv_ctx_kernel_stats(rv_ctx *ctx, double *total_ms, uint64_t *launches, int reset);

/* The hot-path kernel instantiation the context launched last, spelled as rocprofv3 prints it without the spaces
 * ("fused_filter_compact<1,16,2,16,32>", "filter_agg_kernel<1,16,2,4,0>"; "" before the first launch): what a bench
 * line's roofline.kernel names, and the key under which profiles/traffic.json holds that kernel's PMC traffic. */
rv_status rv_ctx_last_kernel(rv_ctx *ctx, char *name, size_t name_len);

/* HIP-event timer on the context stream (bench harness; hipEventRecord both ends). */
rv_status rv_timer_start(rv_ctx *ctx);
rv_status rv_timer_stop(rv_ctx *ctx, float *elapsed_ms);

/* ---- arrays: PrimitiveArray / BooleanArray (a1-a3) ---------------------- */
/* copy a host array to the device; offset is preserved (the buffers are copied from
 * element 0 up to offset+length, like the Arc<[T]> an array slice shares). */
rv_status rv_upload(rv_ctx *ctx, const rv_column *host, rv_dcolumn **out);
/* adopt caller-owned device memory (no copy, not freed by rv_free). */
rv_status rv_wrap(rv_ctx *ctx, const rv_column *device, rv_dcolumn **out);
rv_status rv_generate(rv_ctx *ctx, const rv_synth_spec *spec, rv_dcolumn **out);
rv_status rv_free(rv_ctx *ctx, rv_dcolumn *col);
/* Array::slice, zero-copy (primitive.rs:107-117, boolean.rs:208-219). */
rv_status rv_slice(rv_ctx *ctx, const rv_dcolumn *col, uint64_t offset, uint64_t length,
                   rv_dcolumn **out);
rv_status rv_column_info_get(rv_ctx *ctx, const rv_dcolumn *col, rv_column_info *out);
/* Array::null_count (primitive.rs:90-105): popcount of the validity range on device. */
rv_status rv_null_count(rv_ctx *ctx, const rv_dcolumn *col, uint64_t *out);
/* Download the logical range [0,length).  values: length*8 bytes (RV_INT64/RV_FLOAT64) or
 * ceil(length/8) bytes (RV_BOOLEAN), re-based to offset 0, tail bits zero.  validity:
 * ceil(length/8) bytes, may be NULL; *has_validity tells whether the array carries one. */
rv_status rv_download(rv_ctx *ctx, const rv_dcolumn *col, void *values, uint8_t *validity,
                      int *has_validity);
/* raw device pointers of a device column (interop; valid until rv_free). */
rv_status rv_device_ptrs(rv_ctx *ctx, const rv_dcolumn *col, rv_column *out);

/* StringArray (string.rs:8-147): download of the logical elements.  offsets receives length + 1
 * entries starting at 0, data rv_column_info.data_bytes bytes. */
rv_status rv_download_string(rv_ctx *ctx, const rv_dcolumn *col, int32_t *offsets, uint8_t *data,
                             uint8_t *validity, int *has_validity);

/* dataframe_to_batches' treatment of nulls (streaming.rs:135-233): the null cells of an Int64 / Float64 /
 * Boolean array become 0 / 0.0 / false and the array loses its bitmap; String arrays keep their nulls (a
 * shared view is returned), so does an array without a bitmap. */
rv_status rv_fill_nulls(rv_ctx *ctx, const rv_dcolumn *col, rv_dcolumn **out);

/* ---- predicate evaluation (K1) ------------------------------------------ */
/* AND-of-compares over cols -> selection BooleanArray without validity: bit i == 1 iff
 * row i survives RecordBatch::filter under pred->nulls.  *out_count = survivors.
 * Replaces the eager mask loop (plan.rs:112-130) and the index scan
 * (record_batch.rs:235-240). */
rv_status rv_eval_predicate(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols,
                            const rv_predicate *pred, rv_dcolumn **out_selection,
                            uint64_t *out_count);
/* One compare term as a nullable BooleanArray: value = cell <op> literal, null where the
 * cell is null (the composition rule of SURVEY.md section 8c for streaming compares). */
rv_status rv_compare(rv_ctx *ctx, const rv_dcolumn *col, rv_cmp op, rv_dtype lit_type,
                     int64_t lit_i, double lit_f, rv_dcolumn **out_bool);
/* The same with the literal given as a term (term->column is ignored): the form that takes String literals
 * (`name == "Bob"` over a StringArray column, byte-wise str ordering). */
rv_status rv_compare_term(rv_ctx *ctx, const rv_dcolumn *col, const rv_term *term, rv_dcolumn **out_bool);

/* ---- arithmetic expressions (K8) ------------------------------------------ */
/* Expr::add / sub / mul / div (BinaryOperator::{Plus, Minus, Multiply, Divide}, expr.rs:17-20, 44-74) over Int64 / Float64 columns
 * and literals.  The reference types and names such an expression (logical_plan/plan.rs:204-262) and refuses it at planning
 * (planner.rs:124-126, :151-156), so the cell rules are this library's:
 *   - result dtype, bottom-up as infer_binary_result_type: Float64 on either side -> Float64; Int64 o Int64 -> Int64 (Divide
 *     included); Null o T -> T; Null o Null -> Null; a Boolean / String operand is RV_ERR_TYPE_MISMATCH;
 *   - a null operand makes the cell null and its slot holds the placeholder 0 / 0.0; a Null leaf (an RV_NULL column, a literal of
 *     lit_type RV_NULL) makes EVERY cell null: decided on the host, no kernel runs;
 *   - Int64: + - * wrap in two's complement, / truncates toward zero, x / 0 is null, INT64_MIN / -1 is INT64_MIN;
 *   - an Int64 operand that meets a Float64 is converted first, round to nearest even;
 *   - Float64: one correctly rounded IEEE-754 operation per operator (no fused multiply-add; x / 0.0 is +-inf or NaN, not null;
 *     subnormals are kept; a NaN stays a NaN, its payload is not specified).
 * steps[0 .. n_steps) is the expression in postfix order: RV_ARITH_COL pushes cols[column], RV_ARITH_LIT pushes the literal
 * (lit_type RV_INT64: lit.i, RV_FLOAT64: lit.f, RV_NULL: a null), the four operators pop two values and push one.  The program
 * must leave exactly one value and read at least one column.  Limits: 32 steps, an operand stack of 8, 8 distinct columns.
 * *out: a new column of the common length of the columns read, offset 0, null_count known; it carries a validity bitmap iff a
 * column read carries one or the program has an Int64 division (or every cell is null).
 * Errors (the context stays usable, nothing is created): NULL arguments, a malformed program (an operator with fewer than two
 * operands, more than one value left, no column read, an unknown step) or a column index >= ncols: RV_ERR_INVALID_ARG; columns read
 * of unequal length: RV_ERR_LENGTH_MISMATCH; a Boolean / String column or literal: RV_ERR_TYPE_MISMATCH; over a limit:
 * RV_ERR_UNSUPPORTED.  rv_ctx_last_kernel: arith_kernel<2> / <4> / <8> (the larger of the operand stack and the columns read), arith_all_null when
 * every cell is null, arith_empty for zero rows -- neither of the two launches anything. */
typedef enum rv_arith_op { RV_ARITH_COL = 0, RV_ARITH_LIT = 1, RV_ARITH_ADD = 2, RV_ARITH_SUB = 3, RV_ARITH_MUL = 4, RV_ARITH_DIV = 5 } rv_arith_op;
typedef struct rv_arith_step {
    rv_arith_op op;
    uint32_t column;   /* RV_ARITH_COL: index into the cols[] array handed to the call */
    rv_dtype lit_type; /* RV_ARITH_LIT */
    union {
        int64_t i;
        double f;
    } lit;
} rv_arith_step;
rv_status rv_eval_arith(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols,
                        const rv_arith_step *steps, uint32_t n_steps, rv_dcolumn **out);

/* ---- BooleanArray logic (K3, boolean.rs:120-180) -------------------------- */
rv_status rv_boolean_and(rv_ctx *ctx, const rv_dcolumn *a, const rv_dcolumn *b, rv_dcolumn **out);
rv_status rv_boolean_or(rv_ctx *ctx, const rv_dcolumn *a, const rv_dcolumn *b, rv_dcolumn **out);
rv_status rv_boolean_not(rv_ctx *ctx, const rv_dcolumn *a, rv_dcolumn **out);
rv_status rv_boolean_count(rv_ctx *ctx, const rv_dcolumn *a, uint64_t *count_true,
                           uint64_t *count_false);

/* ---- RecordBatch kernels (S2) -------------------------------------------- */
/* RecordBatch::filter (record_batch.rs:221-243): predicate must be RV_BOOLEAN of the
 * batch length; rows with Some(true) are kept in ascending order; every column goes
 * through take_array semantics (null slots -> 0 / 0.0 / false, validity dropped when no
 * null survives, output offset 0).  out[] receives ncols new handles. */
rv_status rv_filter(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols,
                    const rv_dcolumn *predicate, rv_dcolumn **out, uint64_t *out_rows);
/* RecordBatch::take (record_batch.rs:108-178): arbitrary host index list. */
rv_status rv_take(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols,
                  const uint64_t *indices, uint64_t n_indices, rv_dcolumn **out);
/* The same with the index list resident on the device (an Int64 array without nulls): a selection -> indices -> take
 * chain never leaves HBM.  The bounds pre-pass (record_batch.rs:109-116) is a device reduction that finds the FIRST
 * offending position, so the error text is the reference's ("Index 7 out of bounds for 5 rows"). */
rv_status rv_take_device(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const rv_dcolumn *indices,
                         rv_dcolumn **out);
/* rv_take_device with a NULLABLE index list: a null index yields a null cell of the column's dtype -- value 0 / false /
 * the empty string, validity attached (to the outputs that got a null cell) -- whatever lies under the null.  Non-null
 * indices are bounds-checked with the same text as rv_take_device.  RV_NULL columns stay RV_NULL; String and Boolean
 * columns are included.  An index list without nulls gives exactly rv_take_device's outputs.  The outer joins gather
 * the side that can lack a partner through this (rv_join_probe_kind's index columns are what it takes). */
rv_status rv_take_device_nullable(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const rv_dcolumn *indices,
                                  rv_dcolumn **out);
/* The ascending index list RecordBatch::filter builds from its predicate (record_batch.rs:235-240): the rows of a
 * BooleanArray that are Some(true), as an Int64 device array. */
rv_status rv_selection_indices(rv_ctx *ctx, const rv_dcolumn *selection, rv_dcolumn **out_indices);
/* concat_arrays (record_batch.rs:277-342) for one column position across batches. */
rv_status rv_concat(rv_ctx *ctx, const rv_dcolumn *const *parts, uint32_t nparts,
                    rv_dcolumn **out);

/* ---- inner hash join (PhysicalPlan::HashJoin) ----------------------------- */
/* PhysicalPlan::HashJoin with JoinType::Inner (src/physical_plan/plan.rs:174-284; planned by planner.rs:90-110, reached
 * through LazyFrame::inner_join, builder.rs:85-95).  The left frame is the BUILD side, the right frame the PROBE side
 * (planner.rs:102-108).
 *
 * Key equality is AnyValue's Hash + PartialEq (src/datatypes/series.rs:72-98), not SQL's:
 *   - Null == Null: a null probe key matches every null build key; an RV_NULL key column is all nulls;
 *   - Int64 and Boolean keys match on equal values;
 *   - Float64 keys match when their bits are equal and the value is not NaN.  NaN never matches, not even the same bits
 *     (PartialEq fails).  +0.0 and -0.0 do NOT match: they hash apart (to_bits), and the reference could pair them only
 *     on a random SipHash bucket-and-tag collision;
 *   - key columns of different dtypes (Int64 against Float64: is_comparable_with allows it, series.rs:144-156) match
 *     null to null only: values of different AnyValue variants never compare equal;
 *   - String keys go through the string dictionary (below): rv_string_dict_build / _encode reduce them to Int64 ids
 *     first.  A raw String key column handed to the calls of this section is RV_ERR_UNSUPPORTED (String PAYLOAD
 *     columns are fine).
 * Pairs come in probe-row order and, within a probe row, in ascending build-row order -- the reference's result_pairs
 * (plan.rs:196-204; the Vec push order of its HashMap<AnyValue, Vec<usize>>) -- identically on every run: output
 * positions come from scans of match counts, never from the order atomics land in.
 *
 * A failed call leaves the context usable and creates no outputs. */
typedef struct rv_join_table rv_join_table;  /* a build side hashed on the device; probed by any number of key columns */
/* The reference's HashMap build (plan.rs:183-192) over one key column (a slice is fine).  Build sides of 2^32 rows or
 * more: RV_ERR_UNSUPPORTED (32-bit build row ids inside).  Context option "join_hash_bits" = b (tests) hashes the
 * keys of tables built afterwards to b low bits: long collision chains on small inputs. */
rv_status rv_join_build(rv_ctx *ctx, const rv_dcolumn *build_key, rv_join_table **out);
/* The probe loop (plan.rs:194-204): out_probe_idx / out_build_idx receive the `result_pairs` as two Int64 device
 * arrays without nulls, row indices into the probe key column and the build key column as given (offsets of slices
 * excluded) -- what rv_take_device takes as they are.  The pair count is known on the device before anything is
 * allocated: a count whose two outputs the device cannot hold is RV_ERR_OOM, and the context still works.  A key
 * column of another dtype than the table's matches null to null only (see above).  rv_ctx_last_kernel names the
 * probe kernel that wrote the pairs: join_probe_emit<0> (every list one row: unique build keys),
 * join_probe_emit<1> (lists written lane by lane), join_probe_emit<2> (lists longer than a lane takes, written by
 * a whole workgroup); join_probe_count when no pair came out. */
rv_status rv_join_probe(rv_ctx *ctx, const rv_join_table *table, const rv_dcolumn *probe_key,
                        rv_dcolumn **out_probe_idx, rv_dcolumn **out_build_idx, uint64_t *out_rows);
/* Build rows, hash slots and the longest match list of a table (any pointer may be NULL). */
rv_status rv_join_table_info(const rv_join_table *table, uint64_t *build_rows, uint64_t *slots, uint64_t *longest_list);
rv_status rv_join_table_free(rv_ctx *ctx, rv_join_table *table);
/* The whole operator in one call: build + probe + gather (materialize_join_result, plan.rs:212-255).  out[] receives
 * n_probe + n_build - 1 columns in the reference's order: every probe column, then every build column except
 * build_cols[build_key] (names, and the `_right` suffix of a build column whose name the probe side also has, live in
 * the caller).  Gathered cells keep their nulls; zero pairs give zero-row columns of the same dtypes
 * (create_empty_join_result, plan.rs:257-284).  Errors: a key index out of range RV_ERR_INVALID_ARG, columns of one
 * side of unequal length RV_ERR_LENGTH_MISMATCH, plus those of rv_join_build / rv_join_probe. */
rv_status rv_hash_join(rv_ctx *ctx, const rv_dcolumn *const *build_cols, uint32_t n_build, uint32_t build_key,
                       const rv_dcolumn *const *probe_cols, uint32_t n_probe, uint32_t probe_key,
                       rv_dcolumn **out, uint64_t *out_rows);
/* The streaming inner join's probe over one WINDOW of a resident probe frame (StreamingPhysicalPlan::HashJoin, which the
 * reference leaves todo!(), streaming.rs:128-131, defined by the eager join): the probe frame is cut into BATCHES the way
 * rv_filter_project_chunked cuts a table -- batch k is probe rows [k * chunk_rows, min((k + 1) * chunk_rows, length)), there
 * are K = ceil(length / chunk_rows) of them, none for an empty frame -- and output batch k == rv_hash_join of the whole build
 * side against probe batch k alone (same key rules, same names, same row order).  `table` is rv_join_build over
 * build_cols[build_key]; build_cols are the columns it gathers from.
 *   - out[n_probe + n_build - 1] hold the output batches back to back, in the column order of rv_hash_join; output batch k
 *     is rows [sum(out_rows[0..k)), + out_rows[k]) of every out[j] -- rv_slice_known cuts it out without copying;
 *   - out_rows[K] (capacity `nchunks`): the pairs of EVERY batch, all K, from one count pass and one read-back;
 *   - out_nulls[K x nout] (may be NULL): null count of every materialised output batch and column;
 *   - *out_total (may be NULL): the pairs materialised, sum(out_rows[0 .. *out_batches)).
 * `max_pairs` bounds the window's output: only the longest prefix of batches whose pairs fit max_pairs AND what the device
 * holds (16 bytes of indices per pair, as rv_join_probe) is materialised, and *out_batches reports its batch count.  At least
 * one batch is always taken; only a single batch the device cannot hold is RV_ERR_OOM, with nothing allocated.  max_pairs = 0:
 * the device limit only.  The caller continues with the probe rows from *out_batches x chunk_rows on.
 * Errors: chunk_rows 0, nchunks below K, a key index out of range: RV_ERR_INVALID_ARG; a build column whose length differs
 * from the table's build rows, or unequal columns on one side: RV_ERR_LENGTH_MISMATCH; anything else as rv_hash_join.  A failed
 * call leaves the context usable and creates no outputs.  rv_ctx_last_kernel names the emit kernel as rv_join_probe does, or
 * join_probe_count_batched when no pair came out. */
rv_status rv_hash_join_chunked(rv_ctx *ctx, const rv_join_table *table,
                               const rv_dcolumn *const *build_cols, uint32_t n_build, uint32_t build_key,
                               const rv_dcolumn *const *probe_cols, uint32_t n_probe, uint32_t probe_key,
                               uint64_t chunk_rows, uint64_t max_pairs,
                               rv_dcolumn **out, uint64_t *out_rows, uint64_t nchunks, int64_t *out_nulls,
                               uint64_t *out_total, uint64_t *out_batches);

/* ---- outer, semi and anti hash joins --------------------------------------- */
/* The other kinds of the join above (the reference's enum stops at Inner: logical_plan/plan.rs has //Left, //Outer).
 * Build side and probe side are as in rv_hash_join; key equality is unchanged (AnyValue's, see above), hence:
 *   - a NaN probe key is always unmatched: PROBE_OUTER keeps it with a null partner, PROBE_ANTI keeps it, PROBE_SEMI
 *     drops it;
 *   - a null probe key is matched if and only if the build key has a null: PROBE_ANTI is NOT SQL's NOT IN;
 *   - a NaN build row is never met: FULL_OUTER always emits it as unmatched;
 *   - key columns of different dtypes meet null to null only, so every non-null probe row is unmatched.
 * Row order is fully determined and identical run to run (positions come from scans, never from the order atomics
 * land in):
 *   - INNER / PROBE_OUTER: probe-row order; within a probe row ascending build row; an unmatched probe row
 *     contributes one pair (p, none) at its place;
 *   - FULL_OUTER: the PROBE_OUTER rows, then one pair (none, b) per unmatched build row, ascending b;
 *   - PROBE_SEMI / PROBE_ANTI: ascending probe row, each row once. */
typedef enum rv_join_kind {
    RV_JOIN_INNER = 0,       /* exactly rv_join_probe / rv_hash_join */
    RV_JOIN_PROBE_OUTER = 1, /* every probe row at least once; a probe row without a match pairs with "no build row" */
    RV_JOIN_FULL_OUTER = 2,  /* PROBE_OUTER, then every build row no probe row met */
    RV_JOIN_PROBE_SEMI = 3,  /* the probe rows that have at least one match, once each, probe columns only */
    RV_JOIN_PROBE_ANTI = 4   /* the probe rows that have none, probe columns only */
} rv_join_kind;
/* (the calls below take the kind as `int kind`, one of the values above, as the other calls of this header take their enums) */
/* rv_join_probe for any kind.  The index columns are Int64; a cell with no partner is a NULL cell: validity attached
 * only when some cell is null, null_count known, value 0 under a null -- what rv_take_device_nullable takes.
 * PROBE_SEMI / PROBE_ANTI set *out_build_idx = NULL.  kind == RV_JOIN_INNER gives exactly rv_join_probe's output.  The
 * row total, unmatched rows included, is known on the device before any output is allocated (a FULL_OUTER probe holds
 * its scratch by then: a bit per hash slot and two bits per build row): more than the device holds
 * is RV_ERR_OOM with the context still usable.  An unknown kind: RV_ERR_INVALID_ARG.  `table` is not changed: the
 * record of the build rows a FULL_OUTER probe met lives in the call.
 * rv_ctx_last_kernel: the inner names for RV_JOIN_INNER; otherwise the emit kernel with the kind appended --
 *   PROBE_OUTER  join_probe_emit<0,outer>  join_probe_emit<1,outer>  join_probe_emit<2,outer>
 *   FULL_OUTER   join_probe_emit<0,full>   join_probe_emit<1,full>   join_probe_emit<2,full>
 *   PROBE_SEMI   join_probe_emit<0,semi>   PROBE_ANTI   join_probe_emit<0,anti>
 * (0 / 1 / 2 by the longest list as for the inner join; semi and anti joins are always the compaction, 0) -- and
 * join_probe_count when the emit pass had no row to write. */
rv_status rv_join_probe_kind(rv_ctx *ctx, const rv_join_table *table, const rv_dcolumn *probe_key, int kind,
                             rv_dcolumn **out_probe_idx, rv_dcolumn **out_build_idx, uint64_t *out_rows);
/* rv_hash_join for any kind.  Output columns:
 *   - INNER, PROBE_OUTER: every probe column, then every build column but the key: n_probe + n_build - 1;
 *   - FULL_OUTER: every probe column, then EVERY build column, the key included, at its place: n_probe + n_build (a
 *     row without a probe partner would otherwise lose its key);
 *   - PROBE_SEMI, PROBE_ANTI: the probe columns only: n_probe.
 * A cell of the side without a partner is null.  Zero rows give zero-row columns of the right dtypes.  Errors as
 * rv_hash_join. */
rv_status rv_hash_join_kind(rv_ctx *ctx, const rv_dcolumn *const *build_cols, uint32_t n_build, uint32_t build_key,
                            const rv_dcolumn *const *probe_cols, uint32_t n_probe, uint32_t probe_key,
                            int kind, rv_dcolumn **out, uint64_t *out_rows);
/* rv_hash_join_chunked for the probe-preserving kinds INNER, PROBE_OUTER, PROBE_SEMI and PROBE_ANTI; FULL_OUTER is
 * RV_ERR_UNSUPPORTED (its unmatched build rows belong to no probe batch).  The contract is unchanged: output batch k ==
 * rv_hash_join_kind of the whole build side against probe batch k alone; all K batch counts come from one count pass
 * and one read-back; max_pairs cuts a prefix of batches.  out[] holds the kind's columns (see rv_hash_join_kind);
 * rv_ctx_last_kernel as rv_join_probe_kind, or join_probe_count_batched when no row came out. */
rv_status rv_hash_join_chunked_kind(rv_ctx *ctx, const rv_join_table *table,
                                    const rv_dcolumn *const *build_cols, uint32_t n_build, uint32_t build_key,
                                    const rv_dcolumn *const *probe_cols, uint32_t n_probe, uint32_t probe_key,
                                    int kind, uint64_t chunk_rows, uint64_t max_pairs,
                                    rv_dcolumn **out, uint64_t *out_rows, uint64_t nchunks, int64_t *out_nulls,
                                    uint64_t *out_total, uint64_t *out_batches);

/* ---- string dictionary (String join keys) --------------------------------- */
/* The join kernels take 64 key bits per cell.  A String key column gets there through a DICTIONARY: the distinct
 * non-null strings of one column, each named by an Int64 id, built once on the device; any number of String columns
 * are then ENCODED against it into Int64 id columns, and the Int64 join runs on the ids unchanged.
 *
 * The id of a string is the row index (slice offset excluded) of its FIRST occurrence in the column the dictionary
 * was built from.  An ids column is an RV_INT64 column of the length of `col`, offset 0:
 *   - a null cell is null: the validity is re-based to bit 0, absent when `col` has no nulls, null_count is known;
 *   - a valid cell whose bytes occur in the dictionary gets that string's id;
 *   - a valid cell whose bytes do not occur gets -1.
 * Equality is byte equality of the cell (AnyValue::String's PartialEq / Hash, src/datatypes/series.rs:72-98): "" is
 * a value and not null, embedded NUL bytes count, nothing is normalised.  The result is EXACT -- a hash decides where
 * to look, never whether two strings are equal: every hit is confirmed against the bytes -- and identical on every
 * run: an id is the minimum row, whatever order the atomics land in.
 *
 * Join property (the reason for the id convention): for String key columns B (build) and P (probe), with ids_B from
 * rv_string_dict_build(B) and ids_P = rv_string_dict_encode(dict, P), rv_join_build(ids_B) + rv_join_probe(ids_P)
 * yield exactly the reference's result_pairs for B and P: equal strings meet, null meets null, and an absent string
 * meets nothing because every build id is >= 0.
 *
 * An RV_NULL column is accepted by both calls: all-null ids, an empty dictionary.  Errors leave the context usable
 * and create nothing: a column of any other dtype RV_ERR_TYPE_MISMATCH, NULL arguments RV_ERR_INVALID_ARG, columns
 * of 2^32 rows or more RV_ERR_UNSUPPORTED (the join's own limit).  Context option "string_hash_bits" = b (tests; 0 =
 * all 64) truncates the string hash of dictionaries built afterwards to b low bits: long collision chains on small
 * inputs, the twin of "join_hash_bits". */
typedef struct rv_string_dict rv_string_dict;  /* the distinct strings of a column; encodes any number of columns */
/* Distinct non-null strings of a String column (a slice is fine).  The dictionary shares the column's buffers the way
 * rv_slice does and keeps them alive: freeing the column handle after the build is allowed.  out_ids (may be NULL)
 * receives rv_string_dict_encode(dict, col).  rv_ctx_last_kernel: str_dict_insert, or str_dict_encode with out_ids. */
rv_status rv_string_dict_build(rv_ctx *ctx, const rv_dcolumn *col, rv_string_dict **out, rv_dcolumn **out_ids);
/* The ids of a String (or RV_NULL) column against a dictionary, as described above. */
rv_status rv_string_dict_encode(rv_ctx *ctx, const rv_string_dict *dict, const rv_dcolumn *col, rv_dcolumn **out_ids);
/* Rows of the source column, distinct strings, and hash slots (a power of two, at least twice the non-null rows) of a
 * dictionary (any pointer may be NULL). */
rv_status rv_string_dict_info(const rv_string_dict *dict, uint64_t *rows, uint64_t *distinct, uint64_t *slots);
rv_status rv_string_dict_free(rv_ctx *ctx, rv_string_dict *dict);

/* ---- fused filter + project (K1+K2, the hot path) ------------------------- */
/* == SelectStream(FilterStream(input)) on one batch (stream.rs:136-158, :202-210) and
 * == PhysicalPlan::Filter followed by Select (plan.rs:97-150, :68-96): evaluate pred
 * over cols, keep surviving rows of the projected columns proj[0..nproj) in ascending
 * row order.  Single pass over HBM.  out[] receives nproj handles; if out_selection is
 * non-NULL the selection bitmap is materialised as well. */
rv_status rv_filter_project(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols,
                            const rv_predicate *pred, const uint32_t *proj, uint32_t nproj,
                            rv_dcolumn **out, uint64_t *out_rows, rv_dcolumn **out_selection);

/* The same in two halves, for a streaming operator that keeps the device busy: begin queues the launch of
 * batch k+1 and returns; finish of batch k (row count, output lengths, null counts) is called afterwards,
 * so the host work and the result read-back of one batch overlap the kernel of the next.  Launches finish
 * in the order they began.  Shapes that need several passes (String columns, more columns than one pass
 * takes) are completed inside begin.  The input columns must stay alive until finish; finish consumes the
 * pending handle (also on error). */
rv_status rv_filter_project_begin(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols,
                                  const rv_predicate *pred, const uint32_t *proj, uint32_t nproj,
                                  rv_pending **out_pending);
rv_status rv_filter_project_finish(rv_ctx *ctx, rv_pending *pending, rv_dcolumn **out, uint64_t *out_rows);

/* Seam S1 at the reference's batch size.  The reference streams 1024-row RecordBatches (streaming_planner.rs:32); one
 * launch per such batch costs ~30 us of fixed launch / read-back time for ~10 ns of work.  This call takes K
 * device-resident input batches of one schema (cols[b * ncols + c] = column c of batch b) and runs
 * SelectStream(FilterStream(batch)) (stream.rs:136-158, :202-210) on ALL of them in one pass:
 *   - batches that are adjacent zero-copy slices of the same buffers (RecordBatch::slice, dataframe_to_batches:
 *     streaming.rs:135-233) are read as they lie in HBM, as one batch; separately allocated batches are joined by one
 *     device concat first;
 *   - out[j] (nproj handles) holds the K output batches back to back, in batch order; output batch b is the rows
 *     [sum(out_rows[0..b)), + out_rows[b]) of every out[j] -- rv_slice_known cuts it out without copying;
 *   - out_rows[K]: surviving rows per batch (ONE read-back for all K); out_nulls[K * nproj] (may be NULL): null count
 *     of every output batch and column, so that a slice drops its bitmap exactly where the reference's builder would
 *     (primitive.rs:179-185); *out_total: all survivors.
 * Result == rv_filter_project on every batch on its own.  A window of 4096 batches and more that looks regular from its first and
 * last batch (adjacent zero-copy slices of one length) is filtered on that assumption WHILE its K x ncols handles are validated; what
 * the validation rejects is dropped and reported as the first offending batch's error -- after an error the contents of out_rows /
 * out_nulls are unspecified (the speculative pass may have written counts there). */
rv_status rv_filter_project_batches(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t nbatches, uint32_t ncols,
                                    const rv_predicate *pred, const uint32_t *proj, uint32_t nproj, rv_dcolumn **out,
                                    uint64_t *out_rows, int64_t *out_nulls, uint64_t *out_total);
/* The same over ONE resident table cut the way the reference's chunker cuts a DataFrame: StreamingPhysicalPlan::execute
 * on DataFrameSource -> Filter -> Select with batch size `chunk_rows` (dataframe_to_batches, streaming.rs:135-233;
 * default 1024, streaming_planner.rs:32), collected.  Batch k is rows [k * chunk_rows, min((k + 1) * chunk_rows, length));
 * there are ceil(length / chunk_rows) of them (none for an empty table), and the caller passes the capacity of out_rows
 * (and of out_nulls / nproj) in `nchunks`.  No per-batch handles to build or walk and no boundary table to upload: at 1024
 * rows per batch this is what keeps the host side of the call under the device time.  Result == rv_filter_project_batches
 * over rv_slice(cols, k * chunk_rows, ...) for every k.
 * When a batch is a whole number of the pass's wave ranges (64 x rows-per-lane rows: 1024 by default, so the reference's
 * 1024-row batches qualify) the per-batch survivor counts come out of the fused pass itself: no selection bitmap is
 * written or re-read.  If out_rows lies in memory from rv_host_alloc / rv_host_register the device writes the counts
 * there directly (8 bytes per batch cross PCIe once and the host copies nothing); a pageable array is filled from a
 * pinned staging block. */
rv_status rv_filter_project_chunked(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, uint64_t chunk_rows,
                                    const rv_predicate *pred, const uint32_t *proj, uint32_t nproj, rv_dcolumn **out,
                                    uint64_t *out_rows, uint64_t nchunks, int64_t *out_nulls, uint64_t *out_total);
/* Seam S1 with TWO WINDOWS IN FLIGHT (ABI 4).  A stream operator pulls batches one at a time (DataStream::next_batch,
 * stream.rs:25-28) and looks ahead by a window of them; begun before the window in front of it is finished, a window's pass runs
 * while the host reads that window's counts and hands its batches on -- the device never waits for the host between windows.
 *   rv_filter_project_chunked_begin  == rv_filter_project_chunked up to the launch; out_rows (capacity nchunks) is written by the
 *                                       device when it lies in pinned memory (rv_host_alloc / rv_host_register) -- on a side stream,
 *                                       beside the next window's pass -- and is complete when finish returns;
 *   rv_filter_project_batches_begin  == rv_filter_project_batches likewise: the pass is launched on what the window's first and
 *                                       last batch say it is (a regular stream's), and the walk over its K x ncols handles
 *                                       validates that on a helper thread until finish -- which drops the result and takes the
 *                                       ordinary path (or reports the first offending batch) when the walk says otherwise;
 *   rv_filter_project_window_finish  waits, hands over out[nproj], out_nulls[K * nproj] (may be NULL), *out_total; consumes the
 *                                       pending handle (also on error).  Windows finish in the order they began.
 * Queued: shapes of one chained pass whose batches it can count (a batch a whole number of its wave ranges: 1024 rows do) with
 * device-writable out_rows.  Everything else (several passes, String columns, the mask path of a Boolean-column predicate, pageable
 * out_rows) completes inside begin.  cols / pred / proj / out_rows must stay valid until finish. */
rv_status rv_filter_project_chunked_begin(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, uint64_t chunk_rows,
                                          const rv_predicate *pred, const uint32_t *proj, uint32_t nproj, uint64_t *out_rows,
                                          uint64_t nchunks, rv_pending **out_pending);
rv_status rv_filter_project_batches_begin(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t nbatches, uint32_t ncols,
                                          const rv_predicate *pred, const uint32_t *proj, uint32_t nproj, uint64_t *out_rows,
                                          rv_pending **out_pending);
rv_status rv_filter_project_window_finish(rv_ctx *ctx, rv_pending *pending, rv_dcolumn **out, int64_t *out_nulls,
                                          uint64_t *out_total);
/* rv_slice with the null count of the range supplied by the caller (from rv_filter_project_batches): the view drops
 * the bitmap when it is 0 and needs no device pass to answer null_count(). */
rv_status rv_slice_known(rv_ctx *ctx, const rv_dcolumn *col, uint64_t offset, uint64_t length, int64_t null_count,
                         rv_dcolumn **out);

/* ---- host-resident batches: chunked, overlapped upload + filter + project ---- */
/* Pinned host memory for array buffers.  A caller that keeps its Arc<[T]> / Arc<[u8]> backing
 * stores here gets DMA at PCIe rate and truly asynchronous chunk uploads; pageable buffers work
 * too (the copy is then staged by the runtime). */
rv_status rv_host_alloc(rv_ctx *ctx, size_t bytes, void **out);
rv_status rv_host_free(rv_ctx *ctx, void *ptr);
/* StreamingPhysicalPlan::collect() over a host table (streaming.rs:71-133): replaces
 * dataframe_to_batches (:135-233) + the per-batch pull loop + the final concat
 * (collect_stream_batches, :343-352).  The table is cut into chunks of chunk_rows rows
 * (0 = default 32 Mi; rounded up to a multiple of 64); the upload of chunk k+1 runs on a second
 * stream while chunk k is filtered; the per-chunk outputs are concatenated on the device
 * (rv_concat rules: validity kept only if a null survived).  host_cols[i].offset is honoured
 * (primitive.rs:62-64); String columns are cut at element boundaries (offsets rebased per chunk).
 * Result == rv_filter_project on the uploaded whole columns. */
rv_status rv_filter_project_host(rv_ctx *ctx, const rv_column *host_cols, uint32_t ncols,
                                 const rv_predicate *pred, const uint32_t *proj, uint32_t nproj,
                                 uint64_t chunk_rows, rv_dcolumn **out, uint64_t *out_rows);

/* ---- filter + global aggregate (K4) --------------------------------------- */
/* COUNT(*) of surviving rows and SUM(cols[agg_col]) over surviving non-null cells.
 * RV_INT64: two's-complement wrapping sum in *sum_i (order independent => bit exact).
 * RV_FLOAT64: sum in *sum_f, fixed reduction tree.  The order of the additions follows from the row count, from the number
 * of 8-byte columns the launch reads (the aggregated column, the value columns of the predicate and the nullable value columns
 * an OR / NOT expression propagates nulls from: 1 / 2 / 3-4 columns sum 16 / 8 / 4 rows per lane, tiles of 4096 / 2048 / 1024
 * rows; more than 4: the predicate goes through a selection bitmap and the sum is that of 1 column) and from the width of
 * the loads, which sets which rows of a tile a lane holds: 16 bytes when only the aggregated column is read, 8 bytes otherwise
 * (option "vec" overrides), and always 8 bytes when the first row of one of those columns is not 16-byte aligned (an odd-offset
 * slice).  The grid is a constant (8192 workgroups stride over the tiles whatever the device's CU count; option "agg_grid"
 * changes the tree).  So the same call over the same buffers sums to the same bits run to run and part to part, while another
 * predicate shape, another alignment or row-range shards of other sizes add in a different order: there the Float64 result
 * agrees to rounding (tests: 1e-12 relative on uniform data; a derived gamma_k bound on mixed-sign data), and bit for bit
 * whenever every partial sum is exactly representable (tests: test_agg_float_gpu.py, every kernel variant, load width, grid and
 * sharding over cells k * 2^s; NaN / inf under null cells and in dropped rows never reach the sum).  The Int64 result is exact.
 * The reference has no aggregate operator; semantics defined in DESIGN.md. */
rv_status rv_filter_agg(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols,
                        const rv_predicate *pred, uint32_t agg_col, int64_t *sum_i,
                        double *sum_f, uint64_t *count);

/* ---- grouped aggregation (K9) ----------------------------------------------- */
/* group_by(key).agg([a_0 .. a_{m-1}]): one key column, m >= 1 aggregates, each (op, value column).  The reference has
 * no aggregate operator; the semantics are defined here and in DESIGN.md section 4 K9.
 *
 * Groups.  One group per distinct key value; all null keys form ONE group (AnyValue: Null == Null, as in the join).
 * Key dtypes: RV_INT64; RV_NULL (one group when the column has rows).  RV_FLOAT64, RV_BOOLEAN and RV_STRING keys are
 * RV_ERR_UNSUPPORTED -- String keys go through rv_string_dict_build ids (the host layer does that).
 *
 * Order.  The output rows are the groups by ascending FIRST ROW: a group's smallest row index in the key column as
 * given (slice offset excluded).  Positions come from the first rows and a scan, never from the order atomics land in:
 * the same input gives the same output on every run.  An empty key gives zero groups and zero-row outputs of the right
 * dtypes.
 *
 * Aggregates.  RV_AGG_COUNT_ROWS takes no value column and counts the group's rows; RV_AGG_COUNT counts the non-null
 * cells of a value column of any dtype; RV_AGG_SUM / MIN / MAX run over the non-null cells of an RV_INT64 or
 * RV_FLOAT64 value column (any other dtype: RV_ERR_TYPE_MISMATCH).
 *   counts   Int64, no bitmap.
 *   SUM      the value column's dtype, no bitmap; a group without a non-null cell sums to 0 / +0.0 (as rv_filter_agg
 *            over an empty selection).  Int64: wraps in two's complement, order independent, exact.  Float64: NO
 *            floating-point atomics anywhere on the path.  The rows are grouped by a stable sort, each group's rows
 *            ascending, and a group's additions are ordered by the LENGTH L of its row list (null cells included: each
 *            adds +0.0) and every row's POSITION in it, nothing else: L <= 1024: lane l of one wave adds positions l,
 *            l + 64, ... from +0.0, then the xor butterfly 32, 16, .., 1 over the lanes; longer: thread t of 256 adds
 *            positions t, t + 256, ..., the same butterfly per wave, then (w0 + w1) + (w2 + w3); the result is +0.0 +
 *            that sum (never -0.0).  So the same call over the same buffers gives the same bits run to run; the sum is
 *            bit exact whenever every partial sum is representable, and otherwise |got - exact| <= gamma_{n-1} x
 *            sum|x| per group (n = its non-null cells, gamma_k = k u / (1 - k u), u = 2^-53: the bound of any
 *            summation order).  NaN / inf under null cells never reach a sum.
 *   MIN/MAX  the value column's dtype; null for a group without a non-null cell.  Float64: -0.0 orders below +0.0; if
 *            any non-null cell of the group is NaN the result is NaN (payload unspecified); otherwise the bits of the
 *            smallest / largest cell.  (One integer atomic min / max over an order-preserving map of the bits: exact.)
 *   A bitmap is attached iff some output cell is null; null_count is known; values under nulls are 0.
 *
 * Errors leave the context usable and create nothing: NULL arguments, n_specs == 0, a `col` out of range or an unknown
 * op RV_ERR_INVALID_ARG; a value column whose length differs from the key's RV_ERR_LENGTH_MISMATCH; keys of 2^32 rows
 * or more RV_ERR_UNSUPPORTED (32-bit row ids inside, as the join); more groups than context option "agg_max_groups"
 * (0 = the default 2^26: a group table of at most 1 GiB) RV_ERR_UNSUPPORTED, with the number of distinct keys found
 * before the insert stopped in rv_last_error().  Slices of keys and values at any element offset are fine.  Context
 * option "agg_hash_bits" = b (tests; 0 = all 64) truncates the key hash to b low bits: long probe chains on small
 * inputs, the twin of "join_hash_bits".
 *
 * rv_ctx_last_kernel after rv_hash_aggregate names the accumulate stage: "group_accumulate<lds>" (up to 16384 groups:
 * LDS accumulators per workgroup), "group_accumulate<global>" (more), with "+group_f64_sum" appended -- or
 * "group_f64_sum" alone -- when a Float64 SUM ran.  rv_ctx_kernel_stats (option "profile_kernels") times that stage:
 * the accumulate launches and the Float64 SUM path (its sort included), not the group-id passes before it. */
typedef enum rv_agg_op { RV_AGG_COUNT_ROWS = 0, RV_AGG_COUNT = 1, RV_AGG_SUM = 2, RV_AGG_MIN = 3, RV_AGG_MAX = 4 } rv_agg_op;
typedef struct rv_agg_spec {
    uint32_t op;  /* rv_agg_op */
    uint32_t col; /* index into value_cols; ignored by RV_AGG_COUNT_ROWS */
} rv_agg_spec;
/* Dense group ids: out_gids an Int64 column of key's length without nulls (row -> its group's position in the output),
 * out_first_row an Int64 column of *out_groups rows, ascending (what rv_take_device takes to gather the key cells).
 * out_groups may be NULL. */
rv_status rv_group_ids(rv_ctx *ctx, const rv_dcolumn *key, rv_dcolumn **out_gids, rv_dcolumn **out_first_row, uint64_t *out_groups);
/* The whole operator: out[0] = the key cells of the groups (rv_take_device of key by first_row: null for the null
 * group), out[1 + j] = aggregate j: out has room for n_specs + 1 handles.  out_first_row and out_groups may be NULL. */
rv_status rv_hash_aggregate(rv_ctx *ctx, const rv_dcolumn *key, const rv_dcolumn *const *value_cols, uint32_t n_values,
                            const rv_agg_spec *specs, uint32_t n_specs, rv_dcolumn **out, rv_dcolumn **out_first_row,
                            uint64_t *out_groups);

/* ---- grouped aggregation over several key columns (K9a) ---------------------- */
/* group_by([k_0 .. k_{nkeys-1}]).agg([a_0 .. a_{m-1}]): 1 <= nkeys <= 8 key columns of one length.  A row's key is the TUPLE
 * of its cells, one cell per key column in the order given; two rows are in one group iff their tuples are equal cell by cell.
 * This comment is the normative text (tests/group_keys_model.py the executable one); DESIGN.md section 4 K9a argues it.
 *
 * Cells.  A cell is null, or a value of the column's dtype:
 *   RV_INT64    equal iff the bits are equal.
 *   RV_FLOAT64  every NaN, whatever its sign or payload, equals every other NaN; every other value equals only its own bit
 *               pattern, so -0.0 and +0.0 are DIFFERENT keys.  This is the equality the order of rv_sort induces (all NaNs
 *               compare equal, -0.0 < +0.0): the rows a sort puts side by side as equal are exactly the rows of one group.
 *   RV_BOOLEAN  equal iff the bit is equal.
 *   RV_NULL     every cell is null.
 *   RV_STRING   RV_ERR_UNSUPPORTED -- String keys go through rv_string_dict_build ids (the host layer does that).
 * Nulls.  A null cell equals a null cell of the same column (AnyValue: Null == Null, as K9 and the join have it) and no
 * value; whatever bits lie under a null cell are never read as a value.  There is no special null group: (null, 0),
 * (0, null), (0, 0) and (null, null) are four ordinary, different keys.  With nkeys == 1 this is K9's grouping.
 *
 * Outputs.  rv_hash_aggregate_keys: out[k], k < nkeys = the cells of key column k at the groups' first rows (rv_take_device
 * of the column by first_row: a null stays null, a NaN keeps the bits its first row has); out[nkeys + j] = aggregate j: out
 * has room for nkeys + n_specs handles.  rv_group_ids_keys: out_gids, out_first_row and out_groups as rv_group_ids gives
 * them.  out_first_row (of rv_hash_aggregate_keys) and out_groups may be NULL.
 *
 * Everything else is rv_hash_aggregate's, word for word: the order (groups by ascending first row, the same bytes run to
 * run; an empty key gives zero groups and zero-row outputs of the right dtypes), the aggregates and every numeric rule
 * (Int64 exact, the Float64 SUM order, the MIN / MAX NaN rule), options "agg_max_groups" and "agg_hash_bits" (which
 * truncates the hash of the tuple), slices at any element offset (each column its own), the 2^32-row limit and the names
 * rv_ctx_last_kernel gives the accumulate stage.
 *
 * Errors leave the context usable and create nothing: NULL arguments (a NULL entry of keys included), nkeys == 0,
 * nkeys > 8 and what rv_hash_aggregate calls so RV_ERR_INVALID_ARG; key columns of different lengths, or a value column
 * of another length, RV_ERR_LENGTH_MISMATCH; an RV_STRING key, keys of 2^32 rows or more (checked before anything is
 * read), or more groups than "agg_max_groups" (with the number of distinct keys found so far in rv_last_error())
 * RV_ERR_UNSUPPORTED.
 *
 * rv_ctx_last_kernel after rv_group_ids_keys says "group_ids<keys>" when the passes over tuples ran (group_insert_keys,
 * group_ids_keys: one lane per row, a slot's tuple read at the slot's row, the hash a fold of the cells in key order and
 * of their null flags).  A call with ONE RV_INT64 or RV_NULL key is K9's grouping and runs K9's passes: it says
 * "group_ids".  rv_group_ids and rv_hash_aggregate are unchanged; they still refuse Float64 and Boolean keys. */
rv_status rv_group_ids_keys(rv_ctx *ctx, const rv_dcolumn *const *keys, uint32_t nkeys, rv_dcolumn **out_gids,
                            rv_dcolumn **out_first_row, uint64_t *out_groups);
rv_status rv_hash_aggregate_keys(rv_ctx *ctx, const rv_dcolumn *const *keys, uint32_t nkeys, const rv_dcolumn *const *value_cols,
                                 uint32_t n_values, const rv_agg_spec *specs, uint32_t n_specs, rv_dcolumn **out,
                                 rv_dcolumn **out_first_row, uint64_t *out_groups);

/* ---- sort (K10) ------------------------------------------------------------- */
/* ORDER BY: rv_sort_indices gives the stable permutation of one key column, rv_sort reorders a frame by one or more keys.  The
 * reference has no sort; the semantics are defined here (this comment is the normative text, tests/sort_model.py the executable
 * one) and argued in DESIGN.md section 4 K10.
 *
 * Stability.  Rows whose keys compare equal keep their ascending input order under every flag combination, descending included.
 * The permutation is therefore unique: the same input gives the same indices on every run.
 *
 * Keys.  RV_INT64: the numeric order.  RV_FLOAT64: the order of the map the grouped MIN / MAX use (sign bit set: every bit
 * flipped; otherwise the sign bit set), so -inf < ... < -0.0 < +0.0 < ... < +inf; every NaN, whatever its sign or payload,
 * compares equal to every other NaN and above +inf, so the NaNs stay in row order among themselves.  RV_NULL: every row is null
 * -- the identity, or `prior` unchanged.  RV_BOOLEAN and RV_STRING keys are RV_ERR_UNSUPPORTED.
 *
 * Nulls.  All null cells compare equal and come first (AnyValue: Null is below every value) unless RV_SORT_NULLS_LAST is set.
 * RV_SORT_DESCENDING reverses the order of the VALUES only, by complementing the mapped key -- it never reverses positions, so
 * equal keys stay in row order -- and does not move the nulls: the two flags are independent.  Whatever bits lie under a null
 * cell are never read as a value.
 *
 * Chaining.  `prior` is NULL or an Int64 column without nulls holding a permutation of the key's rows; the result is `prior`
 * reordered stably by key[prior[i]].  Sorting by the keys (k0, k1, ...) is the chain from the last key to the first; there are
 * no composite keys.  A `prior` of another length: RV_ERR_LENGTH_MISMATCH; of another dtype: RV_ERR_TYPE_MISMATCH; with nulls:
 * RV_ERR_INVALID_ARG; an index outside [0, rows): RV_ERR_OUT_OF_BOUNDS with the text rv_take_device gives ("Index 9 out of
 * bounds for 4 rows", the first such index) -- nothing is read through it.
 *
 * Slices of the key (and of its validity) at any offset are fine; indices are relative to the slice.  An empty key gives a
 * zero-row Int64 column.  Keys of 2^32 rows or more: RV_ERR_UNSUPPORTED (32-bit row ids inside, as rv_group_ids).  Unknown flag
 * bits: RV_ERR_INVALID_ARG.  Errors leave the context usable and create nothing.
 *
 * The passes.  An LSD radix sort over the 8-bit digits of the mapped key; a digit position at which all non-null keys agree is
 * skipped (values below 2^16: two passes; an all-equal key: none), and a key with some but not all cells null costs one more
 * pass.  Context option "sort_last_passes" reports the passes of the last call, rv_ctx_last_kernel names "sort_scatter" (or
 * "sort_widen" when no pass ran), rv_ctx_kernel_stats (option "profile_kernels") times the whole sort stage of
 * rv_sort_indices.  Option "sort_engine" = 1 replaces the value passes by rocprim::radix_sort_pairs over all 64 bits. */
#define RV_SORT_DESCENDING 1u
#define RV_SORT_NULLS_LAST 2u
/* the stable permutation: an Int64 column of key->length rows without nulls, what rv_take_device takes */
rv_status rv_sort_indices(rv_ctx *ctx, const rv_dcolumn *key, uint32_t flags, const rv_dcolumn *prior, rv_dcolumn **out_indices);
/* the whole operator: every column of the frame reordered by the keys cols[key_cols[0]], cols[key_cols[1]], ... (flags per key);
 * out has room for ncols handles.  nkeys == 0, a key index out of range or unknown flag bits: RV_ERR_INVALID_ARG; columns of
 * different lengths: RV_ERR_LENGTH_MISMATCH; a key dtype rv_sort_indices refuses: RV_ERR_UNSUPPORTED.  Columns that are no key
 * may be of any dtype rv_take_device gathers (String and Boolean included).  Two keys are two chained rv_sort_indices calls and
 * ONE gather of the frame. */
rv_status rv_sort(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const uint32_t *key_cols, const uint32_t *key_flags,
                  uint32_t nkeys, rv_dcolumn **out);

/* ---- top-k (K11) ------------------------------------------------------------ */
/* ORDER BY ... LIMIT k without sorting the column.  This comment is the normative text, tests/topk_model.py the executable one;
 * DESIGN.md section 4 K11 argues it.
 *
 * The result.  rv_top_k_indices(key, flags, k) is the first min(k, rows) rows of what rv_sort_indices(key, flags, NULL) returns: an
 * Int64 column without nulls.  rv_top_k(cols, keys, k) is the first min(k, rows) rows of every column of rv_sort with the same
 * arguments.  The sort is stable, so both are unique and the same on every run; rows whose keys compare equal come in ascending row
 * order, and ties of the first key that straddle the cut are decided by the later keys, never by row order.  k == 0 gives zero-row
 * columns of the input's dtypes, k >= rows the whole sort.  There is no `prior`.
 *
 * Everything else is the sort's, with the same statuses and texts under this function's name: the key dtypes (RV_INT64, RV_FLOAT64,
 * RV_NULL; RV_BOOLEAN and RV_STRING keys are RV_ERR_UNSUPPORTED), RV_SORT_DESCENDING and RV_SORT_NULLS_LAST, slices at any offset,
 * whatever lies under a null cell is never read as a value, keys of 2^32 rows or more are RV_ERR_UNSUPPORTED, unknown flag bits,
 * nkeys == 0 and a key index out of range are RV_ERR_INVALID_ARG, columns of different lengths RV_ERR_LENGTH_MISMATCH.  Errors
 * leave the context usable and create nothing.  Columns that are no key may be of any dtype rv_take_device gathers.
 *
 * The passes.  A radix SELECT over the 8-bit digits of the first key's mapped key, from the most significant digit at which two
 * non-null keys differ: one pass over the key column counts every digit, each further pass the next differing digit among the rows
 * that still tie with the cut; it stops when no differing digit is left or the candidates -- the rows at or before the cut, every
 * tie of the cut included, the null rows when they come first -- number at most rows / 32.  The candidates' row ids are collected in
 * ascending order, every key column is gathered at them, and rv_sort_indices' chain over those few rows settles the order.  The
 * whole column is sorted instead (rv_sort_indices / rv_sort unchanged, then the first k rows) when k >= rows / 2, when the column
 * is shorter than the built-in crossover, and when the candidates come out as more than half the rows (few distinct keys; nulls
 * last with fewer than k values).  Context option "top_k_last_passes" reports the select's passes over the key column of the last
 * call (0: the whole sort ran), "top_k_last_candidates" the rows it sorted; rv_ctx_last_kernel names "topk_collect" after a select
 * and what the sort names otherwise; rv_ctx_kernel_stats (option "profile_kernels") times the select and the sort stage. */
rv_status rv_top_k_indices(rv_ctx *ctx, const rv_dcolumn *key, uint32_t flags, uint64_t k, rv_dcolumn **out_indices);
/* the whole operator: the first min(k, rows) rows of rv_sort(cols, key_cols, key_flags); out has room for ncols handles.  ONE gather
 * of the frame, of k rows. */
rv_status rv_top_k(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const uint32_t *key_cols, const uint32_t *key_flags,
                   uint32_t nkeys, uint64_t k, rv_dcolumn **out);

/* ---- window functions (K12) -------------------------------------------------- */
/* f(...) OVER (PARTITION BY p_0 .. ORDER BY o_0 ..): one new column per expression, out[j] of the frame's row count and in the
 * INPUT'S ROW ORDER -- a window function adds columns and reorders nothing.  The reference has no window expression; this comment is the
 * normative text, tests/window_model.py the executable one; DESIGN.md section 4 K12 argues it.
 *
 * Partition.  The partition of a row is the set of rows whose tuple of partition-key cells is equal under rv_group_ids_keys' equality
 * (K9a): a null equals a null of the same column, all NaNs are equal, -0.0 != +0.0.  npart == 0: the whole frame is one partition.
 * Partition-key dtypes are what rv_group_ids_keys takes (RV_INT64, RV_FLOAT64, RV_BOOLEAN, RV_NULL), at most 8 columns; an RV_STRING key is
 * RV_ERR_UNSUPPORTED -- the host layer handles String keys through rv_string_dict_build ids.
 *
 * Order.  Within a partition the rows stand in the order rv_sort over (order_cols, order_flags) would give them.  That order is stable, so
 * ties stand in row order and every row has a unique 1-based position `pos` in its partition.  Order-key dtypes and flags are exactly
 * rv_sort_indices' (RV_INT64, RV_FLOAT64, RV_NULL; RV_SORT_DESCENDING, RV_SORT_NULLS_LAST); Boolean and String order keys are refused with
 * its text.  At most 8 order keys.  norder == 0: the order is row order.  Two rows of a partition are PEERS when no order key tells them
 * apart (both cells null, or both values with the same sort key: all NaNs are peers, -0.0 and +0.0 are not); with norder == 0 all rows of a
 * partition are peers.
 *
 * Numbering.  RV_WIN_ROW_NUMBER = pos.  RV_WIN_RANK = pos of the row's first peer.  RV_WIN_DENSE_RANK = the number of peer groups up to and
 * including the row's own.  `col` is ignored (but must be a column index).
 *
 * Running aggregates.  The frame is ROWS UNBOUNDED PRECEDING .. CURRENT ROW: the partition's rows with position <= pos.
 * RV_WIN_CUM_COUNT counts the frame's non-null cells of `col`, any dtype.  RV_WIN_CUM_SUM / CUM_MIN / CUM_MAX take an RV_INT64 or RV_FLOAT64
 * column (any other dtype: RV_ERR_TYPE_MISMATCH), and every numeric rule is rv_hash_aggregate's, applied to the frame instead of the group:
 * Int64 SUM wraps and is exact; SUM over a frame without a non-null cell is 0 / +0.0, no bitmap; MIN / MAX over such a frame is null;
 * Float64 MIN / MAX go through the same order map (-0.0 below +0.0; one NaN in the frame makes the result NaN, payload unspecified);
 * NaN or inf under a null cell never reaches a result.
 *   Float64 CUM_SUM uses no floating-point atomic.  With a (+) b = b when b holds a partition head, else a + b (one IEEE addition; a null
 *   cell and a zero of either sign enter as +0.0, so no result is -0.0), over the rows in sequence order (partitions side by side, each in
 *   its order), tiles of 2048 positions, 256 threads of 8 consecutive positions, 4 waves:
 *     T_t  thread t's left fold of its 8 elements, ((e_0 (+) e_1) (+) ..) (+) e_7;
 *     L_l  what lane l - 1 holds after the steps d = 1, 2, 4, 8, 16, 32 of x_l <- x_{l-d} (+) x_l (l >= d) over the wave's T; identity for lane 0;
 *     W_w  the left fold, from the identity, of the last lanes' x of the waves before wave w;
 *     C_i  the carry into tile i: the same construction over the tile aggregates, 2048 tiles to a round, R (+) (W (+) L) with R the left
 *          fold of the totals of the rounds before;
 *   the result at a thread's k-th position is ((C_i (+) (W_w (+) L_l)) (+) e_0) (+) .. (+) e_k.  Only the row's position in the sequence,
 *   the positions of the partition heads and this fixed geometry enter it: the same call over the same buffers gives the same bits run to
 *   run.  The result is bit exact whenever every partial sum is representable, and otherwise |got - exact| <= gamma_{m-1} x sum|x| over
 *   the frame (m = its non-null cells, gamma as at rv_hash_aggregate: the bound of any summation order).
 *
 * LAG and LEAD.  RV_WIN_LAG(col, offset = k) is the cell of `col` at the partition's row with position pos - k, RV_WIN_LEAD at pos + k;
 * null when there is no such row or that cell is null.  Any dtype rv_take_device_nullable gathers, String and Boolean included.  k == 0
 * copies the column.  `offset` is ignored by every other op.
 *
 * Outputs.  Counts and numbers are Int64 without a bitmap; SUM / MIN / MAX and LAG / LEAD have the column's dtype.  A bitmap is attached
 * iff some output cell is null; null_count is known; values under nulls are 0.  A zero-row frame gives zero-row outputs of the right
 * dtypes.  Slices at any element offset are fine, each column its own.
 *
 * Errors leave the context usable and create nothing: NULL arguments, ncols == 0, nspecs == 0, an unknown op, a column index out of range,
 * unknown flag bits, more than 8 partition or order keys RV_ERR_INVALID_ARG; columns of different lengths RV_ERR_LENGTH_MISMATCH; frames
 * of 2^32 rows or more, and more partitions than context option "agg_max_groups", RV_ERR_UNSUPPORTED.
 *
 * The passes.  (1) The partition ids (rv_group_ids_keys' passes; skipped when npart == 0) and the sequence: rv_sort_indices' chain over
 * the order keys from the last to the first, then over the id column -- with npart == 0 and norder == 0 no sort runs and every kernel reads
 * and writes in place.  All expressions of a call share it.  (2) window_heads: one lane per position, two bitmaps (partition head, peer
 * head).  (3) window_scan, per numbering or aggregate: three launches over the fixed tiles (tile aggregates; their scan by one workgroup;
 * the apply, which stores at out[perm[j]]).  (4) window_shift, per LAG / LEAD: a nullable index list in row order, then
 * rv_take_device_nullable's gather.  No kernel waits for another workgroup.  rv_ctx_last_kernel names "window_scan", or "window_shift" when
 * only LAG / LEAD ran; rv_ctx_kernel_stats (option "profile_kernels") times the sorts (as rv_sort_indices does) and passes (2) - (4). */
typedef enum rv_window_op { RV_WIN_ROW_NUMBER = 0, RV_WIN_RANK = 1, RV_WIN_DENSE_RANK = 2, RV_WIN_CUM_COUNT = 3, RV_WIN_CUM_SUM = 4, RV_WIN_CUM_MIN = 5, RV_WIN_CUM_MAX = 6, RV_WIN_LAG = 7, RV_WIN_LEAD = 8 } rv_window_op;
typedef struct rv_window_spec {
    uint32_t op;     /* rv_window_op */
    uint32_t col;    /* index into cols */
    uint64_t offset; /* RV_WIN_LAG / RV_WIN_LEAD only */
} rv_window_spec;
rv_status rv_window(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const uint32_t *partition_cols, uint32_t npart,
                    const uint32_t *order_cols, const uint32_t *order_flags, uint32_t norder, const rv_window_spec *specs,
                    uint32_t nspecs, rv_dcolumn **out);

/* ---- window frames (K12a) ---------------------------------------------------- */
/* The general form of rv_window: the same partition, order, peers, sequence, output rules (row order; a bitmap iff some cell is null; a
 * known null_count; zeros under nulls), limits and error texts, under its own name.  Ops 0 .. 8 are rv_window_op's with the same values and
 * meaning, ignore preceding / following and give what rv_window gives, so one call computes old and new expressions over ONE sequence.
 * The reference has no window expression; this comment is the normative text, tests/window_frame_model.py the executable one; DESIGN.md
 * section 4 K12a argues it.
 *
 * Frame.  For a row at the 1-based position pos of a partition of len rows, the positions [max(1, pos - preceding), min(len, pos +
 * following)] of that partition; EMPTY when that interval is empty.  Offsets are signed: preceding = 3, following = -1 is "the three rows
 * before this one", preceding = -1, following = RV_FRAME_UNBOUNDED is "everything after this row".  RV_FRAME_UNBOUNDED on either side
 * means the partition's edge.  A finite offset has a magnitude of at most 2^62, and preceding + following >= 0 when both are finite;
 * anything else is RV_ERR_INVALID_ARG naming the expression.  (Offsets are clamped before anything is added: no signed overflow.)
 *
 * RV_WINF_COUNT: the non-null cells of `col` in the frame.  Any dtype.  Int64, no bitmap, 0 for an empty frame.
 *
 * RV_WINF_SUM / MIN / MAX take an RV_INT64 or RV_FLOAT64 column (any other dtype: RV_ERR_TYPE_MISMATCH); every numeric rule is
 * rv_hash_aggregate's applied to the frame, as at rv_window: Int64 SUM wraps and is exact; SUM over a frame without a non-null cell (an
 * empty one included) is 0 / +0.0, no bitmap; MIN / MAX over such a frame is null; Float64 MIN / MAX go through the same order map (-0.0
 * below +0.0; one NaN in the frame makes the result NaN, payload unspecified); nothing under a null cell reaches a result.
 *
 * RV_WINF_AVG: Float64; null when the frame has no non-null cell, otherwise RV_WINF_SUM's result divided by RV_WINF_COUNT's with one IEEE
 * division -- for an Int64 column the wrapped Int64 sum is converted to double first.
 *
 * RV_WINF_FIRST_VALUE / LAST_VALUE: the cell of `col` at the frame's first / last position; null when the frame is empty or that cell is
 * null (there is no IGNORE NULLS).  Any dtype rv_take_device_nullable gathers, String and Boolean included: the route of LAG / LEAD, a
 * nullable index list in row order and then the gather.
 *
 * RV_WINF_NTILE(n = offset): with q = len / n and r = len % n the partition's first r buckets hold q + 1 rows and the rest q, in window
 * order; the result is the row's 1-based bucket (n > len: the bucket is pos).  Int64, no bitmap.  n == 0: RV_ERR_INVALID_ARG.  `col`
 * is ignored (but must be a column index), as are preceding / following.
 *
 * Float64 SUM uses no floating-point atomic.  A frame of the finite width w = preceding + following + 1 cuts every partition into blocks
 * of w positions anchored at the partition's head (with an unbounded side, or w >= len, the block is the partition).  prefix[j] is the
 * sum of j's block up to j, bracketed exactly as rv_window's CUM_SUM with the block heads in the place of the partition heads (T, L, W, C
 * above); suffix[j], the sum of j's block from j on, is the mirror image: the same construction over the positions counted from the
 * sequence's end, so a thread folds its 8 positions from the highest down and a (+) b stands for a AFTER b.  A frame [lo, hi] within one
 * block is prefix[hi] (lo starts the block) or suffix[lo] (hi ends it, or the partition); across two blocks it is the one final addition
 * suffix[lo] + prefix[hi].  The result depends only on the row's position in the sequence, the partition heads, the frame and this fixed
 * geometry: the same call over the same buffers gives the same bits run to run.  It is bit exact whenever every partial sum is
 * representable, and otherwise |got - exact| <= gamma_{m-1} x sum|x| over the frame (m its non-null cells): every result is a summation
 * tree over exactly the frame's cells -- no difference of prefix sums -- and additions of the +0.0 that stands for a null are exact.  A
 * zero of either sign enters as +0.0, so no sum is -0.0.  MIN / MAX / COUNT / Int64 SUM are made the same way and are exact.
 *
 * Errors: rv_window's, and those named above; an op above RV_WINF_NTILE is unknown.
 *
 * The passes.  (1) rv_window's sequence, shared by all expressions.  (2) When a frame op is asked for: head_pos / tail_pos of every
 * position (two scans over the partition-head bitmap; npart == 0: one partition, nothing to scan), and per distinct value column one
 * gather into sequence order (skipped in place).
 * (3) Per distinct finite width the block-head bitmap; per (column, SUM-COUNT-AVG | MIN | MAX, width) the block prefix and / or suffix
 * scan, three launches each, value and non-null count per position (an unbounded preceding side needs the prefix only, an unbounded
 * following side the suffix only).  (4) window_frame, per expression: one lane per position picks the case, combines, finishes and stores
 * at out[perm[j]].  FIRST / LAST / NTILE need (2)'s geometry only.  No kernel waits for another workgroup; the cost does not depend on the
 * frame's width.  rv_ctx_last_kernel names "window_frame" when an op from RV_WINF_COUNT on ran, and what rv_window names otherwise;
 * rv_ctx_kernel_stats (option "profile_kernels") times these passes along with rv_window's. */
#define RV_FRAME_UNBOUNDED INT64_MAX
typedef enum rv_window_frame_op { RV_WINF_COUNT = 9, RV_WINF_SUM = 10, RV_WINF_MIN = 11, RV_WINF_MAX = 12, RV_WINF_AVG = 13, RV_WINF_FIRST_VALUE = 14, RV_WINF_LAST_VALUE = 15, RV_WINF_NTILE = 16 } rv_window_frame_op;
typedef struct rv_window_frame_spec {
    uint32_t op;       /* rv_window_op (0 .. 8) or rv_window_frame_op */
    uint32_t col;      /* index into cols */
    uint64_t offset;   /* RV_WIN_LAG / RV_WIN_LEAD: k; RV_WINF_NTILE: the number of buckets */
    int64_t preceding; /* frame ops only */
    int64_t following;
} rv_window_frame_spec;
rv_status rv_window_frames(rv_ctx *ctx, const rv_dcolumn *const *cols, uint32_t ncols, const uint32_t *partition_cols, uint32_t npart,
                           const uint32_t *order_cols, const uint32_t *order_flags, uint32_t norder, const rv_window_frame_spec *specs,
                           uint32_t nspecs, rv_dcolumn **out);

/* ---- multi-GPU (one process per GPU) --------------------------------------- */
/* Row-range shard of rank `rank` of `world`: [*begin, *end), boundaries at multiples of
 * 64 rows so selection-bitmap words never straddle ranks. */
rv_status rv_shard_range(uint64_t n_rows, uint32_t world, uint32_t rank, uint64_t *begin,
                         uint64_t *end);
#define RV_COMM_ID_BYTES 128
rv_status rv_comm_unique_id(uint8_t id[RV_COMM_ID_BYTES]);
rv_status rv_comm_create(rv_ctx *ctx, const uint8_t id[RV_COMM_ID_BYTES], uint32_t world,
                         uint32_t rank, rv_comm **out);
/* ncclAllReduce(count = 2, ncclInt64, ncclSum) over xGMI: {sum, count} in place. */
rv_status rv_comm_allreduce_sum_count(rv_comm *comm, int64_t *sum, uint64_t *count);
rv_status rv_comm_destroy(rv_comm *comm);

/* ---- multi-GPU, ONE process: a group of contexts (SURVEY.md sections 8b, 8e) ---------- */
/* The caller the north star names is a single Rust process driving the 8 GPUs of a node.  A group owns one
 * context and one host worker thread per entry of `devices`; a table is sharded by row range (shard r holds
 * rows rv_shard_range(length, n, r)), every device runs the same single-pass kernels on its shard, and there is
 * no collective on the data path.  The same device may be listed more than once (contexts are independent):
 * that is how the protocol is rehearsed on a one-GPU box.  Calls on one group are serialised by the caller
 * (`&mut self`), like calls on one context. */
typedef struct rv_group rv_group;
typedef struct rv_gather rv_gather; /* a query result gathered on the host, in rank order == row order */

rv_status rv_group_create(const int *devices, uint32_t n, rv_group **out);
rv_status rv_group_destroy(rv_group *group);
uint32_t rv_group_size(const rv_group *group);
rv_ctx *rv_group_ctx(rv_group *group, uint32_t rank);

/* Sharded columns: shards[r] lives on rank r's device.  rv_group_generate: rank r generates rows
 * [begin_r, end_r) of the spec with the GLOBAL row index (first_row + begin_r), so the shards agree with the
 * unsharded column without moving data.  rv_group_upload: rank r receives rows [begin_r, end_r) of the host
 * array (offset honoured).  rv_group_free releases the n handles. */
rv_status rv_group_generate(rv_group *group, const rv_synth_spec *spec, rv_dcolumn **shards);
rv_status rv_group_upload(rv_group *group, const rv_column *host, rv_dcolumn **shards);
rv_status rv_group_free(rv_group *group, rv_dcolumn **shards);

/* BASELINE configs[3]: row-range partitioned filter + project, no collective, concat on the host.
 * shards[r * ncols + c] = column c of rank r.  Every rank runs rv_filter_project on its shard (all devices
 * at once); the N survivor counts are prefix-summed on the host and every device copies its output into its
 * slice of ONE pinned host buffer per column -- the gather the reference does with
 * collect_stream_batches -> RecordBatch::concat (streaming.rs:343-352, record_batch.rs:245-342), with the
 * shards as the batches: rank order == row order, validity kept only if a null survived somewhere. */
/* The same for a HOST-resident table (ABI 4): StreamingPhysicalPlan::collect() over N devices (streaming.rs:71-133; dataframe_to_batches
 * :135-233 is the source it replaces, collect_stream_batches -> concat :343-352 the gather).  The table is cut into N row ranges
 * (rv_shard_range), every range streamed through its device's own double-buffered chunk pipeline (rv_filter_project_host) -- all
 * devices at once, each over its own PCIe link -- and the survivors gathered in rank order == row order.  host_cols as for
 * rv_filter_project_host (pinned memory uploads at link rate); chunk_rows 0 = 32 Mi.  rank_upload_gbs[n] (may be NULL): what every
 * rank's link carried, GB/s of its range's input bytes over its filter time. */
rv_status rv_group_filter_project_host(rv_group *group, const rv_column *host_cols, uint32_t ncols, const rv_predicate *pred,
                                       const uint32_t *proj, uint32_t nproj, uint64_t chunk_rows, rv_gather **out,
                                       uint64_t *out_rows, double *rank_upload_gbs);
rv_status rv_group_filter_project(rv_group *group, const rv_dcolumn *const *shards, uint32_t ncols,
                                  const rv_predicate *pred, const uint32_t *proj, uint32_t nproj,
                                  rv_gather **out, uint64_t *out_rows);
/* The same in its two phases, for a caller that keeps the result in HBM (and for measuring them apart):
 *   rv_group_filter_project_resident  every rank's rv_filter_project, all devices at once; outs[r * nproj + j] = output
 *                                     column j of rank r, resident on rank r's device (freed with rv_free on
 *                                     rv_group_ctx(group, r)); rank_rows[n] (may be NULL) the survivors per rank.  If any
 *                                     rank fails, every output is released and the first failure is returned -- after ALL
 *                                     ranks have finished, so nothing is still running on a device when the call returns;
 *   rv_group_gather                   the collect leg over such outputs: prefix sum of the N lengths, one pinned host
 *                                     buffer per column, rank order == row order (streaming.rs:343-352). */
rv_status rv_group_filter_project_resident(rv_group *group, const rv_dcolumn *const *shards, uint32_t ncols,
                                           const rv_predicate *pred, const uint32_t *proj, uint32_t nproj,
                                           rv_dcolumn **outs, uint64_t *rank_rows, uint64_t *out_rows);
rv_status rv_group_gather(rv_group *group, const rv_dcolumn *const *outs, uint32_t nproj, rv_gather **out);
/* column j of the result as a host rv_column (pinned memory owned by the result; offset 0). */
rv_status rv_gather_column(const rv_gather *result, uint32_t j, rv_column *view, int64_t *null_count);
/* surviving rows per rank (n entries) and the two phases' wall times: filter_ms = slowest rank's
 * rv_filter_project (launch to row count), gather_ms = prefix sum + device-to-host copies + bitmap merge. */
rv_status rv_gather_stats(const rv_gather *result, uint64_t *rank_rows, double *filter_ms, double *gather_ms);
rv_status rv_gather_free(rv_gather *result);

/* BASELINE configs[4]: rv_filter_agg per rank, then ONE all-reduce of {SUM, COUNT} -- ncclAllReduce(count = 2,
 * ncclInt64, ncclSum) (+ 1 x ncclFloat64 for a Float64 SUM) on communicators made by ncclCommInitAll over the
 * group's devices; every rank ends with the same 16 bytes (checked).  A group that lists a device twice cannot
 * form an RCCL communicator: its partials are summed on the host in rank order instead. */
rv_status rv_group_filter_agg(rv_group *group, const rv_dcolumn *const *shards, uint32_t ncols,
                              const rv_predicate *pred, uint32_t agg_col, int64_t *sum_i, double *sum_f,
                              uint64_t *count);
/* Failure contract of the collective: the all-reduce is entered only after EVERY rank's rv_filter_agg has returned
 * successfully (a rank that fails -- out of memory on one device, a device fault -- makes the call return that rank's
 * error; no rank is left waiting inside RCCL), it is issued for all ranks by the calling thread inside one
 * ncclGroupStart / ncclGroupEnd, and the wait for it is bounded (environment RV_GROUP_TIMEOUT_MS, default 120 000):
 * on a failure or timeout the communicators are aborted (ncclCommAbort) and re-made by the next call.
 * Counters of a group: "rccl_ranks" (ranks of the communicator ncclCommInitAll formed, 0: none yet / host sum),
 * "allreduce_calls", "comm_aborts", "distinct_devices" (0 / 1), "last_agg_filter_us", "last_allreduce_us" (wall time of
 * the two phases of the last rv_group_filter_agg). */
rv_status rv_group_stat(rv_group *group, const char *key, int64_t *value);

/* ---- CSV scan on the device (CsvFileStream, file_stream.rs:10-368) -------------------------------------------------
 * The file goes to HBM in pinned chunks (the read of the next chunk overlaps the parse of this one) and gfx950 kernels
 * split and parse it.  rv_csv_next returns the batches CsvFileStream::next_batch returns, call by call: the header (line
 * 1) is skipped, blank lines are skipped but counted, a trailing '\r' is stripped, cells are trimmed and "" / "null" is a
 * null.  batch_rows 0: calculate_adaptive_batch_size.  Int64 / Float64 columns carry a bitmap only in a batch that holds
 * a null; RV_CSV_NULLS_AS_REFERENCE inverts it as the reference does (file_stream.rs:213-249).
 * A bad line returns RV_ERR_PARSE with the reference's text in rv_last_error() ("Line 3, field 0: Cannot parse 'x2' as
 * Int64", "Line 2: Expected 4 fields, found 3"); the rows of that batch before it are dropped and the next call starts
 * at the line after it.  chunk_bytes 0: 64 MiB; a line longer than a chunk makes the chunk grow.
 * delimiter: one byte (0 .. 255).
 * rv_csv_next: out[0 .. ncols) receives device columns (zero-copy slices of the parsed chunk, released with rv_free);
 * *out_rows == 0: the end of the stream, nothing written to out. */
#define RV_CSV_NULLS_AS_REFERENCE 1u
rv_status rv_csv_open(rv_ctx *ctx, const char *path, const rv_dtype *dtypes, uint32_t ncols, uint32_t delimiter,
                      uint64_t batch_rows, uint32_t flags, uint64_t chunk_bytes, rv_csv_reader **out);
rv_status rv_csv_next(rv_csv_reader *reader, rv_dcolumn **out, uint64_t *out_rows);
/* batch_rows: the rows of a full batch; lines: file lines parsed so far (the header and blank lines included);
 * bytes_read: file bytes read so far */
rv_status rv_csv_reader_info(const rv_csv_reader *reader, uint64_t *batch_rows, uint64_t *lines, uint64_t *bytes_read);
rv_status rv_csv_close(rv_csv_reader *reader);

/* Pin caller-owned host memory (e.g. a shared-memory segment several one-GPU processes gather into) so that
 * rv_download / rv_upload move it by DMA. */
rv_status rv_host_register(rv_ctx *ctx, void *ptr, size_t bytes);
rv_status rv_host_unregister(rv_ctx *ctx, void *ptr);

#ifdef __cplusplus
}
#endif
#endif /* RIVULUS_GPU_H */
