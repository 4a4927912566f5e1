// CPU test of the staged pass's launch rule (rivulus_amd/csrc/fused_rule.hpp): a stand-alone program, built with g++ (plain and with
// -fsanitize=address,undefined) by tests/test_fused_rule_cpu.py, which writes the real launch tables to a file and passes its path:
//   flag NAME VALUE                       the FF_* values of scan_frontend.hpp
//   tall NARROW PACKED                    kNarrowTallRows, kPackedTallRows of fused_table.hpp
//   entry SOURCE NCOLS R VEC WAVES FLAGS  every staged entry in registry order; SOURCE 0..7: lean1 valid1 multi bool full expr roomy narrow
// The specification is the code the rule replaced: `ref` below holds find_fused, pick_fused, narrow_instantiated and the walk loop of
// choose_launch as they stood in fused_launch.hip, over these records (`forced` for the context's option "rows_per_lane"; "none"
// returned where pick_fused raised; in the loop, the sizing's part of `crowded` is an input: true for the first `crowded_first` candidates
// sized).  Nothing is skipped: every combination is compared, "none" on both sides counts as equal, and the counts are printed.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../rivulus_amd/csrc/fused_rule.hpp"

struct Entry {
    int ncols, r, vec, waves, flags;
    int source;
};
static std::vector<Entry> table;
static size_t source_begin[9];
static int kNarrowTallRows, kPackedTallRows;

namespace ref {
namespace rvk {
static int FF_VALIDITY, FF_BOOL, FF_XS, FF_SEL, FF_STAMP, FF_ONE_I64, FF_ONE_F64, FF_PROJALL, FF_NONULL, FF_EXPR, FF_NARROW16, FF_NARROW32, FF_PACK10;
using FusedEntry = Entry;
static const FusedEntry *source(int s, size_t *n) {
    *n = source_begin[s + 1] - source_begin[s];
    return table.data() + source_begin[s];
}
static const FusedEntry *fused_entries_lean1(size_t *n) { return source(0, n); }
static const FusedEntry *fused_entries_valid1(size_t *n) { return source(1, n); }
static const FusedEntry *fused_entries_multi(size_t *n) { return source(2, n); }
static const FusedEntry *fused_entries_bool(size_t *n) { return source(3, n); }
static const FusedEntry *fused_entries_full(size_t *n) { return source(4, n); }
static const FusedEntry *fused_entries_expr(size_t *n) { return source(5, n); }
static const FusedEntry *fused_entries_roomy(size_t *n) { return source(6, n); }
static const FusedEntry *fused_entries_narrow(size_t *n) { return source(7, n); }
}  // namespace rvk
struct Ctx {
    int64_t opt_rows_per_lane;
};
static int kNarrowFlags;

static const rvk::FusedEntry *find_fused(Ctx *ctx, int ncols, int vec, int need, int roomy = 0, int below_r = 1 << 30, int prefer_r = 0) {
    const rvk::FusedEntry *best = nullptr;
    auto scan = [&](const rvk::FusedEntry *t, size_t n) {
        for (size_t i = 0; i < n; ++i) {
            const rvk::FusedEntry &e = t[i];
            const int kShape = rvk::FF_ONE_I64 | rvk::FF_ONE_F64 | rvk::FF_STAMP | rvk::FF_PROJALL | rvk::FF_NONULL | rvk::FF_EXPR | kNarrowFlags;  // must match exactly
            // the generic FF_PROJALL instantiations write the selection bitmap on request (fused_kernel.hpp, kSel)
            const int has = e.flags | (((e.flags & rvk::FF_PROJALL) && !(e.flags & (rvk::FF_ONE_I64 | rvk::FF_ONE_F64))) ? rvk::FF_SEL : 0);
            if (e.ncols != ncols || (ncols > 0 && e.vec != vec) || (has & need) != need) continue;
            if ((e.flags & kShape) != (need & kShape)) continue;
            bool wanted = false;
            if (ctx->opt_rows_per_lane > 0) {
                const int want_r = static_cast<int>(ctx->opt_rows_per_lane & 0xFF);
                const int want_w = static_cast<int>((ctx->opt_rows_per_lane >> 8) & 0xFF);
                wanted = e.r == want_r && (want_w == 0 || e.waves == want_w);
            } else if (prefer_r > 0 && roomy == 0) {
                wanted = e.r == prefer_r;
            }
            // roomy 1: a 16-wave geometry with fewer rows per lane -- its LDS slots hold a larger share of a wave's
            // rows; roomy 2: the 8-wave geometries of fused_roomy.hip, whose slots hold every row of a wave
            if (roomy == 1 && ctx->opt_rows_per_lane <= 0 && ncols >= 1)  // ... among those with fewer than below_r rows per lane, the largest
                wanted = best && e.waves == 16 && e.r < below_r && (best->waves != 16 || best->r >= below_r || e.r > best->r);
            if (roomy == 2 && ctx->opt_rows_per_lane <= 0 && ncols >= 1) wanted = best && (e.waves < best->waves || (e.waves == best->waves && e.r < best->r));
            if (!best || __builtin_popcount(e.flags) < __builtin_popcount(best->flags) ||
                (wanted && e.flags == best->flags))
                best = &e;
        }
    };
    size_t n = 0;
    const rvk::FusedEntry *t;
    // first match wins among equals, so list the preferred default geometry first in each table
    for (int pass = 0; pass < 2 && !best; ++pass) {
        t = rvk::fused_entries_lean1(&n), scan(t, n);
        t = rvk::fused_entries_valid1(&n), scan(t, n);
        t = rvk::fused_entries_multi(&n), scan(t, n);
        t = rvk::fused_entries_bool(&n), scan(t, n);
        t = rvk::fused_entries_full(&n), scan(t, n);
        t = rvk::fused_entries_expr(&n), scan(t, n);
        t = rvk::fused_entries_roomy(&n), scan(t, n);
        t = rvk::fused_entries_narrow(&n), scan(t, n);
        vec = 1;  // every feature set exists with 8-byte loads
    }
    return best;
}
// `prefer`: shape flags worth having when an instantiation exists (FF_PROJALL)
static const rvk::FusedEntry *pick_fused(Ctx *ctx, int ncols, int vec, int need, int prefer = 0, int roomy = 0, int below_r = 1 << 30, int prefer_r = 0) {
    // the refinements the launch qualifies for, dropped one by one (FF_NONULL first) until an instantiation exists
    const rvk::FusedEntry *best = nullptr;
    for (const int pf : {prefer, prefer & ~rvk::FF_NONULL}) {
        if (best || !pf) continue;
        best = find_fused(ctx, ncols, vec, need | pf, roomy, below_r, prefer_r);
        if (best && (best->flags & ~(need | pf)) != 0) best = nullptr;  // not at the price of features the launch does not need
    }
    if (!best) best = find_fused(ctx, ncols, vec, need, roomy, below_r, prefer_r);
    return best;  // (the library raised RV_ERR_INTERNAL "no fused kernel variant" here)
}

static bool narrow_instantiated(int flags, int64_t forced) {
    size_t n = 0;
    const rvk::FusedEntry *t = rvk::fused_entries_narrow(&n);
    const int want_r = static_cast<int>(forced & 0xFF), want_w = static_cast<int>((forced >> 8) & 0xFF);
    for (size_t i = 0; i < n; ++i)
        if (t[i].flags == flags && (forced <= 0 || (t[i].r == want_r && (want_w == 0 || t[i].waves == want_w)))) return true;
    return false;
}
}  // namespace ref

// What a launch sized: the candidate, how (dense sizing), and the flags and selection bitmap the launch stood at.
struct Visit {
    const Entry *e;
    bool dense_sizing;
    int need;
    bool make_selection;
    bool operator==(const Visit &o) const { return e == o.e && dense_sizing == o.dense_sizing && need == o.need && make_selection == o.make_selection; }
};
struct WalkCase {
    int nvals, vec, need, prefer;
    int64_t forced;
    bool counts;          // req && req->counts
    uint64_t chunk_rows;  // req->chunk_rows
    bool sel_deferred;
    int crowded_first;  // the sizing finds the first so many candidates crowded
};
constexpr size_t kMaxWalk = 24;  // (more candidates than any class has: the program fails if a walk gets there)

namespace ref {
static std::vector<Visit> walk(const WalkCase &w) {
    using namespace rvk;
    Ctx context{w.forced}, *ctx = &context;
    struct {
        int need;
        bool make_selection = false;
        const Entry *staged = nullptr;
    } c;
    c.need = w.need;
    const int nvals = w.nvals, vec = w.vec, prefer = w.prefer;
    const bool sel_deferred = w.sel_deferred;
    auto counts_in_pass = [&](int r) { return w.counts && w.chunk_rows % (64u * static_cast<uint64_t>(r)) == 0; };
    std::vector<Visit> out;
    int sized = 0;
    int min_r = 0, below_r = 1 << 30;  // pick_fused's `roomy` level (0 default, 1 walk down the 16-wave geometries, 2 fewest waves)
    bool dense_sizing = false;
    while (out.size() <= kMaxWalk) {
        const int tall_r = (c.need & rvk::FF_PACK10) ? kPackedTallRows : (((c.need & kNarrowFlags) && !w.counts) ? kNarrowTallRows : 0);
        c.staged = pick_fused(ctx, nvals, vec, c.need, prefer, min_r, below_r, tall_r);
        if (!c.staged) break;
        if (min_r == 1 && (c.staged->waves != 16 || c.staged->r >= below_r)) {  // no 16-wave geometry below that many rows per lane left
            if (!dense_sizing) {  // the walk again, sized for a dense selection
                dense_sizing = true;
                below_r = 1 << 30;
            } else if (c.need & rvk::FF_PACK10) {
                c.need &= ~kNarrowFlags;
                min_r = 0, below_r = 1 << 30, dense_sizing = false;
            } else {
                min_r = 2;
            }
            continue;
        }
        if (sel_deferred && !c.make_selection && !counts_in_pass(c.staged->r)) {  // the caller will count the selection bitmap instead
            c.make_selection = true;
            c.need = (c.need | rvk::FF_SEL) & ~kNarrowFlags;  // (the forms that write the selection bitmap read the 8-byte values)
            c.staged = pick_fused(ctx, nvals, vec, c.need, prefer, min_r, below_r);
            if (!c.staged) break;
        }
        out.push_back({c.staged, dense_sizing, c.need, c.make_selection});  // size_staged(ctx, c, *c.staged, n, nvals, nxs, row_bytes, dense_sizing);
        const bool crowded = min_r < 2 && ctx->opt_rows_per_lane <= 0 && nvals >= 1 && sized++ < w.crowded_first;
        if (!crowded) break;
        below_r = c.staged->r;  // the next 16-wave geometry with fewer rows per lane
        min_r = 1;
    }
    if (!c.staged) out.push_back({nullptr, false, 0, false});
    return out;
}
}  // namespace ref

static rvf::Flags rule_flags;
static rvf::Table<Entry> rule_table;

// choose_launch's loop over the rule's candidates (fused_launch.hip)
static std::vector<Visit> rule_walk(const WalkCase &w, bool *reclassed_later) {
    std::vector<Visit> out;
    bool make_selection = false;
    int sized = 0;
    rvf::Walk<Entry> walk{rule_table, rule_flags, {kNarrowTallRows, kPackedTallRows}, w.nvals, w.vec, w.need, w.prefer, w.forced, w.counts};
    const Entry *e = nullptr;
    for (e = walk.first(); out.size() <= kMaxWalk; e = walk.next()) {
        if (e && w.sel_deferred && !make_selection && !(w.counts && rvf::whole_ranges(w.chunk_rows, e->r))) {
            make_selection = true;
            e = walk.reclass((walk.need | ref::rvk::FF_SEL) & ~rule_flags.narrow);
            if (!out.empty()) *reclassed_later = true;
        }
        if (!e) break;
        out.push_back({e, walk.dense_sizing(), walk.need, make_selection});
        const bool crowded = sized++ < w.crowded_first;
        if (!crowded || walk.last()) break;
    }
    if (!e) out.push_back({nullptr, false, 0, false});
    return out;
}

static const Entry *rule_pick(int ncols, int vec, int need, int prefer, int roomy, int below_r, int prefer_r, int64_t forced) {
    const rvf::Class c = rvf::launch_class(rule_table, rule_flags, ncols, vec, need, prefer);
    if (!c.found) return nullptr;
    const rvf::Step step = roomy == 0 ? rvf::Step::kDefault : (roomy == 1 ? rvf::Step::kBelow : rvf::Step::kFewest);
    return rvf::geometry(rule_table, ncols, c, step, below_r, forced, prefer_r);
}

static long failures = 0;
static void fail(const char *what, const std::string &detail) {
    if (++failures <= 20) std::printf("FAILED %s: %s\n", what, detail.c_str());
}
static std::string name(const Entry *e) {
    if (!e) return "none";
    char b[96];
    std::snprintf(b, sizeof b, "<%d,%d,%d,%d,%d>", e->ncols, e->r, e->vec, e->waves, e->flags);
    return b;
}

int main(int argc, char **argv) {
    using namespace ref::rvk;
    if (argc != 2) return std::printf("usage: fused_rule_tests TABLES\n"), 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return std::printf("cannot read %s\n", argv[1]), 2;
    struct {
        const char *name;
        int *value;
    } flags[] = {{"FF_VALIDITY", &FF_VALIDITY}, {"FF_BOOL", &FF_BOOL},       {"FF_XS", &FF_XS},           {"FF_SEL", &FF_SEL},           {"FF_STAMP", &FF_STAMP},
                 {"FF_ONE_I64", &FF_ONE_I64},   {"FF_ONE_F64", &FF_ONE_F64}, {"FF_PROJALL", &FF_PROJALL}, {"FF_NONULL", &FF_NONULL},     {"FF_EXPR", &FF_EXPR},
                 {"FF_NARROW16", &FF_NARROW16}, {"FF_NARROW32", &FF_NARROW32}, {"FF_PACK10", &FF_PACK10}};
    char word[64], fname[64];
    int last_source = -1, flags_read = 0;
    while (std::fscanf(f, "%63s", word) == 1) {
        if (!std::strcmp(word, "flag")) {
            int v = 0;
            if (std::fscanf(f, "%63s %d", fname, &v) != 2) return std::printf("bad flag line\n"), 2;
            for (auto &fl : flags)
                if (!std::strcmp(fl.name, fname)) *fl.value = v, ++flags_read;
        } else if (!std::strcmp(word, "tall")) {
            if (std::fscanf(f, "%d %d", &kNarrowTallRows, &kPackedTallRows) != 2) return std::printf("bad tall line\n"), 2;
        } else if (!std::strcmp(word, "entry")) {
            Entry e{};
            if (std::fscanf(f, "%d %d %d %d %d %d", &e.source, &e.ncols, &e.r, &e.vec, &e.waves, &e.flags) != 6) return std::printf("bad entry line\n"), 2;
            if (e.source < last_source || e.source > 7) return std::printf("entries out of registry order\n"), 2;
            for (; last_source < e.source; ++last_source) source_begin[last_source + 1] = table.size();
            table.push_back(e);
        } else {
            return std::printf("unknown line %s\n", word), 2;
        }
    }
    std::fclose(f);
    for (; last_source < 8; ++last_source) source_begin[last_source + 1] = table.size();
    if (flags_read != 13 || !kNarrowTallRows || !kPackedTallRows || table.empty()) return std::printf("incomplete tables\n"), 2;
    ref::kNarrowFlags = FF_NARROW16 | FF_NARROW32 | FF_PACK10;
    rule_flags = {FF_ONE_I64 | FF_ONE_F64 | FF_STAMP | FF_PROJALL | FF_NONULL | FF_EXPR | ref::kNarrowFlags, FF_ONE_I64 | FF_ONE_F64, FF_PROJALL, FF_NONULL, FF_SEL,
                  ref::kNarrowFlags, FF_PACK10};
    rule_table = {table.data(), table.size()};

    // the values of each dimension
    std::set<int> needs, rows, narrow_flags;
    std::set<int64_t> forced_set = {0, 5 | (3 << 8)};  // (no table holds 5 rows per lane in 3 waves)
    for (const Entry &e : table) {
        const int clearable[4] = {FF_VALIDITY, FF_BOOL, FF_XS, FF_SEL};
        for (int m = 0; m < 16; ++m) {
            int need = e.flags;
            for (int b = 0; b < 4; ++b)
                if (m >> b & 1) need &= ~clearable[b];
            needs.insert(need);
            needs.insert(need | FF_SEL);
        }
        rows.insert(e.r);
        forced_set.insert(e.r | (e.waves << 8));
        forced_set.insert(e.r);
        if (e.flags & ref::kNarrowFlags) narrow_flags.insert(e.flags);
    }
    std::vector<int> below(rows.begin(), rows.end());
    below.push_back(1 << 30);
    const int prefers[4] = {0, FF_PROJALL, FF_PROJALL | FF_NONULL, FF_NONULL};
    const int prefer_rs[4] = {0, 32, 48, 7};

    long picks = 0;
    for (int ncols = 0; ncols <= 4; ++ncols)
        for (int vec = 1; vec <= 2; ++vec)
            for (const int need : needs)
                for (const int prefer : prefers)
                    for (int roomy = 0; roomy <= 2; ++roomy)
                        for (const int below_r : below)
                            for (const int prefer_r : prefer_rs)
                                for (const int64_t forced : forced_set) {
                                    ref::Ctx ctx{forced};
                                    const Entry *want = ref::pick_fused(&ctx, ncols, vec, need, prefer, roomy, below_r, prefer_r);
                                    const Entry *got = rule_pick(ncols, vec, need, prefer, roomy, below_r, prefer_r, forced);
                                    ++picks;
                                    if (want != got) {
                                        char b[200];
                                        std::snprintf(b, sizeof b, "ncols %d vec %d need %d prefer %d roomy %d below_r %d prefer_r %d forced %" PRId64 ": ", ncols, vec, need,
                                                      prefer, roomy, below_r, prefer_r, forced);
                                        fail("pick", b + name(want) + " expected, the rule gives " + name(got));
                                    }
                                }
    std::printf("picks %ld\n", picks);

    long members = 0;
    for (const int fl : narrow_flags)
        for (const int64_t forced : forced_set) {
            ++members;
            if (ref::narrow_instantiated(fl, forced) != rvf::holds_exactly(rule_table, fl, forced)) fail("membership", std::to_string(fl) + " forced " + std::to_string(forced));
        }
    std::printf("members %ld\n", members);

    // every class with more than one geometry, walked: `need` is the class's flags
    std::set<std::vector<int>> classes;
    for (const Entry &a : table) {
        int same = 0;
        for (const Entry &b : table) same += b.ncols == a.ncols && b.vec == a.vec && b.flags == a.flags;
        if (same > 1) classes.insert({a.ncols, a.vec, a.flags});
    }
    const uint64_t chunks[5] = {0, 1024, 768, 1536, 1000};  // per-batch counts off; batches of so many rows
    long walks = 0, restarts = 0, reclassed_later = 0, longest = 0;
    for (const auto &cl : classes)
        for (const int prefer : prefers)
            for (const uint64_t chunk : chunks)
                for (int sel = 0; sel <= 1; ++sel)
                    for (const int64_t forced : {int64_t(0), int64_t(8 | (16 << 8))})
                        for (int crowded_first = 0; crowded_first <= static_cast<int>(kMaxWalk); ++crowded_first) {
                            const WalkCase w{cl[0], cl[1], cl[2], prefer, forced, chunk != 0, chunk, sel != 0, crowded_first};
                            const std::vector<Visit> want = ref::walk(w);
                            bool later = false;
                            const std::vector<Visit> got = rule_walk(w, &later);
                            ++walks;
                            reclassed_later += later;
                            restarts += (cl[2] & FF_PACK10) && !want.empty() && want.back().e && !(want.back().need & FF_PACK10) && !want.back().make_selection;
                            longest = std::max<long>(longest, static_cast<long>(want.size()));
                            if (want.size() > kMaxWalk) fail("walk", "longer than kMaxWalk");
                            if (!(want == got)) {
                                std::string s = "class " + std::to_string(cl[0]) + "/" + std::to_string(cl[1]) + "/" + std::to_string(cl[2]) + " prefer " +
                                                std::to_string(prefer) + " chunk " + std::to_string(chunk) + " sel " + std::to_string(sel) + " forced " + std::to_string(forced) +
                                                " crowded " + std::to_string(crowded_first) + ": expected";
                                for (const Visit &v : want) s += " " + name(v.e) + (v.dense_sizing ? "d" : "") + "/" + std::to_string(v.need);
                                s += "; the rule gives";
                                for (const Visit &v : got) s += " " + name(v.e) + (v.dense_sizing ? "d" : "") + "/" + std::to_string(v.need);
                                fail("walk", s);
                            }
                        }
    std::printf("walks %ld (longest %ld candidates; %ld ended behind the packed restart; %ld changed class for the selection bitmap past the first candidate)\n", walks,
                longest, restarts, reclassed_later);
    if (restarts == 0) fail("walk", "no walk took the packed restart");
    if (reclassed_later == 0) fail("walk", "no walk changed class mid-walk");

    if (failures) return std::printf("%ld FAILED\n", failures), 1;
    std::printf("ok %ld\n", picks + members + walks);
    return 0;
}
