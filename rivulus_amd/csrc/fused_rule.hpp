// Which staged instantiation (fused_table.hpp: ncols, r, vec, waves, flags) serves a launch, and which geometries a launch whose slots
// are crowded tries after it.  Plain C++ for the host: fused_launch.hip decides by it, tests/cpp/fused_rule_tests.cpp holds it to the
// scoring scan it replaced.  It sizes nothing: whether a candidate's slots are crowded is the caller's answer (size_staged).
//   serving_class  the flags and load width of the instantiations that serve (ncols, vec, need)
//   launch_class   ... with the refinements a launch qualifies for (`prefer`) tried first
//   geometry       the member of a class a step of the walk takes
//   Walk           first() / next(): the candidates of one launch, in order
//   holds_exactly  is there an instantiation with exactly these flags, at exactly this forced geometry?
// The registry is read in listed order: the first entry of a class is its default geometry.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

namespace rvf {

// The FF_* values of scan_frontend.hpp the rule reads (that header needs the HIP runtime, so the caller fills them in)
struct Flags {
    int shape;    // what an instantiation must match exactly: FF_ONE_I64 | FF_ONE_F64 | FF_STAMP | FF_PROJALL | FF_NONULL | FF_EXPR | narrow
    int one;      // FF_ONE_I64 | FF_ONE_F64
    int projall, nonull, sel;
    int narrow;   // FF_NARROW16 | FF_NARROW32 | FF_PACK10
    int pack10;
};
struct TallRows {
    int narrow, packed;  // kNarrowTallRows, kPackedTallRows (fused_table.hpp)
};
template <class E>
struct Table {
    const E *e;
    size_t n;
};
constexpr int kAnyRows = 1 << 30;

// option "rows_per_lane" = R | waves << 8 (waves 0: any); <= 0: no geometry forced
template <class E>
bool forced_geometry(const E &e, int64_t forced) {
    const int r = static_cast<int>(forced & 0xFF), waves = static_cast<int>((forced >> 8) & 0xFF);
    return e.r == r && (waves == 0 || e.waves == waves);
}

// per-batch counts out of the pass: a batch must be a whole number of the geometry's wave ranges (64 x rows per lane)
inline bool whole_ranges(uint64_t batch_rows, int r) { return batch_rows % (64u * static_cast<uint64_t>(r)) == 0; }

// ---- the class of a launch ----------------------------------------------------------------------------------------------------
struct Class {
    int flags = 0, vec = 0;
    bool found = false;
};
template <class E>
bool member(const E &e, int ncols, const Class &c) {
    return e.ncols == ncols && (ncols == 0 || e.vec == c.vec) && e.flags == c.flags;
}

// Among the instantiations for ncols columns and this load width whose shape bits are exactly need's and whose features cover it (the
// generic FF_PROJALL forms write the selection bitmap on request: fused_kernel.hpp, kSel): the flags with the fewest bits, the first
// listed on ties.  Every feature set exists with 8-byte loads: vec 1 when there is none with 16-byte loads.
template <class E>
Class serving_class(Table<E> t, const Flags &ff, int ncols, int vec, int need) {
    for (const int v : {vec, 1}) {
        const E *best = nullptr;
        for (size_t i = 0; i < t.n; ++i) {
            const E &e = t.e[i];
            if (e.ncols != ncols || (ncols > 0 && e.vec != v) || (e.flags & ff.shape) != (need & ff.shape)) continue;
            const int has = e.flags | (((e.flags & ff.projall) && !(e.flags & ff.one)) ? ff.sel : 0);
            if ((has & need) != need) continue;
            if (!best || __builtin_popcount(e.flags) < __builtin_popcount(best->flags)) best = &e;
        }
        if (best) return {best->flags, v, true};
    }
    return {};
}
// `prefer`: shape flags worth having when an instantiation exists (FF_PROJALL, FF_NONULL) -- dropped one by one, FF_NONULL first, and
// never at the price of features the launch does not need
template <class E>
Class launch_class(Table<E> t, const Flags &ff, int ncols, int vec, int need, int prefer) {
    int tried = 0;
    for (const int pf : {prefer, prefer & ~ff.nonull}) {
        if (!pf || pf == tried) continue;
        tried = pf;
        const Class c = serving_class(t, ff, ncols, vec, need | pf);
        if (c.found && (c.flags & ~(need | pf)) == 0) return c;
    }
    return serving_class(t, ff, ncols, vec, need);
}

// ---- the geometry a step takes ------------------------------------------------------------------------------------------------
// A launch whose LDS slots would not hold a wave's expected survivors (the caller's `crowded`) walks down:
enum class Step {
    kDefault,     // the first listed geometry -- or the one of `prefer_r` rows per lane, when the class has it
    kBelow,       // the 16-wave geometries with fewer rows per lane than the last one tried, largest first
    kBelowDense,  // the same list again, sized for a dense selection (one workgroup per CU, two stages)
    kFewest       // the fewest waves, then the fewest rows, sized the same way: slots that hold every row of a wave; the last one
};
// The member of class c the step takes; the first listed one when none qualifies (and always for ncols 0, which has one geometry per
// class), none when the class is empty.  A forced geometry overrides every step; of several members that match it, or `prefer_r`, the
// last listed one is taken.
template <class E>
const E *geometry(Table<E> t, int ncols, const Class &c, Step step, int below_r, int64_t forced, int prefer_r) {
    const E *first = nullptr, *pick = nullptr;
    for (size_t i = 0; i < t.n; ++i) {
        const E &e = t.e[i];
        if (!member(e, ncols, c)) continue;
        if (!first) first = &e;
        if (forced > 0) {
            if (forced_geometry(e, forced)) pick = &e;
        } else if (step == Step::kDefault) {
            if (prefer_r > 0 && e.r == prefer_r) pick = &e;
        } else if (ncols < 1) {
            continue;
        } else if (step == Step::kFewest) {
            if (!pick || e.waves < pick->waves || (e.waves == pick->waves && e.r < pick->r)) pick = &e;
        } else if (e.waves == 16 && e.r < below_r && (!pick || e.r > pick->r)) {
            pick = &e;
        }
    }
    return pick ? pick : first;
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------
// The candidates of one launch: first(), then next() while the caller finds the current one crowded and it is not the last().  The
// position is (need, step, below_r); the class is resolved from `need` at every position.
template <class E>
struct Walk {
    Table<E> table;
    Flags ff;
    TallRows tall;
    int ncols, vec, need, prefer;
    int64_t forced;
    bool batch_counts;  // the launch asked for per-batch counts
    Step step = Step::kDefault;
    int below_r = kAnyRows;
    const E *cur = nullptr;

    // (a pass over codes without per-batch counts takes the tall geometry: a 1024-row batch is no whole number of its wave ranges)
    int tall_rows() const { return (need & ff.pack10) ? tall.packed : (((need & ff.narrow) && !batch_counts) ? tall.narrow : 0); }
    const E *resolve(int prefer_r) {
        const Class c = launch_class(table, ff, ncols, vec, need, prefer);
        return cur = c.found ? geometry(table, ncols, c, step, below_r, forced, prefer_r) : nullptr;
    }
    const E *first() { return resolve(tall_rows()); }
    // The launch needs other features after all (the selection bitmap, for a batch that is no whole number of the candidate's wave
    // ranges): the class resolved again, at the position the walk is at.
    const E *reclass(int need_now) {
        need = need_now;
        return resolve(0);
    }
    bool last() const { return step == Step::kFewest || forced > 0 || ncols < 1; }
    bool dense_sizing() const { return step == Step::kBelowDense || step == Step::kFewest; }  // one workgroup per CU, two stages
    // The next candidate after the current one, or none.
    const E *next() {
        if (!cur || last()) return nullptr;
        below_r = cur->r;
        if (step == Step::kDefault) step = Step::kBelow;
        for (;;) {
            const E *e = resolve(0);
            if (!e || (e->waves == 16 && e->r < below_r)) return e;
            // no 16-wave geometry with fewer rows per lane left
            if (step == Step::kBelow) {
                step = Step::kBelowDense;
                below_r = kAnyRows;
            } else if (need & ff.pack10) {
                // denser than the packed class's last geometry admits: the plain lean pass over the 8-byte values, from the top of ITS walk
                need &= ~ff.narrow;
                step = Step::kDefault;
                below_r = kAnyRows;
                return first();
            } else {
                step = Step::kFewest;
                return resolve(0);
            }
        }
    }
};

// ---- exact membership ---------------------------------------------------------------------------------------------------------
template <class E>
bool holds_exactly(Table<E> t, int flags, int64_t forced) {
    for (size_t i = 0; i < t.n; ++i)
        if (t.e[i].flags == flags && (forced <= 0 || forced_geometry(t.e[i], forced))) return true;
    return false;
}

}  // namespace rvf
