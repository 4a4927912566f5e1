// The host-side rule of the narrow companions (runtime.hpp, NarrowCodes; narrow.hip): range arithmetic, code width, the alignment a
// slice needs, which buffers qualify, and when a buffer has been scanned often enough to be worth packing.  Plain C++ without the
// runtime: tests/cpp/narrow_host_tests.cpp builds it on the CPU.
#pragma once
#include <cstdint>

namespace rvn {

// max - min of a column as an unsigned difference: INT64_MIN .. INT64_MAX gives 2^64 - 1, no signed overflow
inline uint64_t value_range(int64_t lo, int64_t hi) { return static_cast<uint64_t>(hi) - static_cast<uint64_t>(lo); }

// bytes of a code that holds every value - min of that range; 0: no companion (the range needs more than 32 bits)
inline int code_bytes(uint64_t range) { return range <= 0xFFFFull ? 2 : (range <= 0xFFFFFFFFull ? 4 : 0); }

// code of one value (what narrow_pack_kernel stores) and its way back (what the pass computes)
inline uint32_t encode(int64_t value, int64_t base) { return static_cast<uint32_t>(static_cast<uint64_t>(value) - static_cast<uint64_t>(base)); }
inline int64_t decode(uint32_t code, int64_t base) { return static_cast<int64_t>(static_cast<uint64_t>(base) + code); }

// A pass reads the codes of rows 2l, 2l + 1 with one load of 2 x code bytes: the slice's first element must be even (4-byte loads
// of 2-byte codes, 8-byte loads of 4-byte codes; the companion itself starts on a 256-byte boundary)
inline bool slice_aligned(uint64_t element_offset) { return (element_offset & 1) == 0; }

// Only Int64 values in a pool block (id != 0: the library allocated it and nothing writes to it once its column's handle is out;
// caller-owned memory behind rv_wrap has id 0) of a column without a null bitmap
inline bool buffer_eligible(uint64_t buffer_id, bool is_int64, bool has_validity) { return buffer_id != 0 && is_int64 && !has_validity; }

// What the lean passes have read of a values buffer.  `extent`: elements the buffer's columns span (the longest view seen: the
// column itself, or the parent of a slice); a WHOLE scan is complete when passes over adjoining or overlapping views, in ascending
// order from element 0, have reached it -- one pass over the column, or a stream's windows one after the other.  A slice read again and
// again never completes one.
struct ScanCover {
    uint64_t extent = 0, covered_to = 0, whole_scans = 0;
    void note_extent(uint64_t end) {
        if (end > extent) extent = end;
    }
    void note_pass(uint64_t offset, uint64_t rows) {
        note_extent(offset + rows);
        if (offset > covered_to) return;  // a gap: not part of a scan from the start
        if (offset + rows > covered_to) covered_to = offset + rows;
        if (extent && covered_to >= extent) {
            whole_scans += 1;
            covered_to = 0;
        }
    }
};

// option "narrow_codes": 0 auto (after `after_scans` whole scans of a buffer of `from_rows` elements and more: thresholds.hpp,
// kNarrowAfterWholeScans / kNarrowFromRows), -1 never, 1 at the first whole scan whatever the size
inline bool worth_building(int64_t option, const ScanCover &c, uint64_t after_scans, uint64_t from_rows) {
    if (option < 0 || c.extent == 0) return false;
    if (option > 0) return c.whole_scans >= 1;
    return c.whole_scans >= after_scans && c.extent >= from_rows;
}

// a view [offset, offset + rows) can be read from codes that cover `count` elements
inline bool view_covered(uint64_t offset, uint64_t rows, uint64_t count) { return offset + rows <= count && offset + rows >= offset; }

}  // namespace rvn
