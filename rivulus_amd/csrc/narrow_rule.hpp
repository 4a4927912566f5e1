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
// kNarrowAfterWholeScans / kNarrowFromRows), -1 never, 1 and 2 at the first whole scan whatever the size (2: the packed layout
// below where the rule allows it; 1 never builds it)
inline bool worth_building(int64_t option, const ScanCover &c, uint64_t after_scans, uint64_t from_rows) {
    if (option < 0 || c.extent == 0) return false;
    if (option > 0) return c.whole_scans >= 1;
    return c.whole_scans >= after_scans && c.extent >= from_rows;
}

// a view [offset, offset + rows) can be read from codes that cover `count` elements
inline bool view_covered(uint64_t offset, uint64_t rows, uint64_t count) { return offset + rows <= count && offset + rows >= offset; }

// ---- the packed layout: 10-bit codes, six per 8-byte word --------------------------------------------------------------------------
// A SUPER-GROUP is 384 consecutive elements of the values buffer, from element 384 g, stored as 64 little-endian 8-byte words (512
// bytes).  Word l of it holds the codes of elements 384 g + 128 s + 2 l + h, s in {0, 1, 2}, h in {0, 1}: field k = 2 s + h sits in the
// low dword (k < 3) or the high dword (k >= 3) at bits [10 (k % 3), 10 (k % 3) + 10).  Bits 30 and 31 of both dwords are zero, so no
// field straddles a dword and a row is unpacked with one bit-field extract.  Lane l of a wave that reads word l of consecutive
// super-groups owns rows 2 l, 2 l + 1 of every 128-row group: the row-to-lane mapping of the pair loads of 2- and 4-byte codes, so a
// pass over packed codes ranks, masks and writes out exactly as those do.  Elements past the buffer's count read as code 0.
constexpr uint64_t kPackGroup = 384;      // elements of a super-group
constexpr uint64_t kPackGroupBytes = 512; // bytes of one
constexpr uint32_t kPackBits = 10, kPackMask = 1023;
struct PackedAt {
    uint64_t word;   // index of the 8-byte word in the companion
    uint32_t dword;  // 0: low half of the word, 1: high half
    uint32_t shift;  // bit of the field inside the dword: 0, 10 or 20
};
inline PackedAt packed_at(uint64_t element) {
    const uint64_t g = element / kPackGroup, e = element % kPackGroup;
    const uint32_t s = static_cast<uint32_t>(e / 128), l = static_cast<uint32_t>(e % 128) / 2, h = static_cast<uint32_t>(e & 1);
    const uint32_t k = 2 * s + h;
    return PackedAt{g * 64 + l, k / 3, kPackBits * (k % 3)};
}
// bytes of the packed companion of `count` elements: whole super-groups
inline uint64_t packed_bytes(uint64_t count) { return (count + kPackGroup - 1) / kPackGroup * kPackGroupBytes; }
inline bool packed_width_ok(uint64_t range) { return range <= kPackMask; }
// a view a pass over packed codes can read: a wave range starts on a super-group only when the view does
inline bool packed_view_aligned(uint64_t element_offset) { return element_offset % kPackGroup == 0; }
// the host's pack and unpack of one code (the device kernels do the same with the same arithmetic: tests compare them)
inline void packed_put(uint64_t *words, uint64_t element, uint32_t code) {
    const PackedAt a = packed_at(element);
    words[a.word] |= static_cast<uint64_t>(code & kPackMask) << (32 * a.dword + a.shift);
}
inline uint32_t packed_get(const uint64_t *words, uint64_t element) {
    const PackedAt a = packed_at(element);
    return static_cast<uint32_t>(words[a.word] >> (32 * a.dword + a.shift)) & kPackMask;
}

// ---- which layout is built, and which launch reads which ---------------------------------------------------------------------------
enum class Layout : int { kPlain = 0, kPacked = 1 };  // kPlain: 2- or 4-byte codes, one after the other
// What a launch is, as far as the companions care: its view's first element, and whether it wants per-batch survivor counts (a
// stream's windows: their 1024-row batches are whole wave ranges at 16 rows per lane only, and no packed geometry has that).
struct LaunchKind {
    uint64_t offset;
    bool batch_counts;
};
// a launch that can read a packed companion (it must also be the lean Int64 form and be covered: narrow.hip)
inline bool reads_packed(const LaunchKind &k) { return !k.batch_counts && packed_view_aligned(k.offset); }
// The layout built behind the pass `k` that completed the triggering whole scan: packed when the range fits 10 bits and that pass
// could itself have read packed codes -- a whole-column launch in practice -- else 2- or 4-byte codes as ever.  Option 1 never packs.
inline Layout layout_to_build(int64_t option, uint64_t range, const LaunchKind &k) {
    return (option != 1 && packed_width_ok(range) && reads_packed(k)) ? Layout::kPacked : Layout::kPlain;
}
// A buffer holds at most one companion of each layout.  `have_plain` / `have_packed`: what it holds.  The layout this launch reads
// (`*found` false: none it can read -- the 8-byte values).
inline Layout layout_to_read(const LaunchKind &k, bool have_plain, bool have_packed, bool *found) {
    *found = true;
    if (have_packed && reads_packed(k)) return Layout::kPacked;
    if (have_plain && slice_aligned(k.offset)) return Layout::kPlain;
    *found = false;
    return Layout::kPlain;
}
// The two covers of a buffer.  The first counts every lean pass until the first companion is built; from then on the launches that
// cannot use the companion the buffer has are counted in a second one, and when THEY complete their whole scans the other layout is
// built beside it by the same trigger -- a table scanned whole and later streamed, or the other way round, ends on codes either way.
// Where a finished lean pass is counted:
enum class CountIn : int { kNowhere = 0, kFirst = 1, kSecond = 2 };
inline CountIn count_pass_in(const LaunchKind &k, bool have_plain, bool have_packed) {
    if (!have_plain && !have_packed) return CountIn::kFirst;
    if (have_plain && have_packed) return CountIn::kNowhere;
    bool found = false;
    layout_to_read(k, have_plain, have_packed, &found);
    return found ? CountIn::kNowhere : CountIn::kSecond;
}
// The layout the second cover's trigger builds behind pass `k`, `*build` false: none (the launches it counted can read neither
// layout -- slices at odd elements -- or the packed one is not allowed: not tried again)
inline Layout second_layout(int64_t option, uint64_t range, const LaunchKind &k, bool have_packed, bool *build) {
    if (have_packed) {  // 2-byte codes beside the packed ones (a range of 1023 and less always has them)
        *build = slice_aligned(k.offset);
        return Layout::kPlain;
    }
    *build = layout_to_build(option, range, k) == Layout::kPacked;
    return Layout::kPacked;
}

}  // namespace rvn
