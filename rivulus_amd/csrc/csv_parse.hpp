// Cell parsers of the device CSV scan (csv_kernels.hpp), written once for the device and the host: plain g++ compiles
// this header for the CPU fuzz test (tests/cpp/csv_parse_fuzz.cpp), hipcc for the kernels.
//
// The rule is the host CsvFileStream's (rivulus_host.hpp): trim the ASCII isspace set, "" / "null" is a null cell, then
//   Int64    optional sign, one or more digits, overflow is an error               (str::parse::<i64>, strtoll)
//   Boolean  true / t / 1 / false / f / 0, ASCII case-insensitive
//   Float64  [+-] (inf | infinity | nan, any case | digits [. digits] | . digits) [(e|E) [+-] digits], no hex,
//            correctly rounded (strtod / Rust's dec2flt), "-nan" keeps its sign as strtod does.
// Float64 goes in three steps, the way dec2flt does: the exact fast path (w <= 2^53, |e| small), Eisel-Lemire over a
// 128-bit table of powers of five (19 significant digits; longer mantissas are truncated and tried at w and w + 1), and
// for whatever that cannot decide the exact decimal slow path (parse_f64_slow: ~800 bytes of digits, so the kernels
// call it from a kernel of its own).
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RVCSV_HD __host__ __device__ inline
#define RVCSV_TABLE_QUALIFIER static __device__
#else
#define RVCSV_HD inline
#define RVCSV_TABLE_QUALIFIER static
#endif

#include "csv_pow5_table.hpp"

namespace rvcsv {

// the ASCII isspace set: space, \t \n \v \f \r
RVCSV_HD bool is_space(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }
RVCSV_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
RVCSV_HD uint8_t lower(uint8_t c) { return (c >= 'A' && c <= 'Z') ? static_cast<uint8_t>(c + 32) : c; }

// [*b, *e) -> trimmed in place
RVCSV_HD void trim(const uint8_t *s, uint32_t *b, uint32_t *e) {
    uint32_t x = *b, y = *e;
    while (x < y && is_space(s[x])) ++x;
    while (y > x && is_space(s[y - 1])) --y;
    *b = x;
    *e = y;
}

RVCSV_HD bool is_null_cell(const uint8_t *s, uint32_t n) {
    return n == 0 || (n == 4 && s[0] == 'n' && s[1] == 'u' && s[2] == 'l' && s[3] == 'l');
}

RVCSV_HD bool parse_i64(const uint8_t *s, uint32_t n, int64_t *out) {
    uint32_t i = 0;
    bool neg = false;
    if (n > 0 && (s[0] == '+' || s[0] == '-')) neg = s[i++] == '-';
    if (i == n) return false;
    const uint64_t limit = neg ? (uint64_t(1) << 63) : (uint64_t(1) << 63) - 1;
    uint64_t acc = 0;
    for (; i < n; ++i) {
        if (!is_digit(s[i])) return false;
        const uint64_t d = s[i] - '0';
        if (acc > (limit - d) / 10) return false;  // acc * 10 + d > limit
        acc = acc * 10 + d;
    }
    *out = neg ? static_cast<int64_t>(0 - acc) : static_cast<int64_t>(acc);
    return true;
}

RVCSV_HD bool parse_bool(const uint8_t *s, uint32_t n, bool *out) {
    if (n == 1) {
        const uint8_t c = lower(s[0]);
        if (c == 't' || c == '1') return *out = true, true;
        if (c == 'f' || c == '0') return *out = false, true;
        return false;
    }
    if (n == 4 && lower(s[0]) == 't' && lower(s[1]) == 'r' && lower(s[2]) == 'u' && lower(s[3]) == 'e') return *out = true, true;
    if (n == 5 && lower(s[0]) == 'f' && lower(s[1]) == 'a' && lower(s[2]) == 'l' && lower(s[3]) == 's' && lower(s[4]) == 'e')
        return *out = false, true;
    return false;
}

// ---- Float64 ----------------------------------------------------------------------------------------------------------
enum F64Status : uint32_t { kF64Ok = 0, kF64Bad = 1, kF64Slow = 2 };

RVCSV_HD bool ieq(const uint8_t *s, uint32_t n, const char *lit) {  // ASCII case-insensitive, lit lowercase
    for (uint32_t i = 0; i < n; ++i)
        if (lit[i] == 0 || lower(s[i]) != static_cast<uint8_t>(lit[i])) return false;
    return lit[n] == 0;
}

RVCSV_HD uint64_t mul_hi(uint64_t a, uint64_t b, uint64_t *lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    *lo = a * b;
    return __umul64hi(a, b);
#else
    const unsigned __int128 p = static_cast<unsigned __int128>(a) * b;
    *lo = static_cast<uint64_t>(p);
    return static_cast<uint64_t>(p >> 64);
#endif
}

RVCSV_HD int clz64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll(x);
#else
    return __builtin_clzll(x);
#endif
}

RVCSV_HD double bits_to_double(uint64_t b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
}

// Biased binary exponent and explicit mantissa bits; e < 0: undecided.
struct BiasedFp {
    uint64_t f;
    int32_t e;
};

// Eisel-Lemire: w * 10^q, w != 0, correctly rounded, or e = -1 when the 128-bit product cannot decide
RVCSV_HD BiasedFp eisel_lemire(int64_t q, uint64_t w) {
    if (w == 0 || q < kPow5MinQ) return {0, 0};
    if (q > kPow5MaxQ) return {0, 0x7FF};
    const int lz = clz64(w);
    w <<= lz;
    const int idx = 2 * static_cast<int>(q - kPow5MinQ);
    const uint64_t mask = ~uint64_t(0) >> 55;  // 52 explicit bits + 3
    uint64_t lo;
    uint64_t hi = mul_hi(w, kPow5Table[idx], &lo);
    if ((hi & mask) == mask) {
        uint64_t lo2;
        const uint64_t hi2 = mul_hi(w, kPow5Table[idx + 1], &lo2);
        lo += hi2;
        if (hi2 > lo) ++hi;
    }
    if (lo == ~uint64_t(0) && !(q >= -27 && q <= 55)) return {0, -1};
    const int upper = static_cast<int>(hi >> 63);
    const int shift = upper + 64 - 52 - 3;
    uint64_t m = hi >> shift;
    int32_t p2 = static_cast<int32_t>((((152170 + 65536) * q) >> 16) + 63) + upper - lz + 1023;
    if (p2 <= 0) {  // subnormal
        if (-p2 + 1 >= 64) return {0, 0};
        m >>= -p2 + 1;
        m += m & 1;
        m >>= 1;
        return {m, m >= (uint64_t(1) << 52) ? 1 : 0};
    }
    if (lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << shift) == hi) m &= ~uint64_t(1);  // exact tie: round to even
    m += m & 1;
    m >>= 1;
    if (m >= (uint64_t(2) << 52)) {
        m = uint64_t(1) << 52;
        ++p2;
    }
    m &= ~(uint64_t(1) << 52);
    if (p2 >= 0x7FF) return {0, 0x7FF};
    return {m, p2};
}

constexpr int kMaxExp = 0x10000;  // explicit exponents saturate here (anything beyond is 0 or inf anyway)

// The grammar; on success the significant digits as dec2flt's Number: w (first 19 significant digits), q (w * 10^q),
// many (more than 19 significant digits), the mantissa span [m0, m1) and the explicit exponent.
struct F64Syntax {
    bool neg;
    uint8_t special;  // 0 number, 1 inf, 2 nan
    bool many;
    uint64_t w;
    int64_t q;
    uint32_t m0, m1;  // mantissa digits and '.', relative to the cell
    int32_t exp;      // explicit exponent, saturated
};

RVCSV_HD bool f64_syntax(const uint8_t *s, uint32_t n, F64Syntax *o) {
    uint32_t i = 0;
    o->neg = false;
    o->special = 0;
    o->many = false;
    if (n > 0 && (s[0] == '+' || s[0] == '-')) o->neg = s[i++] == '-';
    const uint32_t r = n - i;
    if (r > 0 && !is_digit(s[i]) && s[i] != '.') {
        if (ieq(s + i, r, "inf") || ieq(s + i, r, "infinity")) return o->special = 1, true;
        if (ieq(s + i, r, "nan")) return o->special = 2, true;
        return false;
    }
    o->m0 = i;
    uint64_t w = 0;
    int ndig = 0;         // significant digits seen (leading zeros excluded)
    int64_t q = 0;        // decimal exponent of w's last digit
    int64_t dropped = 0;  // significant integer digits beyond the 19 kept
    uint32_t digits = 0;
    for (; i < n && is_digit(s[i]); ++i, ++digits) {
        if (ndig == 0 && s[i] == '0') continue;
        if (ndig < 19) w = w * 10 + (s[i] - '0');
        else ++dropped;
        ++ndig;
    }
    q += dropped;
    if (i < n && s[i] == '.') {
        for (++i; i < n && is_digit(s[i]); ++i, ++digits) {
            if (ndig == 0 && s[i] == '0') {
                --q;
                continue;
            }
            if (ndig < 19) {
                w = w * 10 + (s[i] - '0');
                --q;
            }
            ++ndig;
        }
    }
    if (digits == 0) return false;
    o->m1 = i;
    int32_t ex = 0;
    if (i < n && (s[i] == 'e' || s[i] == 'E')) {
        ++i;
        bool eneg = false;
        if (i < n && (s[i] == '+' || s[i] == '-')) eneg = s[i++] == '-';
        uint32_t ed = 0;
        for (; i < n && is_digit(s[i]); ++i, ++ed)
            if (ex < kMaxExp) ex = ex * 10 + (s[i] - '0');
        if (ed == 0) return false;
        if (eneg) ex = -ex;
    }
    if (i != n) return false;
    o->exp = ex;
    o->w = w;
    o->q = q + ex;
    o->many = ndig > 19;
    return true;
}

RVCSV_HD double pow10_exact(int e) {  // 10^0 .. 10^22 are exact doubles
    double p = 1.0;
    for (int k = 0; k < e; ++k) p *= 10.0;
    return p;
}

RVCSV_HD uint64_t f64_bits(bool neg, BiasedFp fp) {
    return (neg ? uint64_t(1) << 63 : 0) | (static_cast<uint64_t>(fp.e) << 52) | fp.f;
}

// kF64Ok: *out holds the value; kF64Bad: not a Float64; kF64Slow: valid, but only parse_f64_slow decides it
RVCSV_HD F64Status parse_f64(const uint8_t *s, uint32_t n, double *out) {
    F64Syntax x;
    if (!f64_syntax(s, n, &x)) return kF64Bad;
    const uint64_t sign = x.neg ? uint64_t(1) << 63 : 0;
    if (x.special == 1) return *out = bits_to_double(sign | 0x7FF0000000000000ull), kF64Ok;
    if (x.special == 2) return *out = bits_to_double(sign | 0x7FF8000000000000ull), kF64Ok;
    if (x.w == 0) return *out = bits_to_double(sign), kF64Ok;
    if (!x.many && x.w <= (uint64_t(1) << 53) && x.q >= -22 && x.q <= 22) {  // exact: one correctly rounded operation
        double v = static_cast<double>(x.w);
        v = x.q < 0 ? v / pow10_exact(static_cast<int>(-x.q)) : v * pow10_exact(static_cast<int>(x.q));
        *out = x.neg ? -v : v;
        return kF64Ok;
    }
    BiasedFp fp = eisel_lemire(x.q, x.w);
    if (x.many && fp.e >= 0) {
        const BiasedFp up = eisel_lemire(x.q, x.w + 1);
        if (up.e != fp.e || up.f != fp.f) fp.e = -1;
    }
    if (fp.e < 0) return kF64Slow;
    *out = bits_to_double(f64_bits(x.neg, fp));
    return kF64Ok;
}

// ---- exact slow path: decimal shifting over up to 768 digits (dec2flt's parse_long_mantissa) --------------------------
struct Decimal {
    static constexpr int kMaxDigits = 768;
    static constexpr int kPointRange = 2047;
    int32_t num_digits;
    int32_t point;
    bool truncated;
    uint8_t d[kMaxDigits + 24];  // room for the digits a left shift adds before they are moved into place

    RVCSV_HD void strip() {
        while (num_digits != 0 && d[num_digits - 1] == 0) --num_digits;
    }
    RVCSV_HD uint64_t round() const {
        if (num_digits == 0 || point < 0) return 0;
        if (point > 18) return ~uint64_t(0);
        uint64_t n = 0;
        for (int i = 0; i < point; ++i) n = n * 10 + (i < num_digits ? d[i] : 0);
        bool up = false;
        if (point < num_digits) {
            up = d[point] >= 5;
            if (d[point] == 5 && point + 1 == num_digits) up = truncated || (point != 0 && (d[point - 1] & 1));
        }
        return n + (up ? 1 : 0);
    }
    RVCSV_HD void left_shift(int shift) {  // * 2^shift, shift <= 60
        if (num_digits == 0) return;
        const int room = ((shift * 1233) >> 12) + 1;  // >= the digits the shift adds
        int r = num_digits, w = num_digits + room;
        uint64_t n = 0;
        while (r != 0) {
            --r;
            --w;
            n += static_cast<uint64_t>(d[r]) << shift;
            const uint64_t qt = n / 10;
            d[w] = static_cast<uint8_t>(n - 10 * qt);
            n = qt;
        }
        while (n > 0) {
            --w;
            const uint64_t qt = n / 10;
            d[w] = static_cast<uint8_t>(n - 10 * qt);
            n = qt;
        }
        const int added = room - w;  // the digits start at w >= 0
        int total = num_digits + added;
        for (int k = 0; k < total; ++k) d[k] = d[k + w];
        if (total > kMaxDigits) {
            for (int k = kMaxDigits; k < total; ++k)
                if (d[k]) truncated = true;
            total = kMaxDigits;
        }
        num_digits = total;
        point += added;
        strip();
    }
    RVCSV_HD void right_shift(int shift) {  // / 2^shift, shift <= 60
        int r = 0, w = 0;
        uint64_t n = 0;
        while ((n >> shift) == 0) {
            if (r < num_digits) {
                n = 10 * n + d[r++];
            } else if (n == 0) {
                return;
            } else {
                while ((n >> shift) == 0) {
                    n *= 10;
                    ++r;
                }
                break;
            }
        }
        point -= r - 1;
        if (point < -kPointRange) {
            num_digits = 0;
            point = 0;
            truncated = false;
            return;
        }
        const uint64_t mask = (uint64_t(1) << shift) - 1;
        while (r < num_digits) {
            const uint8_t nd = static_cast<uint8_t>(n >> shift);
            n = 10 * (n & mask) + d[r++];
            d[w++] = nd;
        }
        while (n > 0) {
            const uint8_t nd = static_cast<uint8_t>(n >> shift);
            n = 10 * (n & mask);
            if (w < kMaxDigits) d[w++] = nd;
            else if (nd > 0) truncated = true;
        }
        num_digits = w;
        strip();
    }
};

// the digits of a cell that f64_syntax accepted as a number
RVCSV_HD void decimal_from(const uint8_t *s, const F64Syntax &x, Decimal *dec) {
    dec->num_digits = 0;
    dec->point = 0;
    dec->truncated = false;
    int32_t all = 0;  // digits added, kept or not
    int32_t int_digits = 0;
    bool seen_point = false, any = false;
    int32_t frac_lead_zeros = 0;
    for (uint32_t i = x.m0; i < x.m1; ++i) {
        const uint8_t c = s[i];
        if (c == '.') {
            seen_point = true;
            continue;
        }
        if (!any && c == '0') {
            if (seen_point) ++frac_lead_zeros;
            continue;
        }
        any = true;
        if (all < Decimal::kMaxDigits) dec->d[all] = static_cast<uint8_t>(c - '0');
        else if (c != '0') dec->truncated = true;
        ++all;
        if (!seen_point) ++int_digits;
    }
    if (all == 0) return;
    // point: digits before the decimal point, counted from the first significant digit
    int32_t point = int_digits > 0 ? int_digits : -frac_lead_zeros;
    int32_t kept = all < Decimal::kMaxDigits ? all : Decimal::kMaxDigits;
    dec->num_digits = kept;
    dec->strip();
    int64_t p = static_cast<int64_t>(point) + x.exp;
    if (p > 100000) p = 100000;
    if (p < -100000) p = -100000;
    dec->point = static_cast<int32_t>(p);
}

RVCSV_HD int slow_shift(int n) {
    const uint8_t powers[19] = {0, 3, 6, 9, 13, 16, 19, 23, 26, 29, 33, 36, 39, 43, 46, 49, 53, 56, 59};
    return n < 19 ? powers[n] : 60;
}

// exact value of a cell parse_f64 returned kF64Slow for; `dec` is caller-provided room (~800 bytes)
RVCSV_HD double parse_f64_slow(const uint8_t *s, uint32_t n, Decimal *dec) {
    F64Syntax x;
    f64_syntax(s, n, &x);
    decimal_from(s, x, dec);
    Decimal &d = *dec;
    BiasedFp fp{0, 0};
    int32_t exp2 = 0;
    if (d.num_digits == 0 || d.point < -324) return bits_to_double(f64_bits(x.neg, {0, 0}));
    if (d.point >= 310) return bits_to_double(f64_bits(x.neg, {0, 0x7FF}));
    while (d.point > 0) {
        const int sh = slow_shift(d.point);
        d.right_shift(sh);
        if (d.point < -Decimal::kPointRange) return bits_to_double(f64_bits(x.neg, {0, 0}));
        exp2 += sh;
    }
    while (d.point <= 0) {
        int sh;
        if (d.point == 0) {
            if (d.d[0] >= 5) break;
            sh = d.d[0] < 2 ? 2 : 1;
        } else {
            sh = slow_shift(-d.point);
        }
        d.left_shift(sh);
        if (d.point > Decimal::kPointRange) return bits_to_double(f64_bits(x.neg, {0, 0x7FF}));
        exp2 -= sh;
    }
    exp2 -= 1;
    while (-1023 + 1 > exp2) {
        int k = (-1023 + 1) - exp2;
        if (k > 60) k = 60;
        d.right_shift(k);
        exp2 += k;
    }
    if (exp2 + 1023 >= 0x7FF) return bits_to_double(f64_bits(x.neg, {0, 0x7FF}));
    d.left_shift(53);
    uint64_t m = d.round();
    if (m >= (uint64_t(1) << 53)) {
        d.right_shift(1);
        ++exp2;
        m = d.round();
        if (exp2 + 1023 >= 0x7FF) return bits_to_double(f64_bits(x.neg, {0, 0x7FF}));
    }
    int32_t p2 = exp2 + 1023;
    if (m < (uint64_t(1) << 52)) --p2;
    fp.f = m & ((uint64_t(1) << 52) - 1);
    fp.e = p2;
    return bits_to_double(f64_bits(x.neg, fp));
}

}  // namespace rvcsv
