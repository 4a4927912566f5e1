// Fuzz check of the CSV cell parsers (rivulus_amd/csrc/csv_parse.hpp) on the host: every generated cell is parsed by
//   * the device parser (compiled here by g++),
//   * the host CsvFileStream's rule (rivulus_host.hpp: the character pre-check, then strtoll / strtod),
//   * the oracle's grammar (oracle/oracle_csv.hpp: rust_parse_i64 / rust_parse_f64),
// and the three must agree: same accept / reject, same bits.  The one known difference: rust_parse_f64 drops the sign of
// "-nan", which strtod (and Rust) keep -- the device follows strtod.  Prints one line per group and "ok <cells>" at the end.
#include <algorithm>
#include <cerrno>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../oracle/oracle_csv.hpp"
#include "../../rivulus_amd/csrc/csv_parse.hpp"

namespace {

uint64_t bits(double d) {
    uint64_t b;
    std::memcpy(&b, &d, 8);
    return b;
}

// host CsvFileStream::parse_line, Int64 / Float64 arms
bool host_i64(const std::string &f, int64_t &out) {
    size_t k = (f[0] == '+' || f[0] == '-') ? 1 : 0;
    bool ok = k < f.size();
    for (size_t q = k; q < f.size(); ++q) ok = ok && std::isdigit(static_cast<unsigned char>(f[q]));
    errno = 0;
    char *end = nullptr;
    const long long v = ok ? std::strtoll(f.c_str(), &end, 10) : 0;
    if (!ok || errno == ERANGE || *end) return false;
    out = v;
    return true;
}
bool host_f64(const std::string &f, double &out) {
    bool ok = true;
    for (char ch : f) ok = ok && (std::isalnum(static_cast<unsigned char>(ch)) || ch == '+' || ch == '-' || ch == '.');
    if (f.find_first_of("xXpP") != std::string::npos) ok = false;
    char *end = nullptr;
    const double v = ok ? std::strtod(f.c_str(), &end) : 0.0;
    if (!ok || end == f.c_str() || *end) return false;
    out = v;
    return true;
}

uint64_t g_cells = 0, g_slow = 0, g_fail = 0;
rvcsv::Decimal g_dec;

void fail(const char *what, const std::string &s, const char *detail) {
    if (g_fail++ < 20) std::printf("FAIL %s: '%s' %s\n", what, s.size() > 200 ? (s.substr(0, 200) + "...").c_str() : s.c_str(), detail);
}

void check_f64(const std::string &s) {
    ++g_cells;
    double hv = 0, dv = 0, ov = 0;
    const bool h = host_f64(s, hv);
    const bool o = rvo::rust_parse_f64(s, ov);
    const auto *p = reinterpret_cast<const uint8_t *>(s.data());
    rvcsv::F64Status st = rvcsv::parse_f64(p, static_cast<uint32_t>(s.size()), &dv);
    if (st == rvcsv::kF64Slow) {
        ++g_slow;
        dv = rvcsv::parse_f64_slow(p, static_cast<uint32_t>(s.size()), &g_dec);
    }
    const bool d = st != rvcsv::kF64Bad;
    if (h != d) return fail("f64 accept", s, h ? "host accepts, device rejects" : "device accepts, host rejects");
    if (h != o) return fail("f64 grammar", s, h ? "oracle rejects" : "oracle accepts");
    if (!h) return;
    if (bits(hv) != bits(dv)) {
        char b[96];
        std::snprintf(b, sizeof b, "host %016" PRIx64 " device %016" PRIx64, bits(hv), bits(dv));
        return fail("f64 bits", s, b);
    }
    if (!std::isnan(hv) && bits(hv) != bits(ov)) return fail("f64 oracle bits", s, "");
}

// every slow-path cell also parsed only through the slow path must give the same value (the slow path is exact for all)
void check_slow_direct(const std::string &s) {
    double hv = 0;
    if (!host_f64(s, hv) || std::isnan(hv) || std::isinf(hv)) return;
    rvcsv::F64Syntax x;
    const auto *p = reinterpret_cast<const uint8_t *>(s.data());
    if (!rvcsv::f64_syntax(p, static_cast<uint32_t>(s.size()), &x) || x.special) return;
    ++g_cells;
    const double dv = rvcsv::parse_f64_slow(p, static_cast<uint32_t>(s.size()), &g_dec);
    if (bits(hv) != bits(dv)) fail("f64 slow path", s, "");
}

void check_i64(const std::string &s) {
    ++g_cells;
    int64_t hv = 0, dv = 0, ov = 0;
    const bool h = host_i64(s, hv);
    const bool o = rvo::rust_parse_i64(s, ov);
    const bool d = rvcsv::parse_i64(reinterpret_cast<const uint8_t *>(s.data()), static_cast<uint32_t>(s.size()), &dv);
    if (h != d) return fail("i64 accept", s, h ? "host accepts" : "device accepts");
    if (h != o) return fail("i64 grammar", s, "");
    if (h && (hv != dv || hv != ov)) fail("i64 value", s, "");
}

void check_bool(const std::string &s) {
    ++g_cells;
    std::string l = s;
    for (auto &ch : l) ch = static_cast<char>(std::tolower(static_cast<unsigned char>(ch)));
    const bool ht = l == "true" || l == "t" || l == "1", hf = l == "false" || l == "f" || l == "0";
    bool dv = false;
    const bool d = rvcsv::parse_bool(reinterpret_cast<const uint8_t *>(s.data()), static_cast<uint32_t>(s.size()), &dv);
    if (d != (ht || hf) || (d && dv != ht)) fail("bool", s, "");
}

std::string digits(std::mt19937_64 &rng, int n, bool lead_nonzero) {
    std::string s;
    for (int i = 0; i < n; ++i) s.push_back(static_cast<char>('0' + ((i == 0 && lead_nonzero) ? 1 + rng() % 9 : rng() % 10)));
    return s;
}

double random_double(std::mt19937_64 &rng) {
    for (;;) {
        const double d = [&] {
            const uint64_t b = rng();
            double x;
            std::memcpy(&x, &b, 8);
            return x;
        }();
        if (std::isfinite(d)) return d;
    }
}

std::string fmt(const char *f, int prec, long double v) {
    char buf[1024];
    std::snprintf(buf, sizeof buf, f, prec, v);
    return buf;
}

}  // namespace

int main(int argc, char **argv) {
    const uint64_t target = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 10000000ull;
    std::mt19937_64 rng(20261016);

    // fixed cases: boundaries and malformed input
    const char *fixed_f[] = {"2.4703282292062327e-324", "2.4703282292062328e-324", "2.4703282292062326e-324", "4.9406564584124654e-324",
                             "2.2250738585072011e-308", "2.2250738585072014e-308", "1.7976931348623157e308", "1.7976931348623158e308",
                             "1.7976931348623159e308", "1e-400", "1e400", "-1e400", "0e999999999", "0.000e-99999", "000000.0000e5",
                             "0001.5", ".5", "5.", "-.5", "+5.", "inf", "-inf", "+INF", "Infinity", "-iNfInItY", "nan", "-nan", "+NaN",
                             "1e", ".", "+", "-", "1_0", "0x1p3", "0X10", "nan(1)", "infinit", "infinityy", "nana", "1e+", "1e-", "e5",
                             "1.2.3", "1e5.5", "--1", "+-1", "1-", "9007199254740993", "9007199254740992.5", "123456789012345678901234567890",
                             "0.1", "0.2", "0.3", "1e22", "1e23", "9.007199254740993e15", "7.2057594037927933e16", "1e-22", "1e-23",
                             "2.225073858507201136057409796709131975934819546351645648e-308",
                             "4.4501477170144022721148195934182639518696390927032912960468522194496444440421538910330590478162701758282983178260792422137401728773891892910553144148156412434867599762821265346585071045737627442980259622449029037796981144446145705102663115100318287949527959668236039986479250965780342141637013812613333119898765515451440315261253813266652951306000184917766328660755595837392240989947807556594098101021612198814605258742579179000071675999344145086087205681577915435923018910334964869420614052182892431445797605163650903606514140377217442262561590244668525767372446430075513332450079650686719491377688478005309963967709758965844137894433796621993967316936280457084866613206797017728916080020698679408551343728867675409720757232455434770912461317493580281734466552734375e-308",
                             "1448997445238699", "18446744073709551615", "18446744073709551616e-30", "1e-45", "3.4028236e38"};
    for (const char *s : fixed_f) check_f64(s);
    const char *fixed_i[] = {"9223372036854775807", "9223372036854775808", "-9223372036854775808", "-9223372036854775809", "+0", "-0", "0000000000000000000000000001",
                             "+", "-", "1_0", "1.0", "1e3", "99999999999999999999", "--1", "+-1", " 1", "0x10"};
    for (const char *s : fixed_i) check_i64(s);
    const char *fixed_b[] = {"true", "TRUE", "True", "t", "T", "1", "false", "FaLsE", "f", "F", "0", "yes", "no", "2", "tru", "falsey", "truE"};
    for (const char *s : fixed_b) check_bool(s);
    const uint64_t slow_before_random = g_slow;

    const char alphabet[] = "0123456789+-.eEinfatyINFATYxp_ ";
    uint64_t groups[8] = {};
    while (g_cells < target) {
        const int kind = static_cast<int>(rng() % 100);
        if (kind < 25) {  // shortest / 15-17 digit forms of random doubles
            const double d = random_double(rng);
            check_f64(fmt("%.*Le", 14 + static_cast<int>(rng() % 4), d));
            groups[0]++;
        } else if (kind < 37) {  // near halfway points: the midpoint of two neighbours, to 17-40 digits, +- one ulp of the last digit
            const double d = std::fabs(random_double(rng));
            const long double mid = (static_cast<long double>(d) + static_cast<long double>(std::nextafter(d, INFINITY))) / 2;
            std::string s = fmt("%.*Le", 16 + static_cast<int>(rng() % 24), mid);
            check_f64(s);
            groups[1]++;
        } else if (kind < 38) {  // exact halfway points (every digit of the midpoint)
            const double d = std::ldexp(static_cast<double>(rng() >> 11), static_cast<int>(rng() % 200) - 150);
            const long double mid = (static_cast<long double>(d) + static_cast<long double>(std::nextafter(d, INFINITY))) / 2;
            std::string s = fmt("%.*Le", 200, mid);
            check_f64(s);
            check_slow_direct(s);
            groups[2]++;
            if (rng() % 4 == 0) {  // the same point with a tail past the slow path's 768 digits: zeros (still a tie) or a 1 (above it)
                const size_t e = s.find('e');
                std::string mant = s.substr(0, e);
                while (mant.back() == '0') mant.pop_back();
                const std::string tail = std::string(780 + rng() % 40, '0');
                check_f64(mant + tail + s.substr(e));
                check_f64(mant + tail + "1" + s.substr(e));
                check_slow_direct(mant + tail + "1" + s.substr(e));
                groups[7]++;
            }
        } else if (kind < 40) {  // subnormals and the underflow edge
            const double d = std::ldexp(static_cast<double>(rng() >> (12 + rng() % 50)), -1074);
            check_f64(fmt("%.*Le", 15 + static_cast<int>(rng() % 25), d));
            check_f64(fmt("%.*Le", 16, static_cast<long double>(d) * (1.0L + ((rng() & 1) ? 1e-17L : -1e-17L))));
            groups[3]++;
        } else if (kind < 60) {  // random decimal forms: long mantissas, leading zeros, huge exponents
            std::string s;
            if (rng() % 4 == 0) s.push_back(rng() % 2 ? '-' : '+');
            s += std::string(rng() % 3, '0');
            const int a = static_cast<int>(rng() % 24), b = static_cast<int>(rng() % 24);
            s += digits(rng, a, false);
            if (rng() % 3 || a == 0) s += "." + digits(rng, b, false);
            if (rng() % 2) {
                s += (rng() % 2) ? "e" : "E";
                if (rng() % 2) s.push_back(rng() % 2 ? '-' : '+');
                const int r = static_cast<int>(rng() % 10);
                s += std::to_string(r < 6 ? rng() % 30 : (r < 9 ? rng() % 400 : rng() % 100000));
            }
            check_f64(s);
            if (rng() % 16 == 0) check_slow_direct(s);
            groups[4]++;
        } else if (kind < 80) {  // Int64: random values, boundaries, digit strings
            std::string s;
            const int r = static_cast<int>(rng() % 4);
            if (r == 0) s = std::to_string(static_cast<int64_t>(rng()));
            else if (r == 1) s = std::to_string(static_cast<int64_t>(rng()) >> (rng() % 63));
            else if (r == 2) s = std::string(rng() % 2 ? "-" : "") + digits(rng, 1 + static_cast<int>(rng() % 22), rng() % 2);
            else s = (rng() % 2 ? "-922337203685477580" : "922337203685477580") + std::to_string(rng() % 10);
            check_i64(s);
            groups[5]++;
        } else {  // garbage from the number alphabet: every parser, grammar agreement
            std::string s;
            const int n = 1 + static_cast<int>(rng() % 10);
            for (int i = 0; i < n; ++i) s.push_back(alphabet[rng() % (sizeof(alphabet) - 1)]);
            if (s.front() == ' ' || s.back() == ' ') continue;  // cells arrive trimmed
            check_f64(s);
            check_i64(s);
            check_bool(s);
            groups[6]++;
        }
    }
    std::printf("groups: doubles %" PRIu64 ", near-halfway %" PRIu64 ", exact-halfway %" PRIu64 ", subnormal %" PRIu64 ", decimal forms %" PRIu64
                ", int64 %" PRIu64 ", garbage %" PRIu64 ", halfway + a tail past 768 digits %" PRIu64 "\n",
                groups[0], groups[1], groups[2], groups[3], groups[4], groups[5], groups[6], groups[7]);
    if (groups[7] == 0) {
        std::printf("FAIL no cell longer than the slow path's digit buffer\n");
        return 1;
    }
    std::printf("slow path: %" PRIu64 " cells (%" PRIu64 " of them random)\n", g_slow, g_slow - slow_before_random);
    if (g_slow - slow_before_random == 0) {
        std::printf("FAIL the random cells never reached the slow path\n");
        return 1;
    }
    if (g_fail) {
        std::printf("FAIL %" PRIu64 " mismatches in %" PRIu64 " cells\n", g_fail, g_cells);
        return 1;
    }
    std::printf("ok %" PRIu64 " cells\n", g_cells);
    return 0;
}
