// Fixed-point number text for the overlays, one statement for host and device: the string Python's "%.{d}f" % v gives
// for d = 0, 1, 2, and the decimal text of an int32.  No libc formatting (there is none on the device), no tables.
//
// Contract: exact for every double with |v| < 1e9, -0.0 and results that round to zero from below included
// ("%.1f" % -0.04 is "-0.0"), ties decided half-to-even on the exact binary value; NaN -> "nan", +-inf -> "inf" / "-inf";
// a finite |v| >= 1e9 is written as "inf" / "-inf".  Nothing is written when the text does not fit `cap` characters
// (no terminator is added); the return value is then -1, else the length.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AV_FMT_HD __host__ __device__ inline
#else
#define AV_FMT_HD inline
#endif

namespace fmtnum {

constexpr int MAX_FIXED = 16;      // longest text of fmt_fixed: '-' + 12 digits + '.' (< 16)
constexpr int MAX_INT = 11;        // "-2147483648"

AV_FMT_HD int put(const char* s, int n, char* out, int cap) {
    if (n > cap) return -1;
    for (int k = 0; k < n; ++k) out[k] = s[k];
    return n;
}

AV_FMT_HD int fmt_int(int32_t v, char* out, int cap) {
    char t[MAX_INT];
    uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    int n = 0;
    do { t[MAX_INT - 1 - n++] = (char)('0' + u % 10u), u /= 10u; } while (u);
    if (v < 0) t[MAX_INT - 1 - n++] = '-';
    return put(t + MAX_INT - n, n, out, cap);
}

AV_FMT_HD int fmt_fixed(double v, int decimals, char* out, int cap) {
    if (decimals < 0 || decimals > 2) return -1;
    if (v != v) return put("nan", 3, out, cap);
    const bool neg = std::signbit(v);
    const double a = std::fabs(v);
    if (!(a < 1e9)) return neg ? put("-inf", 4, out, cap) : put("inf", 3, out, cap);
    // n = a * 10^d rounded to an integer, half to even, on the exact product: p is the rounded product, e its exact residual
    const double m = decimals == 0 ? 1.0 : decimals == 1 ? 10.0 : 100.0;
    const double p = a * m, e = std::fma(a, m, -p);
    const double q = std::floor(p), t = (p - q) - 0.5;          // both subtractions are exact (p < 2^37)
    uint64_t n = (uint64_t)q;
    if (t > 0.0 || (t == 0.0 && e > 0.0)) n += 1;
    else if (t == 0.0 && e == 0.0) n += n & 1u;
    char s[MAX_FIXED];
    int k = MAX_FIXED;
    for (int dgt = 0; dgt < decimals; ++dgt) s[--k] = (char)('0' + n % 10u), n /= 10u;
    if (decimals) s[--k] = '.';
    do { s[--k] = (char)('0' + n % 10u), n /= 10u; } while (n);
    if (neg) s[--k] = '-';
    return put(s + k, MAX_FIXED - k, out, cap);
}

}  // namespace fmtnum
