// pp_fmt_g.h -- C's printf("%g") of a float32 widened to double, EXACT over all of float32, in integer arithmetic only: host and
// device code (pp_bam_sam.hip prints aux floats with it; tools/bam_sam_host_check.cpp runs it against printf).  No HIP in it.
//
// A finite float is m * 2^e with m < 2^24 and -149 <= e <= 104.  For e >= 0 it is the integer N = m << e; for e < 0 it is
// N / 10^k with N = m * 5^k, k = -e: either way the decimal digits of the integer N (at most 384 bits, twelve 32-bit limbs; at most 112
// digits) are exactly the value's significant digits.  N is divided by 10^9 until nothing is left; of the nine-digit chunks only the
// two highest are kept, and whether anything below them is non-zero.  The six digits "%g" prints are the leading six of N, rounded on
// the digits behind them with ties to even -- the value's exact decimal expansion, so the rounding is printf's.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PP_FMT_HD __host__ __device__
#else
#define PP_FMT_HD
#endif

namespace pp_fmt {

struct Text16 {  // up to sixteen characters, low byte first
    uint64_t lo = 0, hi = 0;
    uint32_t n = 0;
    PP_FMT_HD void put(uint32_t c) {
        if (n < 8u) lo |= (uint64_t)c << (8u * n);
        else if (n < 16u) hi |= (uint64_t)c << (8u * (n - 8u));
        n++;
    }
    PP_FMT_HD uint32_t at(uint32_t i) const { return (uint32_t)((i < 8u ? lo >> (8u * i) : hi >> (8u * (i - 8u))) & 0xFFu); }
};

PP_FMT_HD inline uint32_t digits_of(uint64_t v) {  // decimal digits of v >= 1
    uint32_t n = 1;
    while (v >= 10u) { v /= 10u; n++; }
    return n;
}

PP_FMT_HD inline uint64_t pow10_of(uint32_t k) {  // k <= 18
    uint64_t p = 1;
    for (uint32_t i = 0; i < k; i++) p *= 10u;
    return p;
}

// "%g" of the finite float with these bits (inf and nan: the caller's), at most 13 characters
PP_FMT_HD inline Text16 fmt_g(uint32_t bits) {
    Text16 T;
    if (bits >> 31) T.put('-');
    const uint32_t ef = (bits >> 23) & 0xFFu, mant = bits & 0x7FFFFFu;
    if (ef == 0 && mant == 0) { T.put('0'); return T; }
    uint32_t m = ef ? mant | 0x800000u : mant;
    int e = ef ? (int)ef - 150 : -149;
    while (e < 0 && !(m & 1u)) { m >>= 1; e++; }
    // ---- N = m << e, or m * 5^k
    uint32_t N[12];
    for (int i = 0; i < 12; i++) N[i] = 0;
    uint32_t k = 0, used = 1;  // used: limbs that may be non-zero
    if (e >= 0) {
        const uint32_t w = (uint32_t)e >> 5, s = (uint32_t)e & 31u;
        const uint64_t v = (uint64_t)m << s;
        N[w] = (uint32_t)v;
        N[w + 1] = (uint32_t)(v >> 32);
        used = w + 2u;
    } else {
        k = (uint32_t)-e;
        N[0] = m;
        for (uint32_t left = k; left;) {
            const uint32_t step = left < 13u ? left : 13u;
            uint32_t f = 1;
            for (uint32_t i = 0; i < step; i++) f *= 5u;  // 5^13 < 2^32
            uint64_t carry = 0;
            for (uint32_t i = 0; i < used; i++) {
                const uint64_t v = (uint64_t)N[i] * f + carry;
                N[i] = (uint32_t)v;
                carry = v >> 32;
            }
            if (carry && used < 12u) N[used++] = (uint32_t)carry;
            left -= step;
        }
    }
    // ---- the chunks of nine digits, lowest first: the two highest and whether anything below them is set
    uint64_t top = 0, next = 0;
    uint32_t count = 0;
    bool sticky = false;
    while (used) {
        uint64_t rem = 0;
        for (uint32_t i = used; i-- > 0;) {
            const uint64_t v = rem << 32 | N[i];
            N[i] = (uint32_t)(v / 1000000000u);
            rem = v % 1000000000u;
        }
        while (used && N[used - 1] == 0) used--;
        sticky = sticky || (count >= 2u && next != 0);
        next = top;
        top = rem;
        count++;
    }
    // (top != 0: the loop ends with the highest chunk)
    const uint32_t dt = digits_of(top);
    const uint32_t D = 9u * (count - 1u) + dt;  // the digits of N
    uint64_t L = top;
    uint32_t DL = dt;
    if (count >= 2u) { L = top * 1000000000u + next; DL += 9u; }
    uint64_t d6;
    int X = (int)D - 1 - (int)k;  // the decimal exponent of the first digit
    if (DL <= 6u) d6 = L * pow10_of(6u - DL);
    else {
        const uint64_t p = pow10_of(DL - 6u), rem = L % p, half = p / 2u;
        d6 = L / p;
        if (rem > half || (rem == half && (sticky || (d6 & 1u)))) d6++;
        if (d6 == 1000000u) { d6 = 100000u; X++; }
    }
    uint32_t nd = 6;
    while (nd > 1u && d6 % 10u == 0) { d6 /= 10u; nd--; }
    // digit i of the nd digits, first digit i = 0
    auto digit = [&](uint32_t i) { return (uint32_t)('0' + (d6 / pow10_of(nd - 1u - i)) % 10u); };
    if (X < -4 || X >= 6) {
        T.put(digit(0));
        if (nd > 1u) {
            T.put('.');
            for (uint32_t i = 1; i < nd; i++) T.put(digit(i));
        }
        T.put('e');
        T.put(X < 0 ? '-' : '+');
        const uint32_t a = (uint32_t)(X < 0 ? -X : X);  // at most 45
        T.put('0' + a / 10u);
        T.put('0' + a % 10u);
    } else if (X >= 0) {
        const uint32_t whole = (uint32_t)X + 1u;
        for (uint32_t i = 0; i < whole; i++) T.put(i < nd ? digit(i) : (uint32_t)'0');
        if (nd > whole) {
            T.put('.');
            for (uint32_t i = whole; i < nd; i++) T.put(digit(i));
        }
    } else {
        T.put('0');
        T.put('.');
        for (int i = 0; i < -X - 1; i++) T.put('0');
        for (uint32_t i = 0; i < nd; i++) T.put(digit(i));
    }
    return T;
}

}  // namespace pp_fmt
