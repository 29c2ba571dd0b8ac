// pp_depth_host.h -- the host part of pp_depth_bedgraph and pp_polish_depth (pp_k_depth.h, pp_polish_text.hip): plain C++ with no HIP in
// it, as pp_bed_host.h (whose name table, offset checks, job checks and digit helpers it uses), so that a stand-alone program can run
// it under a sanitizer (tools/depth_host_check.cpp).  It holds the argument checks, the bins' table, the rounding of a bin's mean and
// the arithmetic of one bedGraph line -- its length and its k-th byte -- as constexpr functions: the kernels call the very same ones,
// so the digit widths the GPU tests cannot reach are checked on the CPU.  tests/depth_model.py defines the bytes.
#pragma once
#include "pp_bed_host.h"

namespace pp_depth_host {

using pp_bed_host::digit;
using pp_bed_host::ERR_ARG;
using pp_bed_host::ERR_LIMIT;
using pp_bed_host::fail;
using pp_bed_host::ndig;
using pp_bed_host::OK;

constexpr uint32_t BIN_MAX = 1u << 24;                    // the widest bin
constexpr uint64_t DEPTH_BAD_BITS = 0x41F0000000000000ull;  // the bits of 2^32 as a double: a depth's bits lie below them, as an unsigned
                                                            // number (a set sign bit, -0.0 too, a NaN and an infinity lie above)
constexpr uint64_t TENTHS_MAX = 10ull << 32;              // tenths of the largest double below 2^32 (it rounds up)

// ---- one line: name \t start \t end \t value \n --------------------------------------------------------------------------------
// value: v with `frac` decimals -- the runs form writes tenths (frac 1), the bins form hundredths (frac 2)
constexpr uint64_t pow10_of(uint32_t frac) { return frac == 1u ? 10u : 100u; }
constexpr uint32_t value_len(uint64_t v, uint32_t frac) { return ndig(v / pow10_of(frac)) + 1u + frac; }
constexpr uint64_t line_len(uint64_t name_len, uint64_t a, uint64_t b, uint64_t v, uint32_t frac) {
    return name_len + ndig(a) + ndig(b) + value_len(v, frac) + 4u;
}
// pp_bed_host::digit, in 32-bit arithmetic where the number fits (starts, ends and all but the largest values do: on the device a
// 64-bit division by ten costs several times a 32-bit one, and the text pass makes one per digit and byte)
constexpr uint32_t digit_of(uint64_t v, uint32_t behind) {
    if (v > 0xFFFFFFFFull) return digit(v, behind);
    uint32_t w = (uint32_t)v;
    for (; behind > 0u; behind--) w /= 10u;
    return (uint32_t)'0' + w % 10u;
}
// byte k of the line (k < line_len): na = ndig(a), nb = ndig(b), nv = value_len(v, frac)
constexpr uint32_t line_byte(const uint8_t *name, uint64_t name_len, uint64_t a, uint32_t na, uint64_t b, uint32_t nb, uint64_t v, uint32_t nv,
                             uint32_t frac, uint64_t k) {
    if (k < name_len) return name[k];
    k -= name_len;
    if (k == 0u) return (uint32_t)'\t';
    k -= 1u;
    if (k < na) return digit_of(a, na - 1u - (uint32_t)k);
    k -= na;
    if (k == 0u) return (uint32_t)'\t';
    k -= 1u;
    if (k < nb) return digit_of(b, nb - 1u - (uint32_t)k);
    k -= nb;
    if (k == 0u) return (uint32_t)'\t';
    k -= 1u;
    if (k >= nv) return (uint32_t)'\n';
    const uint32_t behind = nv - 1u - (uint32_t)k;  // bytes of the value behind this one
    if (behind == frac) return (uint32_t)'.';
    return digit_of(v, behind > frac ? behind - 1u : behind);
}

// the mean of n tenths whose sum is S, in hundredths, ties to even: 10 S / n rounded (S < 2^60, 1 <= n <= 2^24)
constexpr uint64_t mean_hundredths(uint64_t S, uint64_t n) {
    const uint64_t q = 10u * S / n, r = 10u * S % n;
    return q + ((2u * r > n || (2u * r == n && (q & 1u))) ? 1u : 0u);
}

// ---- the calls' arguments ------------------------------------------------------------------------------------------------------
struct Plan {
    pp_bed_host::Plan names;         // the name table and G
    std::vector<uint64_t> bin_base;  // bins form: n + 1 entries, the first record of each contig (bin_base[n]: the records); else empty
};

// Judged in this order: null arguments, the memory kind, the bin, the alignment of a device array, then what pp_status_bed judges of
// the offsets and the names.  have_depth: the pointer is not null; aligned: a device array lies on a multiple of 8 bytes.
inline int plan(const char *who, bool have_out, bool have_depth, bool mem_ok, bool aligned, uint32_t n, const uint64_t *contig_off,
                const char *const *names, uint32_t bin, Plan &P, char *msg, size_t cap) {
    P = Plan();
    if (!have_out || !have_depth || !names || !contig_off) return fail(ERR_ARG, msg, cap, who, "null argument");
    if (!mem_ok) return fail(ERR_ARG, msg, cap, who, "the depths are PP_MEM_HOST or PP_MEM_DEVICE");
    if (bin > BIN_MAX) return fail(ERR_ARG, msg, cap, who, "a bin of more than 2^24 positions");
    if (!aligned) return fail(ERR_ARG, msg, cap, who, "a device array of depths that is not aligned to 8 bytes");
    if (int rc = pp_bed_host::plan(who, true, true, true, n, contig_off, names, pp_bed_host::MASK_ALL, P.names, msg, cap)) return rc;
    if (bin) {
        P.bin_base.assign((size_t)n + 1, 0);
        for (uint32_t c = 0; c < n; c++) P.bin_base[c + 1] = P.bin_base[c] + (contig_off[c + 1] - contig_off[c] + bin - 1u) / bin;
    }
    return OK;
}

}  // namespace pp_depth_host
