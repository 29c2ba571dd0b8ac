// pp_bam_sam_host.h -- the host part of pp_bam_sam (pp_bam_sam.hip): the SAM header text of a BAM header, the reference names as the
// kernels read them, and whether each name can stand in a SAM line.  Plain C++ with no HIP in it, so that a stand-alone program can
// run it under a sanitizer (tools/bam_sam_host_check.cpp).  No byte outside [0, records_at) is read: the header walk is
// pp_bam_host::header over exactly those bytes.  tests/bam_sam_model.py (header_text) states the same rules.
#pragma once
#include "pp_bam_host.h"

#include <algorithm>
#include <string>
#include <vector>

namespace pp_bam_sam_host {

constexpr int OK = 0, ERR_ARG = 4, ERR_LIMIT = 5;  // PP_OK, PP_ERR_ARG, PP_ERR_LIMIT

// can this reference name stand as RNAME / RNEXT / SN and read back as itself?  Not empty, not "*", not "=", bytes 0x21 .. 0x7E
inline bool name_ok(const uint8_t *p, uint32_t n) {
    if (n == 0 || (n == 1 && (p[0] == (uint8_t)'*' || p[0] == (uint8_t)'='))) return false;
    for (uint32_t i = 0; i < n; i++)
        if (p[i] < 0x21 || p[i] > 0x7E) return false;
    return true;
}

struct Header {
    std::string text;               // the output's header lines
    std::vector<uint8_t> names;     // the reference names back to back ...
    std::vector<uint64_t> name_off; // ... name i is names[name_off[i], name_off[i + 1])
    std::vector<uint8_t> ok;        // name_ok of each
};

// bytes[0, records_at) must be a BAM header that ends exactly at records_at
inline int header_text(const uint8_t *bytes, uint64_t records_at, Header *H, char *msg, size_t msg_cap) {
    uint32_t n_ref = 0;
    uint64_t at = 0;
    int rc = pp_bam_host::header(bytes, records_at, 0, &n_ref, nullptr, nullptr, nullptr, &at, msg, msg_cap);
    if (rc != OK && !(rc == ERR_ARG && n_ref)) return ERR_ARG;
    std::vector<uint64_t> off(n_ref);
    std::vector<uint32_t> len(n_ref), ln(n_ref);
    if (n_ref && (rc = pp_bam_host::header(bytes, records_at, n_ref, &n_ref, off.data(), len.data(), ln.data(), &at, msg, msg_cap))) return ERR_ARG;
    if (at != records_at) {
        if (msg && msg_cap) snprintf(msg, msg_cap, "the BAM header ends at %llu, not at records_at %llu", (unsigned long long)at, (unsigned long long)records_at);
        return ERR_ARG;
    }
    uint64_t l_text = pp_bam_host::le32(bytes + 4);
    while (l_text && bytes[8 + l_text - 1] == 0) l_text--;
    H->text.assign((const char *)bytes + 8, (size_t)l_text);
    if (l_text && H->text.back() != '\n') H->text.push_back('\n');
    H->names.clear();
    H->name_off.assign(1, 0);
    H->ok.clear();
    for (uint32_t i = 0; i < n_ref; i++) {
        H->names.insert(H->names.end(), bytes + off[i], bytes + off[i] + len[i]);
        H->name_off.push_back(H->names.size());
        H->ok.push_back(name_ok(bytes + off[i], len[i]) ? 1 : 0);
    }
    bool has_sq = false;  // a line whose first column is exactly "@SQ"
    for (size_t s = 0; s < H->text.size() && !has_sq;) {
        size_t e = H->text.find('\n', s);
        if (e == std::string::npos) e = H->text.size();
        const size_t t = std::min(H->text.find('\t', s), e);
        has_sq = t - s == 3 && H->text.compare(s, 3, "@SQ") == 0;
        s = e + 1;
    }
    if (!has_sq) {
        for (uint32_t i = 0; i < n_ref; i++) {
            if (!H->ok[i] || ln[i] == 0 || ln[i] > 0x7FFFFFFFu) {
                if (msg && msg_cap) snprintf(msg, msg_cap, "reference %llu has no @SQ line (its name or its length %llu)", (unsigned long long)i, (unsigned long long)ln[i]);
                return ERR_LIMIT;
            }
            H->text += "@SQ\tSN:";
            H->text.append((const char *)bytes + off[i], len[i]);
            H->text += "\tLN:" + std::to_string(ln[i]) + "\n";
        }
    }
    return OK;
}

}  // namespace pp_bam_sam_host
