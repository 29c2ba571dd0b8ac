// pp_vcf_host.h -- the host part of pp_polish_vcf (pp_k_vcf.h, pp_polish_text.hip): what is proportional to the number of contigs, plain
// C++ with no HIP in it, as pp_fasta_out_host.h, so that a stand-alone program can run it under a sanitizer
// (tools/vcf_host_check.cpp).  plan() judges the caller's arguments and the state of the context's job, and builds the VCF header and
// the name table the kernels read.  tests/vcf_model.py defines the bytes.  It reads contig_off[0, n], names[0, n) and every name up
// to its NUL, and nothing else.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace pp_vcf_host {

constexpr int OK = 0, ERR_ARG = 4, ERR_LIMIT = 5;  // PP_OK, PP_ERR_ARG, PP_ERR_LIMIT
constexpr uint64_t TEXT_LIMIT = 1ull << 40;        // a text of this many bytes or more is refused

struct JobState {  // of the context the call is made on
    bool finished;   // a pp_polish_finish succeeded and no pp_polish_begin followed (a job that ended in an error leaves none)
    bool emit_set;   // pp_polish_set_emit ranges: a rank's share has no defined runs at its edges
};

struct Plan {
    std::string header;              // the "##" lines and the column line
    std::string names;               // the contig names, one behind the other ...
    std::vector<uint64_t> name_off;  // ... n + 1 offsets into them
};

inline int fail(int code, char *msg, size_t cap, const char *what) {
    if (msg && cap) snprintf(msg, cap, "pp_polish_vcf: %s", what);
    return code;
}

// Judged in this order: null arguments, the job's state (then its contig table), a null name, a name that holds a tab or a newline
// (ERR_ARG), then the header's size (ERR_LIMIT: the text would have 2^40 bytes or more whatever the records are).
inline int plan(bool have_out, const JobState &S, uint32_t n, const uint64_t *contig_off, const char *const *names, const char *version, Plan &P,
                char *msg, size_t cap) {
    P = Plan();
    if (!have_out || !names || !version) return fail(ERR_ARG, msg, cap, "null argument");
    if (!S.finished) return fail(ERR_ARG, msg, cap, "no finished polish job on this context (a job that ended in an error leaves none)");
    if (S.emit_set) return fail(ERR_ARG, msg, cap, "the context has pp_polish_set_emit ranges: a rank's share has no defined runs at its edges");
    if (!contig_off) return fail(ERR_ARG, msg, cap, "null argument");  // (a context that never had a job has no table: said above)
    P.name_off.assign((size_t)n + 1, 0);
    uint64_t total = 96 + strlen(version);  // (an upper bound of the three fixed lines)
    for (uint32_t c = 0; c < n; c++) {
        if (!names[c]) return fail(ERR_ARG, msg, cap, "a contig name is NULL");
        const size_t len = strlen(names[c]);
        if (memchr(names[c], '\t', len) || memchr(names[c], '\n', len)) return fail(ERR_ARG, msg, cap, "a contig name that holds a tab or a newline");
        P.name_off[c + 1] = P.name_off[c] + len;
        total += len + 48;  // (an upper bound of the contig's header line)
        if (total >= TEXT_LIMIT) return fail(ERR_LIMIT, msg, cap, "a text of 2^40 bytes or more");
    }
    P.names.reserve((size_t)P.name_off[n]);
    P.header.reserve((size_t)total);
    P.header += "##fileformat=VCFv4.2\n##source=";
    P.header += version;
    P.header += '\n';
    char num[48];
    for (uint32_t c = 0; c < n; c++) {
        P.names += names[c];
        P.header += "##contig=<ID=";
        P.header += names[c];
        snprintf(num, sizeof num, ",length=%llu>\n", (unsigned long long)(contig_off[c + 1] - contig_off[c]));
        P.header += num;
    }
    P.header += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
    return OK;
}

// the header and the records' bytes together (the records' size is known once the device has scanned them)
inline int text_size(uint64_t n_header, uint64_t n_records_bytes, uint64_t *n_text, char *msg, size_t cap) {
    if (n_records_bytes >= TEXT_LIMIT || n_header + n_records_bytes >= TEXT_LIMIT) return fail(ERR_LIMIT, msg, cap, "a text of 2^40 bytes or more");
    *n_text = n_header + n_records_bytes;
    return OK;
}

}  // namespace pp_vcf_host
