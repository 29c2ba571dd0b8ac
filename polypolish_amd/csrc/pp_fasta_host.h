// pp_fasta_host.h -- the host part of pp_fasta_records (pp_fasta.hip): what is proportional to the number of header lines, plain C++
// with no HIP in it, as pp_sam_host.h, so that a stand-alone program can run it under a sanitizer (tools/fasta_host_check.cpp).
// The device hands over, per header line (a line whose first byte is '>'), its offset in the text, its length without the line end
// and the number of sequence bytes in front of it, plus the header lines' bytes packed one behind the other; and the first offending
// sequence byte, if any.  This file restates load_fasta_not_gzipped and check_load_fasta (src/misc.rs:102-133, 56-75) as load_fasta of
// pp_ingest.cpp does, on those: the UTF-8 check of the headers, the split into name and description, unnamed headers merged away, the
// three checks behind the walk.  It reads no byte outside the ranges it is given.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <unordered_set>
#include <vector>

#include "pp_host.h"

namespace pp_fasta_host {

constexpr int OK = 0, ERR_QUIT = 1, ERR_LIMIT = 5;  // PP_OK, PP_ERR_QUIT, PP_ERR_LIMIT

struct Header {  // one header line as the device found it
    uint64_t off;  // of its '>' in the text
    uint64_t len;  // without "\n" and without the "\r" in front of it
    uint64_t pre;  // sequence bytes in front of it
};

struct Contigs {
    std::vector<std::string> names, descs;
    std::vector<uint64_t> off;  // n + 1
};

inline int fail(int code, char *msg, size_t cap, const char *fmt, const char *path) {
    if (msg && cap) snprintf(msg, cap, fmt, path);
    return code;
}

// text[1..].splitn(2, char::is_whitespace) on one header line (valid UTF-8, line[0] == '>')
inline void split_header(const char *line, size_t n, std::string &name, std::string &desc) {
    size_t i = 1, wl = 0;
    while (i < n && !(wl = pph::rust_ws_len(line + i, n - i))) i++;
    name.assign(line + 1, i - 1);
    desc = i < n ? std::string(line + i + wl, n - i - wl) : std::string();
}

// The first header in front of text offset `before` that is not valid UTF-8: its index, or n_hdr.  packed holds the header lines
// one behind the other, header h at the sum of the lengths in front of it.
inline size_t first_bad_header(const char *packed, const Header *h, size_t n_hdr, uint64_t before) {
    uint64_t at = 0;
    for (size_t i = 0; i < n_hdr && h[i].off < before; at += h[i].len, i++)
        if (!pph::valid_utf8(packed + at, (size_t)h[i].len)) return i;
    return n_hdr;
}

// What load_fasta says to an offending sequence line (its bytes without the "\n"; a "\r" at its end is dropped here): `have` is
// whether a named header is open.  OK if it takes the line.
inline int sequence_line(const char *path, const char *line, size_t n, bool have, char *msg, size_t cap) {
    if (n > 0 && line[n - 1] == '\r') n--;
    if (n == 0 || line[0] == '>') return OK;
    const bool utf8 = pph::valid_utf8(line, n);
    if (!have) return utf8 ? fail(ERR_QUIT, msg, cap, "\"%s\" is not correctly formatted", path) : fail(ERR_QUIT, msg, cap, "unable to load \"%s\"", path);
    bool ascii = true;
    for (size_t i = 0; i < n && ascii; i++) ascii = ((unsigned char)line[i] & 0x80u) == 0;
    if (ascii) return OK;
    if (!utf8) return fail(ERR_QUIT, msg, cap, "unable to load \"%s\"", path);
    return fail(ERR_LIMIT, msg, cap, "\"%s\" contains a non-ASCII byte in a sequence line (not supported by this implementation)", path);
}

// The contigs of a text no line of which was refused: every header is valid UTF-8, no sequence byte stands behind an unnamed header
// or in front of the first one.  Unnamed headers open nothing; then check_load_fasta.
inline int contigs(const char *path, const char *packed, const Header *h, size_t n_hdr, uint64_t n_bases, Contigs &c, char *msg, size_t cap) {
    c.names.clear(); c.descs.clear(); c.off.clear();
    uint64_t at = 0;
    std::string name, desc;
    for (size_t i = 0; i < n_hdr; at += h[i].len, i++) {
        split_header(packed + at, (size_t)h[i].len, name, desc);
        if (name.empty()) continue;
        c.names.push_back(name);
        c.descs.push_back(desc);
        c.off.push_back(h[i].pre);
    }
    c.off.push_back(n_bases);
    if (c.names.empty()) return fail(ERR_QUIT, msg, cap, "\"%s\" contains no sequences", path);
    for (size_t i = 0; i < c.names.size(); i++)
        if (c.off[i + 1] == c.off[i]) return fail(ERR_QUIT, msg, cap, "\"%s\" has an empty sequence", path);
    std::unordered_set<std::string> seen;
    for (const std::string &s : c.names)
        if (!seen.insert(s).second) return fail(ERR_QUIT, msg, cap, "\"%s\" has a duplicated name", path);
    return OK;
}

}  // namespace pp_fasta_host
