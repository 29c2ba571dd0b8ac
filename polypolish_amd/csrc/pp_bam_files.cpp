// pp_bam_files.cpp -- pp_aln_file_kind (SAM text, BAM or uncompressed BAM, told by the file's head) and the command drivers' front
// ends for one BAM file and for one file of SAM text (pp_bam_files.h).  Host code over the C ABI only: every alignment byte behind the compressed file is produced
// and consumed on the device by the links this file joins.
#include "pp_bam_files.h"

#include "pp_aln_kind_host.h"

#include <cstdarg>

static_assert(pp_aln_host::SAM == PP_ALN_SAM && pp_aln_host::BAM == PP_ALN_BAM && pp_aln_host::BAM_RAW == PP_ALN_BAM_RAW &&
                  pp_aln_host::SAM_BGZF == PP_ALN_SAM_BGZF, "pp_aln_kind_host.h numbers the kinds as the header does");

extern "C" char *pp_bam_msg_buf_(size_t *cap);  // pp_bam.hip: the per-thread message behind pp_bam_last_error()

namespace {

// up to cap bytes of the file from `at`; -1: the file cannot be read
ssize_t read_at(int fd, uint64_t at, uint8_t *buf, size_t cap) {
    size_t n = 0;
    while (n < cap) {
        const ssize_t r = pread(fd, buf + n, cap - n, (off_t)(at + n));
        if (r < 0) return -1;
        if (r == 0) break;
        n += (size_t)r;
    }
    return (ssize_t)n;
}

// the library's words without the "pp_symbol: " in front of them
const char *words(const char *msg) {
    if (strncmp(msg, "pp_", 3) != 0) return msg;
    const char *c = strstr(msg, ": ");
    return c ? c + 2 : msg;
}

}  // namespace

// pp_aln_file_kind; with_text (pp_aln_file_kind_text): BGZF whose content is not BAM is bgzipped SAM text, not a refusal
static int aln_file_kind(const char *path, int *kind, bool with_text) {
    size_t cap = 0;
    char *msg = pp_bam_msg_buf_(&cap);
    msg[0] = 0;
    if (!path || !kind) {
        snprintf(msg, cap, "%s: null argument", with_text ? "pp_aln_file_kind_text" : "pp_aln_file_kind");
        return PP_ERR_ARG;
    }
    *kind = PP_ALN_SAM;
    auto quit = [&](const char *fmt) {
        snprintf(msg, cap, fmt, path);
        return PP_ERR_QUIT;
    };
    static const char UNABLE[] = "unable to load alignments from \"%s\"";
    static const char NOT_BGZF[] = "\"%s\" is gzip-compressed but not BGZF: of the compressed forms only BAM is read";
    static const char NOT_BAM[] = "\"%s\" is BGZF-compressed but does not hold BAM: SAM text is read uncompressed";
    static const char CUT[] = "\"%s\" begins like a gzip file and ends before a whole gzip header";
    struct stat st;
    if (stat(path, &st) != 0) return quit(UNABLE);
    if (!S_ISREG(st.st_mode)) return PP_OK;  // a pipe is never opened just to look at it: text
    // the walk is pp_aln_kind_host.h's, over a window of the file read with pread
    struct FileSrc {
        int fd;
        std::vector<uint8_t> buf;
        const uint8_t *at(uint64_t off, size_t *n) {
            const ssize_t r = read_at(fd, off, buf.data(), buf.size());
            *n = r < 0 ? 0 : (size_t)r;
            return r < 0 ? nullptr : buf.data();
        }
    } src{open(path, O_RDONLY), std::vector<uint8_t>(pp_aln_host::WINDOW)};
    if (src.fd < 0) return quit(UNABLE);
    const int answer = pp_aln_host::kind_of(src, kind, with_text);
    close(src.fd);
    switch (answer) {
    case pp_aln_host::OK: return PP_OK;
    case pp_aln_host::NOT_BGZF: return quit(NOT_BGZF);
    case pp_aln_host::NOT_BAM: return quit(NOT_BAM);
    case pp_aln_host::CUT: return quit(CUT);
    default: return quit(UNABLE);
    }
}

extern "C" int pp_aln_file_kind(const char *path, int *kind) { return aln_file_kind(path, kind, false); }
extern "C" int pp_aln_file_kind_text(const char *path, int *kind) { return aln_file_kind(path, kind, true); }

namespace ppb {

int fail(pp_ctx *ctx, int code, const char *fmt, ...) {
    char buf[1536];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return pp_ctx_set_error_(ctx, code, buf);
}

void BamFile::drop_records() {
    pp_bam_free(rec);
    rec = nullptr;
    n_decoded = 0;
    pp_bgzf_free(z);
    z = nullptr;
    file.close_file();
    file.fallback = {};
    host_off = {};
    bytes = nullptr;
    rec_off = nullptr;
}

int BamFile::open(pp_ctx *c, const char *p, int k, pp_names *rnames, const pph::Lap *lap) {
    ctx = c;
    path = p;
    kind = k;
    auto lapped = [&](const char *what) {
        if (lap && lap->on) (*lap)((std::string(what) + " " + path).c_str());
    };
    if (!file.open_file(p)) return fail(ctx, PP_ERR_QUIT, "unable to load alignments from \"%s\"", p);
    std::vector<uint8_t> head;  // a prefix of the uncompressed bytes: the header
    const uint8_t *hb = nullptr;
    uint64_t hn = 0;
    if (kind == PP_ALN_BAM) {
        if (int rc = inflate_file(ctx, p, file, &z)) return rc;
        file.close_file();  // the compressed bytes are not needed again
        file.fallback = {};
        pp_bgzf_bytes(z, &bytes, &n_bytes);
        mem = PP_MEM_DEVICE;
        lapped("read + inflated");
    } else {
        bytes = (const uint8_t *)file.text;
        n_bytes = file.size;
        mem = PP_MEM_HOST;
        hb = bytes;
        hn = n_bytes;
    }
    std::vector<uint64_t> name_off;
    std::vector<uint32_t> name_len, ref_len;
    uint32_t cap = 64;
    for (uint64_t prefix = 65536;;) {
        if (kind == PP_ALN_BAM) {
            hn = std::min(prefix, n_bytes);
            head.resize(hn ? hn : 1);
            if (hn)
                if (int rc = pp_ctx_download(ctx, head.data(), bytes, hn)) return rc;
            hb = head.data();
        }
        name_off.resize(cap);
        name_len.resize(cap);
        ref_len.resize(cap);
        const int rc = pp_bam_header(hb, hn, cap, &n_ref, name_off.data(), name_len.data(), ref_len.data(), &records_at);
        if (rc == PP_OK) break;
        if (n_ref > cap) { cap = n_ref; continue; }
        if (hn < n_bytes) { prefix *= 2; continue; }
        return fail(ctx, rc, "invalid BAM header in \"%s\": %s", p, words(pp_bam_last_error()));
    }
    if (rnames) {  // the header's names plus "*" -> contig indices, and distinct ids beyond them for names the assembly lacks
        std::vector<uint8_t> blob;
        std::vector<uint64_t> off(n_ref + 1);
        std::vector<uint32_t> len(n_ref + 1);
        for (uint32_t i = 0; i < n_ref; i++) {
            off[i] = blob.size();
            len[i] = name_len[i];
            blob.insert(blob.end(), hb + name_off[i], hb + name_off[i] + name_len[i]);
        }
        off[n_ref] = blob.size();
        len[n_ref] = 1;
        blob.push_back('*');
        ref_map.assign(n_ref + 1, 0);
        if (int rc = pp_names_ids(rnames, blob.data(), blob.size(), off.data(), len.data(), n_ref + 1, PP_MEM_HOST, nullptr, ref_map.data(), nullptr))
            return rc;
    }
    uint64_t end = 0;
    if (kind == PP_ALN_BAM) {
        if (int rc = pp_bgzf_bam_walk(z, records_at, &n_rec, &end)) {
            if (rc != PP_ERR_ARG) return rc;
            return fail(ctx, rc, "broken record chain in \"%s\" (record %llu): %s", p, (unsigned long long)n_rec + 1, words(pp_bam_last_error()));
        }
        rec_off = pp_bgzf_rec_off(z);
    } else {
        pp_bam_offs *offs = nullptr;
        if (int rc = pp_bam_walk_device(ctx, bytes, n_bytes, records_at, PP_MEM_HOST, &offs, &n_rec, &end)) {
            if (rc != PP_ERR_ARG) return rc;
            return fail(ctx, rc, "broken record chain in \"%s\" (record %llu): %s", p, (unsigned long long)n_rec + 1, words(pp_bam_last_error()));
        }
        host_off.assign(n_rec + 1, 0);  // (never empty: a null rec_off would ask pp_bam_records for a walk of its own)
        const int rc = n_rec ? pp_ctx_download(ctx, host_off.data(), pp_bam_offs_dev(offs), n_rec * 8) : PP_OK;
        pp_bam_offs_free(offs);
        if (rc) return rc;
        rec_off = host_off.data();
    }
    lapped("header + walked");
    return PP_OK;
}

int inflate_file(pp_ctx *ctx, const char *path, const pph::FileText &file, pp_bgzf **z) {
    uint64_t bad = 0;
    const int rc = pp_bgzf_inflate(ctx, (const uint8_t *)file.text, file.size, nullptr, 0, PP_MEM_HOST, z, &bad);
    if (rc != PP_ERR_ARG) return rc;
    const std::string why = words(pp_last_error(ctx));
    return fail(ctx, rc, "invalid BGZF data in \"%s\" (block %llu): %s", path, (unsigned long long)bad + 1, why.c_str());
}

void TextFile::drop_records() {
    pp_sam_free(rec);
    rec = nullptr;
    n_decoded = 0;
    pp_bgzf_free(z);
    z = nullptr;
    file.close_file();
    file.fallback = {};
}

int TextFile::open(pp_ctx *c, const char *p, int k, pp_names *names, const pph::Lap *l) {
    ctx = c;
    path = p;
    kind = k;
    rnames = names;
    lap = l;
    struct stat st;
    if (stat(p, &st) == 0 && !S_ISREG(st.st_mode))
        return fail(ctx, PP_ERR_QUIT, "--text_chain reads regular files: \"%s\" is none (a pipe or a process substitution can be read once, and the replay of the lines in front of a refused one reads the file again)", p);
    return PP_OK;
}

// Read (and inflate) the file, decode its first `limit` lines, intern the names.  The library's sentence about a refused line names
// the path "text": the file's own path in its place.
int TextFile::decode(uint64_t limit, pp_names *qnames, uint64_t *bad) {
    drop_records();
    line_of.clear();
    auto lapped = [&](const char *what) {
        if (lap && lap->on) (*lap)((std::string(what) + " " + path).c_str());
    };
    const char *p = path.c_str();
    if (!file.open_file(p)) return fail(ctx, PP_ERR_QUIT, "unable to load alignments from \"%s\"", p);
    const uint8_t *bytes = (const uint8_t *)file.text;
    uint64_t n_bytes = file.size;
    int mem = PP_MEM_HOST;
    if (kind == PP_ALN_SAM_BGZF) {
        if (int rc = inflate_file(ctx, p, file, &z)) return rc;
        file.close_file();
        file.fallback = {};
        pp_bgzf_bytes(z, &bytes, &n_bytes);
        mem = PP_MEM_DEVICE;
        lapped("read + inflated");
    }
    uint64_t b = ~0ull;
    const int rc = limit == ~0ull ? pp_sam_records(ctx, bytes, n_bytes, mem, &rec, &b) : pp_sam_records_lines(ctx, bytes, n_bytes, mem, limit, &rec, &b);
    if (bad) *bad = b;
    pp_bgzf_free(z);  // the object has its own copy
    z = nullptr;
    file.close_file();
    file.fallback = {};
    if (rc) {
        std::string said = pp_last_error(ctx);
        const size_t at = said.find("\"text\"");
        if (at != std::string::npos) said.replace(at, 6, "\"" + path + "\"");
        else if (rc == PP_ERR_NOT_ASCII) said = "\"" + path + "\" holds bytes outside ASCII, which the text chain does not read";
        return pp_ctx_set_error_(ctx, rc, said.c_str());
    }
    pp_raw_batch view;
    pp_sam_raw(rec, &view);
    n_decoded = view.n_rec;
    if (!n_decoded) return PP_OK;
    line_of.resize((size_t)n_decoded);
    if (int rd = pp_ctx_download(ctx, line_of.data(), pp_sam_lines(rec), n_decoded * 4)) return rd;
    const uint8_t *nb = nullptr;
    uint64_t nn = 0;
    const uint64_t *noff = nullptr;
    const uint32_t *nlen = nullptr;
    pp_sam_rnames(rec, &nb, &nn, &noff, &nlen);
    if (int rn = pp_names_ids(rnames, nb, nn, noff, nlen, n_decoded, PP_MEM_DEVICE, nullptr, pp_sam_contig(rec), nullptr)) return rn;
    pp_sam_names(rec, &nb, &nn, &noff, &nlen);
    return pp_names_ids(qnames, nb, nn, noff, nlen, n_decoded, PP_MEM_DEVICE, pp_sam_read_id(rec), nullptr, nullptr);
}

int BamFile::decode(uint64_t limit, pp_names *qnames, uint64_t *bad) {
    pp_bam_free(rec);
    rec = nullptr;
    n_decoded = 0;
    uint64_t b = 0;
    const int rc = pp_bam_records(ctx, bytes, n_bytes, rec_off, limit, mem, ref_map.empty() ? nullptr : ref_map.data(), n_ref, &rec, &b);
    if (bad) *bad = b;
    if (rc) {
        const unsigned long long n1 = (unsigned long long)b + 1;
        const std::string why = pp_last_error(ctx);
        if (rc == PP_ERR_QUIT) return fail(ctx, rc, "missing NM tag in \"%s\" (record %llu)", path.c_str(), n1);
        if (rc == PP_ERR_PANIC) return fail(ctx, rc, "negative NM tag in \"%s\" (record %llu): the reference panics on parse::<u32>", path.c_str(), n1);
        if (rc == PP_ERR_ARG) return fail(ctx, rc, "invalid BAM record in \"%s\" (record %llu): %s", path.c_str(), n1, words(why.c_str()));
        return rc;
    }
    n_decoded = limit;
    if (!limit) return PP_OK;
    const uint8_t *nb = nullptr;
    uint64_t nn = 0;
    const uint64_t *noff = nullptr;
    const uint32_t *nlen = nullptr;
    pp_bam_names(rec, &nb, &nn, &noff, &nlen);
    return pp_names_ids(qnames, nb, nn, noff, nlen, limit, PP_MEM_DEVICE, pp_bam_read_id(rec), nullptr, nullptr);
}

int download_groups(const Front &B, uint64_t n, std::vector<uint16_t> &flag, std::vector<uint64_t> &read_id) {
    flag.assign(n ? n : 1, 0);
    read_id.assign(n ? n : 1, 0);
    if (!n) return PP_OK;
    pp_raw_batch raw;
    B.raw(&raw);
    if (int rc = pp_ctx_download(B.ctx, flag.data(), raw.flag, n * 2)) return rc;
    return pp_ctx_download(B.ctx, read_id.data(), raw.read_id, n * 8);
}

int file_kind(pp_ctx *ctx, const char *path, int *kind) {
    const int rc = pp_ctx_text_chain_(ctx) ? pp_aln_file_kind_text(path, kind) : pp_aln_file_kind(path, kind);
    if (rc == PP_ERR_QUIT && strncmp(pp_bam_last_error(), "unable to load", 14) == 0) {
        *kind = PP_ALN_SAM;
        return PP_OK;
    }
    return rc ? pp_ctx_set_error_(ctx, rc, pp_bam_last_error()) : PP_OK;
}

int seed_names(pp_names *t, const pp_assembly *a) {
    const uint32_t nc = pp_assembly_n_contigs(a);
    std::vector<uint8_t> blob;
    std::vector<uint64_t> off(nc ? nc : 1);
    std::vector<uint32_t> len(nc ? nc : 1), id(nc ? nc : 1);
    for (uint32_t c = 0; c < nc; c++) {
        const char *name = pp_assembly_name(a, c);
        off[c] = blob.size();
        len[c] = (uint32_t)strlen(name);
        blob.insert(blob.end(), name, name + len[c]);
    }
    if (blob.empty()) blob.push_back(0);
    return pp_names_ids(t, blob.data(), blob.size(), off.data(), len.data(), nc, PP_MEM_HOST, nullptr, id.data(), nullptr);
}

std::string name_of(const pp_names *t, uint64_t id) {
    uint32_t len = 0;
    std::vector<uint8_t> buf(256);
    int rc = pp_names_name(t, id, buf.data(), (uint32_t)buf.size(), &len);
    if (rc && len > buf.size()) {
        buf.resize(len);
        rc = pp_names_name(t, id, buf.data(), (uint32_t)buf.size(), &len);
    }
    return rc ? std::string("?") : std::string((const char *)buf.data(), len);
}

}  // namespace ppb
