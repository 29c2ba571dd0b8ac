// pp_cli.cpp -- `polypolish`, a drop-in for the reference binary's command line
// (src/main.rs:23-126): same subcommands, flag names, short flags, defaults, stdout/stderr split
// and exit codes (0 ok, 1 "Error: ...", 2 usage, 101 where the reference would panic).
// All work happens in libpolypolish_hip.so on an MI355X; there is no CPU path.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

#include "polypolish_hip.h"
#include "pp_host.h"
#include "pp_bed_host.h"

static const char *HELP =
    "Polypolish (MI355X/gfx950 implementation, parity target v0.6.1)\n"
    "short-read polishing of long-read assemblies\n\n"
    "Usage: polypolish <COMMAND>\n\n"
    "Commands:\n"
    "  filter  filter paired-end alignments based on insert size\n"
    "  polish  polish a long-read assembly using short-read alignments\n"
    "  filter-polish  both in one process, without the intermediate SAM files (not in the reference)\n\n"
    "Options:\n  -h, --help     Print help\n  -V, --version  Print version\n";

static const char *HELP_FILTER =
    "filter paired-end alignments based on insert size\n\n"
    "Usage: polypolish filter [OPTIONS] --in1 <IN1> --in2 <IN2> --out1 <OUT1> --out2 <OUT2>\n\n"
    "Options:\n"
    "      --in1 <IN1>                  Input SAM file - first read in pairs\n"
    "      --in2 <IN2>                  Input SAM file - first second in pairs\n"
    "      --out1 <OUT1>                Output SAM file - first read in pairs\n"
    "      --out2 <OUT2>                Output SAM file - first second in pairs\n"
    "                                   (two BAM inputs are read as they are and give two BAM outputs)\n"
    "      --out_bam                    SAM text inputs: write the outputs as compressed BAM (not in the reference)\n"
    "      --out_sam                    BAM inputs: write the outputs as SAM text (not in the reference)\n"
    "      --text_chain                 SAM text inputs, plain or bgzipped, through the record chain on the device (not in the reference)\n"
    "      --sort_out                   BAM outputs: write them in coordinate order, header SO:coordinate (not in the reference)\n"
    "      --out_bai                    with --sort_out: write OUT1.bai and OUT2.bai next to the outputs (not in the reference)\n"
    "      --orientation <ORIENTATION>  Expected pair orientation [default: auto]\n"
    "      --low <LOW>                  Low percentile threshold [default: 0.1]\n"
    "      --high <HIGH>                High percentile threshold [default: 99.9]\n"
    "  -h, --help                       Print help\n  -V, --version                    Print version\n";

static const char *HELP_POLISH =
    "polish a long-read assembly using short-read alignments\n\n"
    "Usage: polypolish polish [OPTIONS] <ASSEMBLY> [SAM]...\n\n"
    "Arguments:\n  <ASSEMBLY>  Assembly to polish (one file in FASTA format)\n"
    "  [SAM]...    Short read alignments (one or more files in SAM format, or all of them in BAM format)\n\n"
    "Options:\n"
    "      --debug <DEBUG>                        Optional file to store per-base information for debugging purposes\n"
    "  -i, --fraction_invalid <FRACTION_INVALID>  A base must make up less than this fraction of the read depth to be considered invalid [default: 0.2]\n"
    "  -v, --fraction_valid <FRACTION_VALID>      A base must make up at least this fraction of the read depth to be considered valid [default: 0.5]\n"
    "  -m, --max_errors <MAX_ERRORS>              Ignore alignments with more than this many mismatches and indels [default: 10]\n"
    "  -d, --min_depth <MIN_DEPTH>                A base must occur at least this many times in the pileup to be considered valid [default: 5]\n"
    "      --careful                              Ignore any reads with multiple alignments\n"
    "      --regroup                              BAM files whose reads do not stand together (coordinate-sorted): bring every read's alignments together first\n"
    "      --text_chain                           SAM text, plain or bgzipped, through the record chain on the device; --regroup then takes text as well (not in the reference)\n"
    "      --out <PATH>                           Write the polished FASTA to PATH instead of stdout (not in the reference)\n"
    "      --wrap <N>                             Line width of the polished FASTA, made on the device; 0: one line per contig (not in the reference)\n"
    "      --out_bgzf                             Compress the polished FASTA into BGZF blocks on the device (not in the reference)\n"
    "      --index                                With --out: write PATH.fai, and PATH.gzi with --out_bgzf (not in the reference)\n"
    "      --vcf <PATH>                           Write the polish's edits to PATH as VCF 4.2, made on the device (one GPU; not in the reference)\n"
    "      --vcf_bgzf                             With --vcf: compress the VCF into BGZF blocks on the device (not in the reference)\n"
    "      --bed <PATH>                           Write the runs of undecided positions to PATH as BED, made on the device (one GPU; not in the reference)\n"
    "      --bed_bgzf                             With --bed: compress the BED into BGZF blocks on the device (not in the reference)\n"
    "      --soft_mask                            Write the bases of undecided positions in lower case (one GPU; not in the reference)\n"
    "      --bed_status <LIST>                    The statuses --bed and --soft_mask select: a comma-separated list of kept, changed,\n"
    "                                             low_depth, none, multiple, too_close [default: low_depth,none,multiple,too_close]\n"
    "      --depth <PATH>                         Write the read depth to PATH as bedGraph, made on the device (one GPU; not in the reference)\n"
    "      --depth_bin <N>                        With --depth: the mean depth of bins of N positions; 0: runs of equal depth [default: 0] (not in the reference)\n"
    "      --depth_bgzf                           With --depth: compress the bedGraph into BGZF blocks on the device (not in the reference)\n"
    "      --vcf_tbi                              With --vcf_bgzf: write PATH.tbi, the tabix index of the VCF, made on the device (not in the reference)\n"
    "      --bed_tbi                              With --bed_bgzf: write PATH.tbi, the tabix index of the BED, made on the device (not in the reference)\n"
    "      --depth_tbi                            With --depth_bgzf: write PATH.tbi, the tabix index of the bedGraph, made on the device (not in the reference)\n"
    "  -h, --help                                 Print help\n  -V, --version                              Print version\n";

static const char *HELP_FUSED =
    "filter paired-end alignments by insert size and polish with them, in one process\n\n"
    "Usage: polypolish filter-polish [OPTIONS] --in1 <IN1> --in2 <IN2> <ASSEMBLY>\n\n"
    "Options: those of `filter` (--out1/--out2 optional: write the tagged SAMs as well) and of `polish`.\n"
    "The FASTA on stdout is byte-identical to `filter` followed by `polish` on its outputs.\n"
    "--in1/--in2 are both SAM text or both BAM; with BAM the optional outputs are BAM as well.\n"
    "--regroup: coordinate-sorted BAM inputs (the polish brings every read's alignments together; the outputs keep file order).\n"
    "--out_bam: SAM text inputs with --out1/--out2: write the outputs as compressed BAM.\n"
    "--out_sam: BAM inputs with --out1/--out2: write the outputs as SAM text.\n"
    "--sort_out: BAM outputs in coordinate order, header SO:coordinate; --out_bai: with it, OUT1.bai and OUT2.bai (not in the reference).\n"
    "--text_chain: SAM text inputs, plain or bgzipped, through the record chain on the device; --regroup then takes text as well (not in the reference).\n"
    "--out <PATH>: write the polished FASTA to PATH instead of stdout (not in the reference).\n"
    "--wrap <N>: line width of the polished FASTA, made on the device; 0: one line per contig (not in the reference).\n"
    "--out_bgzf: compress the polished FASTA into BGZF blocks on the device (not in the reference).\n"
    "--index: with --out, write PATH.fai, and PATH.gzi with --out_bgzf (not in the reference).\n"
    "--vcf <PATH>: write the polish's edits to PATH as VCF 4.2, made on the device (not in the reference).\n"
    "--vcf_bgzf: with --vcf, compress the VCF into BGZF blocks on the device (not in the reference).\n"
    "--bed <PATH>: write the runs of undecided positions to PATH as BED, made on the device (not in the reference).\n"
    "--bed_bgzf: with --bed, compress the BED into BGZF blocks on the device (not in the reference).\n"
    "--soft_mask: write the bases of undecided positions in lower case (not in the reference).\n"
    "--bed_status <LIST>: the statuses --bed and --soft_mask select, a comma-separated list of kept, changed, low_depth, none,\n"
    "multiple, too_close; default low_depth,none,multiple,too_close (not in the reference).\n"
    "--depth <PATH>: write the read depth to PATH as bedGraph, made on the device (not in the reference).\n"
    "--depth_bin <N>: with --depth, the mean depth of bins of N positions; 0, the default: runs of equal depth (not in the reference).\n"
    "--depth_bgzf: with --depth, compress the bedGraph into BGZF blocks on the device (not in the reference).\n"
    "--vcf_tbi, --bed_tbi, --depth_tbi: with --vcf_bgzf, --bed_bgzf, --depth_bgzf, write the track's tabix index to PATH.tbi, made on\n"
    "the device (not in the reference).\n";

static int usage_error(const char *msg) {
    fprintf(stderr, "error: %s\n\nFor more information, try '--help'.\n", msg);
    return 2;
}

static bool parse_f64(const char *s, double &v) {
    char *e = nullptr;
    v = strtod(s, &e);
    return e && *e == 0 && e != s;
}
static bool parse_u32(const char *s, uint32_t &v) {
    if (!*s) return false;
    char *e = nullptr;
    if (*s == '-') return false;
    unsigned long long x = strtoull(s, &e, 10);
    if (!e || *e != 0 || x > 0xFFFFFFFFull) return false;
    v = (uint32_t)x;
    return true;
}

// ---- clap's argument grammar (the reference derives its parser with clap 4.4, src/main.rs:23-109) ----------------
//   --name value | --name=value | -x value | -xvalue | -x=value | flags clustered (-hV) | "--" ends the options |
//   a lone "-" is a positional | an option given twice is an error | unknown options are errors.
struct OptSpec {
    const char *long_name;   // "--min_depth"
    char short_name;         // 'd', or 0
    bool takes_value;
    const char *value_name;  // "<MIN_DEPTH>" (error texts)
};

struct Parsed {
    std::vector<const char *> value;  // per option: the value (flags: "" when present), nullptr when absent
    std::vector<const char *> positional;
    int help = 0, version = 0;
    std::string error;                // non-empty: usage error (exit 2)
};

static std::string opt_display(const OptSpec &o) {
    std::string d = o.long_name;
    if (o.takes_value) { d += ' '; d += o.value_name; }
    return d;
}

static bool looks_like_option(const char *a) { return a[0] == '-' && a[1] != 0; }

static Parsed parse_args(int argc, char **argv, int first, const std::vector<OptSpec> &specs) {
    Parsed P;
    P.value.assign(specs.size(), nullptr);
    bool only_positional = false;
    auto set = [&](size_t k, const char *v) {
        if (P.value[k]) { P.error = "the argument '" + opt_display(specs[k]) + "' cannot be used multiple times"; return false; }
        P.value[k] = v;
        return true;
    };
    for (int i = first; i < argc && P.error.empty(); i++) {
        const char *a = argv[i];
        if (only_positional || a[0] != '-' || a[1] == 0) { P.positional.push_back(a); continue; }
        if (a[1] == '-') {
            if (a[2] == 0) { only_positional = true; continue; }
            const char *eq = strchr(a, '=');
            const std::string name = eq ? std::string(a, (size_t)(eq - a)) : std::string(a);
            if (name == "--help") { P.help = 1; return P; }
            if (name == "--version") { P.version = 1; return P; }
            size_t k = 0;
            while (k < specs.size() && name != specs[k].long_name) k++;
            if (k == specs.size()) { P.error = "unexpected argument '" + name + "' found"; break; }
            if (!specs[k].takes_value) {
                if (eq) { P.error = "unexpected value '" + std::string(eq + 1) + "' for '" + name + "' found; no more were expected"; break; }
                set(k, "");
                continue;
            }
            // clap takes the next argument as the value unless it looks like an option (a leading '-', other than a lone
            // "-"): `--debug --careful x.fa` is "a value is required", not a file named "--careful"
            const char *v = eq ? eq + 1 : (i + 1 < argc && !looks_like_option(argv[i + 1]) ? argv[++i] : nullptr);
            if (!v) { P.error = "a value is required for '" + opt_display(specs[k]) + "' but none was supplied"; break; }
            set(k, v);
            continue;
        }
        for (const char *c = a + 1; *c && P.error.empty(); c++) {  // a cluster of short options
            if (*c == 'h') { P.help = 1; return P; }
            if (*c == 'V') { P.version = 1; return P; }
            size_t k = 0;
            while (k < specs.size() && specs[k].short_name != *c) k++;
            if (k == specs.size()) { P.error = std::string("unexpected argument '-") + *c + "' found"; break; }
            if (!specs[k].takes_value) { set(k, ""); continue; }
            const char *v = c[1] ? (c[1] == '=' ? c + 2 : c + 1) : (i + 1 < argc && !looks_like_option(argv[i + 1]) ? argv[++i] : nullptr);
            if (!v) { P.error = "a value is required for '" + opt_display(specs[k]) + "' but none was supplied"; break; }
            set(k, v);
            break;  // the rest of the argument was the value
        }
    }
    return P;
}

// value of option k as f64 / u32 (clap's value_parser for the field type); false + error text on a bad value
static bool take_f64(const Parsed &P, const std::vector<OptSpec> &specs, size_t k, double &dst, std::string &err) {
    if (!P.value[k]) return true;
    if (parse_f64(P.value[k], dst)) return true;
    err = std::string("invalid value '") + P.value[k] + "' for '" + opt_display(specs[k]) + "': invalid float literal";
    return false;
}
static bool take_u32(const Parsed &P, const std::vector<OptSpec> &specs, size_t k, uint32_t &dst, std::string &err) {
    if (!P.value[k]) return true;
    if (parse_u32(P.value[k], dst)) return true;
    err = std::string("invalid value '") + P.value[k] + "' for '" + opt_display(specs[k]) + "': invalid digit found in string";
    return false;
}

// ---- the polished FASTA's form and place (not in the reference): --out, --wrap, --out_bgzf, --index ----
struct FastaForm {
    const char *out = nullptr;  // --out: the file instead of stdout
    bool wrap = false, bgzf = false, index = false;
    uint32_t width = 0;
    bool any() const { return wrap || bgzf; }
};
// the four options at specs[k0 ..]; false + error text on a --wrap that is no number (take_u32's words) or above 2^31 - 1
static bool take_fasta_form(const Parsed &P, const std::vector<OptSpec> &specs, size_t k0, FastaForm &F, std::string &err) {
    F.out = P.value[k0];
    F.wrap = P.value[k0 + 1] != nullptr;
    F.bgzf = P.value[k0 + 2] != nullptr;
    F.index = P.value[k0 + 3] != nullptr;
    if (!take_u32(P, specs, k0 + 1, F.width, err)) return false;
    if (F.width > 0x7FFFFFFFu) {
        err = std::string("invalid value '") + P.value[k0 + 1] + "' for '" + opt_display(specs[k0 + 1]) + "': number too large to fit in target type";
        return false;
    }
    return true;
}
static int refuse_bai_without_sort() {
    fprintf(stderr, "\nError: --out_bai needs --sort_out: a .bai indexes a coordinate-sorted BAM file\n");
    return 1;
}
static int refuse_index_without_out() {
    fprintf(stderr, "\nError: --index needs --out <PATH>: the indexes are written next to the file (PATH.fai, PATH.gzi)\n");
    return 1;
}
static int refuse_vcf_bgzf_without_vcf() { return usage_error("--vcf_bgzf needs --vcf <PATH>: it compresses the VCF file"); }
// --bed, --bed_bgzf, --soft_mask, --bed_status: four options from k0 on.  false with the usage error in err
struct BedForm {
    const char *path = nullptr;
    bool bgzf = false, soft_mask = false;
    uint32_t mask = PP_BED_UNDECIDED;
    bool any() const { return path || soft_mask; }
};
static bool take_bed_form(const Parsed &P, size_t k0, BedForm &B, std::string &err) {
    B.path = P.value[k0];
    B.bgzf = P.value[k0 + 1] != nullptr;
    B.soft_mask = P.value[k0 + 2] != nullptr;
    const char *list = P.value[k0 + 3];
    if (B.bgzf && !B.path) { err = "--bed_bgzf needs --bed <PATH>: it compresses the BED file"; return false; }
    if (list && !B.any()) { err = "--bed_status needs --bed <PATH> or --soft_mask: it chooses what they select"; return false; }
    if (list) {
        char msg[192] = "";
        if (pp_bed_host::parse_status_list(list, strlen(list), &B.mask, msg, sizeof msg)) {
            err = std::string("invalid value '") + list + "' for '--bed_status <LIST>': " + msg;
            return false;
        }
    }
    return true;
}
static void set_bed_form(pp_ctx *ctx, const BedForm &B) {
    pp_ctx_set_bed(ctx, B.path != nullptr, B.mask, B.bgzf);
    pp_ctx_set_soft_mask(ctx, B.soft_mask ? B.mask : 0u);
}
// --depth, --depth_bin, --depth_bgzf: three options from k0 on.  false with the usage error in err
struct DepthForm {
    const char *path = nullptr;
    bool bgzf = false;
    uint32_t bin = 0;
};
static bool take_depth_form(const Parsed &P, const std::vector<OptSpec> &specs, size_t k0, DepthForm &D, std::string &err) {
    D.path = P.value[k0];
    D.bgzf = P.value[k0 + 2] != nullptr;
    if (P.value[k0 + 1] && !D.path) { err = "--depth_bin needs --depth <PATH>: it chooses the form of the depth track"; return false; }
    if (D.bgzf && !D.path) { err = "--depth_bgzf needs --depth <PATH>: it compresses the depth track"; return false; }
    if (!take_u32(P, specs, k0 + 1, D.bin, err)) return false;
    if (D.bin > (1u << 24)) {
        err = std::string("invalid value '") + P.value[k0 + 1] + "' for '" + opt_display(specs[k0 + 1]) + "': " + P.value[k0 + 1] + " is not in 0..=16777216";
        return false;
    }
    return true;
}
// --vcf_tbi, --bed_tbi, --depth_tbi: three options from k0 on, each for a track that is written compressed.  false with the usage error in err
struct TbiForm {
    bool on[3] = {false, false, false};  // PP_TBI_VCF | _BED | _DEPTH
};
static bool take_tbi_form(const Parsed &P, size_t k0, bool vcf_bgzf, bool bed_bgzf, bool depth_bgzf, TbiForm &T, std::string &err) {
    for (int w = 0; w < 3; w++) T.on[w] = P.value[k0 + w] != nullptr;
    if (T.on[PP_TBI_VCF] && !vcf_bgzf) { err = "--vcf_tbi needs --vcf_bgzf: a .tbi indexes the bgzipped VCF file"; return false; }
    if (T.on[PP_TBI_BED] && !bed_bgzf) { err = "--bed_tbi needs --bed_bgzf: a .tbi indexes the bgzipped BED file"; return false; }
    if (T.on[PP_TBI_DEPTH] && !depth_bgzf) { err = "--depth_tbi needs --depth_bgzf: a .tbi indexes the bgzipped depth track"; return false; }
    return true;
}
static bool write_file(const std::string &path, const uint8_t *data, uint64_t len) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = (len == 0 || fwrite(data, 1, len, f) == len);
    return (fclose(f) == 0) && ok;
}
// The FASTA of a command that succeeded: to --out (created only now; a failed run leaves nothing behind) or to stdout, the indexes
// next to the file.  0, or 1 with the message on stderr.
static int deliver_fasta(pp_ctx *ctx, const FastaForm &F, const pp_bytes &fasta) {
    if (!F.out) {
        fwrite(fasta.data, 1, fasta.len, stdout);
        return 0;
    }
    bool ok = write_file(F.out, fasta.data, fasta.len);
    if (ok && F.index) {
        pp_bytes fai{nullptr, 0}, gzi{nullptr, 0};
        ok = pp_ctx_fasta_index(ctx, &fai, &gzi) == PP_OK && write_file(std::string(F.out) + ".fai", fai.data, fai.len) &&
             (!F.bgzf || write_file(std::string(F.out) + ".gzi", gzi.data, gzi.len));
        if (!ok) { remove((std::string(F.out) + ".fai").c_str()); remove((std::string(F.out) + ".gzi").c_str()); }
        pp_bytes_free(&fai);
        pp_bytes_free(&gzi);
    }
    if (ok) return 0;
    remove(F.out);
    fprintf(stderr, "\nError: unable to write the polished sequence to \"%s\"\n", F.out);
    return 1;
}
// The index of a track that was just written (--vcf_tbi, --bed_tbi, --depth_tbi; pp_ctx_tbi) to PATH.tbi.  An index that cannot be
// written leaves no track and no index behind.  0, or 1 with the message on stderr.
static int deliver_tbi(pp_ctx *ctx, int which, const char *path, const char *what) {
    const std::string to = std::string(path) + ".tbi";
    pp_bytes tbi{nullptr, 0};
    const bool ok = pp_ctx_tbi(ctx, which, &tbi) == PP_OK && write_file(to, tbi.data, tbi.len);
    pp_bytes_free(&tbi);
    if (ok) return 0;
    remove(to.c_str());
    remove(path);
    fprintf(stderr, "\nError: unable to write the index of the %s to \"%s\"\n", what, to.c_str());
    return 1;
}
// The VCF of a command that succeeded (--vcf; pp_ctx_vcf), written before the FASTA is delivered: created only now, so a refused or
// failed run leaves no file behind.  0, or 1 with the message on stderr.
static int deliver_vcf(pp_ctx *ctx, const char *path, bool tbi) {
    if (!path) return 0;
    pp_bytes vcf{nullptr, 0};
    const bool ok = pp_ctx_vcf(ctx, &vcf) == PP_OK && write_file(path, vcf.data, vcf.len);
    pp_bytes_free(&vcf);
    if (ok) return tbi ? deliver_tbi(ctx, PP_TBI_VCF, path, "VCF") : 0;
    remove(path);
    fprintf(stderr, "\nError: unable to write the VCF to \"%s\"\n", path);
    return 1;
}
// ... and the BED (--bed; pp_ctx_bed), behind the VCF
static int deliver_bed(pp_ctx *ctx, const char *path, bool tbi) {
    if (!path) return 0;
    pp_bytes bed{nullptr, 0};
    const bool ok = pp_ctx_bed(ctx, &bed) == PP_OK && write_file(path, bed.data, bed.len);
    pp_bytes_free(&bed);
    if (ok) return tbi ? deliver_tbi(ctx, PP_TBI_BED, path, "BED") : 0;
    remove(path);
    fprintf(stderr, "\nError: unable to write the BED to \"%s\"\n", path);
    return 1;
}
// ... and the depth track (--depth; pp_ctx_depth), behind the BED
static int deliver_depth(pp_ctx *ctx, const char *path, bool tbi) {
    if (!path) return 0;
    pp_bytes track{nullptr, 0};
    const bool ok = pp_ctx_depth(ctx, &track) == PP_OK && write_file(path, track.data, track.len);
    pp_bytes_free(&track);
    if (ok) return tbi ? deliver_tbi(ctx, PP_TBI_DEPTH, path, "depth track") : 0;
    remove(path);
    fprintf(stderr, "\nError: unable to write the depth track to \"%s\"\n", path);
    return 1;
}
// the form on a context: --index alone still needs the text's table, so it takes the device link at width 0
static void set_fasta_form(pp_ctx *ctx, const FastaForm &F) {
    if (F.any() || F.index) pp_ctx_set_fasta_form(ctx, (int64_t)F.width, F.bgzf);
    pp_ctx_set_fasta_out_name_(ctx, F.out);
}

static int no_device(int device) {
    fprintf(stderr, "\nError: no usable MI355X (HIP) device %d -- this build has no CPU path\n", device);
    return 1;
}

// A finished run has nothing left to save: flush the streams and leave without tearing down the HIP
// runtime and unmapping gigabytes of parsed input page by page (the kernel reclaims both at exit).
static int finish(int code) {
    fflush(stdout);
    if (getenv("PP_TIMING")) fprintf(stderr, "[timing] %-36s %8s    (process %7.3f s)\n", "output written, leaving", "", pph::seconds_since_process_start());
    fflush(stderr);
    _exit(code);
}

// The devices `polish` runs on.  The count comes from the environment or sysfs first: asking HIP initialises the
// runtime (a few 100 ms that the single-GPU path hides behind the host parse), so it is only asked when there may
// be more than one GPU.
static std::vector<int> polish_devices(int device, bool single_only) {
    std::vector<int> one{device};
    if (single_only || getenv("PP_DEVICE")) return one;
    if (const char *sh = getenv("PP_SHARE_GPU")) {
        const int n = atoi(sh);
        return n > 1 ? std::vector<int>((size_t)n, device) : one;
    }
    int guess = 0;
    const char *vis = getenv("HIP_VISIBLE_DEVICES") ? getenv("HIP_VISIBLE_DEVICES") : getenv("ROCR_VISIBLE_DEVICES");
    if (vis && *vis) {
        guess = 1;
        for (const char *p = vis; *p; p++) guess += *p == ',';
    } else {
        for (int node = 0; node < 64; node++) {  // kfd topology: GPU nodes have SIMDs
            char path[128];
            snprintf(path, sizeof path, "/sys/class/kfd/kfd/topology/nodes/%d/properties", node);
            FILE *f = fopen(path, "r");
            if (!f) break;
            char key[64];
            unsigned long long val;
            while (fscanf(f, "%63s %llu", key, &val) == 2)
                if (!strcmp(key, "simd_count") && val > 0) { guess++; break; }
            fclose(f);
        }
    }
    int want = guess;
    if (const char *g = getenv("PP_GPUS")) want = std::min(want, std::max(1, atoi(g)));
    if (want <= 1) return one;
    const int have = pp_device_count();
    want = std::min(want, have);
    if (want <= 1) return one;
    std::vector<int> v;
    for (int d = 0; d < want; d++) v.push_back(d);
    return v;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fputs(HELP, stderr);
        return 2;
    }
    std::string cmd = argv[1];
    if (cmd == "-h" || cmd == "--help") { fputs(HELP, stdout); return 0; }
    if (cmd == "-V" || cmd == "--version") { printf("Polypolish v0.6.1 (%s)\n", pp_version()); return 0; }
    int device = getenv("PP_DEVICE") ? atoi(getenv("PP_DEVICE")) : 0;
    pp_process_leaving_soon_(1);  // every command ends in finish(): _exit without tearing the mappings and the runtime down

    if (cmd == "polish") {
        pp_polish_options opt{0.2, 0.5, 10, 5, 0, nullptr, 0};
        bool regroup = false;  // (not in the reference) BAM files whose reads do not stand together: pp_ctx_set_regroup
        bool text_chain = false;  // (not in the reference) SAM text through the record chain: pp_ctx_set_text_chain
        const std::vector<OptSpec> specs = {{"--debug", 0, true, "<DEBUG>"},
                                            {"--fraction_invalid", 'i', true, "<FRACTION_INVALID>"},
                                            {"--fraction_valid", 'v', true, "<FRACTION_VALID>"},
                                            {"--max_errors", 'm', true, "<MAX_ERRORS>"},
                                            {"--min_depth", 'd', true, "<MIN_DEPTH>"},
                                            {"--careful", 0, false, ""},
                                            {"--regroup", 0, false, ""},
                                            {"--text_chain", 0, false, ""},
                                            {"--out", 0, true, "<PATH>"},
                                            {"--wrap", 0, true, "<N>"},
                                            {"--out_bgzf", 0, false, ""},
                                            {"--index", 0, false, ""},
                                            {"--vcf", 0, true, "<PATH>"},
                                            {"--vcf_bgzf", 0, false, ""},
                                            {"--bed", 0, true, "<PATH>"},
                                            {"--bed_bgzf", 0, false, ""},
                                            {"--soft_mask", 0, false, ""},
                                            {"--bed_status", 0, true, "<LIST>"},
                                            {"--depth", 0, true, "<PATH>"},
                                            {"--depth_bin", 0, true, "<N>"},
                                            {"--depth_bgzf", 0, false, ""},
                                            {"--vcf_tbi", 0, false, ""},
                                            {"--bed_tbi", 0, false, ""},
                                            {"--depth_tbi", 0, false, ""}};
        FastaForm form;
        const Parsed P = parse_args(argc, argv, 2, specs);
        if (P.help) { fputs(HELP_POLISH, stdout); return 0; }
        if (P.version) { printf("polypolish-polish v0.6.1\n"); return 0; }
        std::string perr = P.error;
        if (perr.empty()) {
            opt.debug_path = P.value[0];
            opt.careful = P.value[5] != nullptr;
            regroup = P.value[6] != nullptr;
            text_chain = P.value[7] != nullptr;
            (void)(take_f64(P, specs, 1, opt.fraction_invalid, perr) && take_f64(P, specs, 2, opt.fraction_valid, perr) &&
                   take_u32(P, specs, 3, opt.max_errors, perr) && take_u32(P, specs, 4, opt.min_depth, perr) &&
                   take_fasta_form(P, specs, 8, form, perr));
        }
        if (!perr.empty()) return usage_error(perr.c_str());
        const char *vcf = P.value[12];
        const bool vcf_bgzf = P.value[13] != nullptr;
        if (vcf_bgzf && !vcf) return refuse_vcf_bgzf_without_vcf();
        BedForm bed;
        if (!take_bed_form(P, 14, bed, perr)) return usage_error(perr.c_str());
        DepthForm depth;
        if (!take_depth_form(P, specs, 18, depth, perr)) return usage_error(perr.c_str());
        TbiForm tbi;
        if (!take_tbi_form(P, 21, vcf_bgzf, bed.bgzf, depth.bgzf, tbi, perr)) return usage_error(perr.c_str());
        if (form.index && !form.out) return refuse_index_without_out();
        const char *assembly = P.positional.empty() ? nullptr : P.positional[0];
        std::vector<const char *> sams(P.positional.begin() + (P.positional.empty() ? 0 : 1), P.positional.end());
        if (!assembly) return usage_error("the following required arguments were not provided:\n  <ASSEMBLY>");
        // Several GPUs polish (contigs / windows of a large contig shard across them) when PP_GPUS=n asks for them, --debug
        // included (every context formats the lines of the positions it emits).  On small jobs one GPU is the faster choice end to end: the polish itself is a millisecond per 5 Mbp,
        // what a second context adds is its start-up.  (Until round 4 the CLI switched by itself from 8 GiB of SAM text on;
        // the path has only ever run with several contexts on ONE device -- PP_SHARE_GPU=n, tests on a one-GPU box -- so it
        // stays opt-in until it has been run on a multi-GPU node.)
        const bool few = !getenv("PP_GPUS") && !getenv("PP_SHARE_GPU");
        // BAM input runs on one GPU: asking for several is refused whatever the box has
        const bool several = (getenv("PP_GPUS") && atoi(getenv("PP_GPUS")) > 1) || (getenv("PP_SHARE_GPU") && atoi(getenv("PP_SHARE_GPU")) > 1);
        if (several && vcf) {  // (refused before any file is opened, as BAM input below)
            fprintf(stderr, "\nError: --vcf runs on one GPU: polish without PP_GPUS / PP_SHARE_GPU, or without --vcf\n");
            return 1;
        }
        if (several && bed.any()) {
            fprintf(stderr, "\nError: %s runs on one GPU: polish without PP_GPUS / PP_SHARE_GPU, or without %s\n", bed.path ? "--bed" : "--soft_mask", bed.path ? "--bed" : "--soft_mask");
            return 1;
        }
        if (several && depth.path) {
            fprintf(stderr, "\nError: --depth runs on one GPU: polish without PP_GPUS / PP_SHARE_GPU, or without --depth\n");
            return 1;
        }
        for (size_t i = 0; several && i < sams.size(); i++) {
            int kind = PP_ALN_SAM;
            if ((text_chain ? pp_aln_file_kind_text(sams[i], &kind) : pp_aln_file_kind(sams[i], &kind)) != PP_OK) continue;
            if (kind == PP_ALN_BAM || kind == PP_ALN_BAM_RAW) {
                fprintf(stderr, "\nError: BAM input (\"%s\") runs on one GPU: polish it without PP_GPUS / PP_SHARE_GPU, or convert it to SAM text\n", sams[i]);
                return 1;
            }
            if (text_chain) {
                fprintf(stderr, "\nError: SAM text on the record chain (--text_chain, \"%s\") runs on one GPU: polish it without PP_GPUS / PP_SHARE_GPU, or without --text_chain\n", sams[i]);
                return 1;
            }
        }
        std::vector<int> devs = polish_devices(device, few);
        if (devs.size() > 1) {
            std::vector<pp_ctx *> cs(devs.size(), nullptr);
            for (size_t d = 0; d < devs.size(); d++)
                if (pp_ctx_create_async(devs[d], &cs[d]) || pp_ctx_set_regroup(cs[d], regroup) || pp_ctx_set_text_chain(cs[d], text_chain)) return no_device(devs[d]);
            set_fasta_form(cs[0], form);
            pp_ctx_set_vcf(cs[0], vcf != nullptr, vcf_bgzf);  // (several contexts: the driver refuses it by name)
            set_bed_form(cs[0], bed);
            pp_ctx_set_depth(cs[0], depth.path != nullptr, depth.bin, depth.bgzf);
            pp_ctx_set_tbi(cs[0], tbi.on[PP_TBI_VCF], tbi.on[PP_TBI_BED], tbi.on[PP_TBI_DEPTH]);
            pp_bytes fasta{nullptr, 0};
            int rc = pp_polish_files_multi(cs.data(), (int)cs.size(), assembly, sams.data(), (int)sams.size(), &opt, &fasta);
            for (size_t d = 0; d < devs.size(); d++)
                if (pp_ctx_wait(cs[d]) != PP_OK) return no_device(devs[d]);
            if (rc) {
                fprintf(stderr, "\nError: %s\n", pp_last_error(cs[0]));
                for (pp_ctx *c : cs) pp_ctx_destroy(c);
                return rc == PP_ERR_PANIC ? 101 : 1;
            }
            if (deliver_vcf(cs[0], vcf, tbi.on[PP_TBI_VCF]) || deliver_bed(cs[0], bed.path, tbi.on[PP_TBI_BED]) || deliver_depth(cs[0], depth.path, tbi.on[PP_TBI_DEPTH]) || deliver_fasta(cs[0], form, fasta)) return 1;
            return finish(0);
        }
        // the device initialises on a helper thread while the host loads and parses the inputs
        pp_ctx *ctx = nullptr;
        int rc = pp_ctx_create_async(device, &ctx);
        if (rc) return no_device(device);
        pp_ctx_set_regroup(ctx, regroup);
        pp_ctx_set_text_chain(ctx, text_chain);
        set_fasta_form(ctx, form);
        pp_ctx_set_vcf(ctx, vcf != nullptr, vcf_bgzf);
        set_bed_form(ctx, bed);
        pp_ctx_set_depth(ctx, depth.path != nullptr, depth.bin, depth.bgzf);
        pp_ctx_set_tbi(ctx, tbi.on[PP_TBI_VCF], tbi.on[PP_TBI_BED], tbi.on[PP_TBI_DEPTH]);
        pp_bytes fasta{nullptr, 0};
        rc = pp_polish_files(ctx, assembly, sams.data(), (int)sams.size(), &opt, &fasta);
        if (pp_ctx_wait(ctx) != PP_OK) return no_device(device);
        if (rc) {
            fprintf(stderr, "\nError: %s\n", pp_last_error(ctx));
            pp_ctx_destroy(ctx);
            return rc == PP_ERR_PANIC ? 101 : 1;
        }
        if (deliver_vcf(ctx, vcf, tbi.on[PP_TBI_VCF]) || deliver_bed(ctx, bed.path, tbi.on[PP_TBI_BED]) || deliver_depth(ctx, depth.path, tbi.on[PP_TBI_DEPTH]) || deliver_fasta(ctx, form, fasta)) return 1;
        return finish(0);
    }

    if (cmd == "filter-polish") {
        pp_polish_options opt{0.2, 0.5, 10, 5, 0, nullptr, 0};
        const char *orientation = "auto";
        double low = 0.1, high = 99.9;
        bool regroup = false;
        const std::vector<OptSpec> specs = {{"--in1", 0, true, "<IN1>"}, {"--in2", 0, true, "<IN2>"},
                                            {"--out1", 0, true, "<OUT1>"}, {"--out2", 0, true, "<OUT2>"},
                                            {"--orientation", 0, true, "<ORIENTATION>"}, {"--low", 0, true, "<LOW>"},
                                            {"--high", 0, true, "<HIGH>"}, {"--debug", 0, true, "<DEBUG>"},
                                            {"--fraction_invalid", 'i', true, "<FRACTION_INVALID>"},
                                            {"--fraction_valid", 'v', true, "<FRACTION_VALID>"},
                                            {"--max_errors", 'm', true, "<MAX_ERRORS>"},
                                            {"--min_depth", 'd', true, "<MIN_DEPTH>"},
                                            {"--careful", 0, false, ""},
                                            {"--regroup", 0, false, ""},
                                            {"--out_bam", 0, false, ""},
                                            {"--out_sam", 0, false, ""},
                                            {"--text_chain", 0, false, ""},
                                            {"--out", 0, true, "<PATH>"},
                                            {"--wrap", 0, true, "<N>"},
                                            {"--out_bgzf", 0, false, ""},
                                            {"--index", 0, false, ""},
                                            {"--sort_out", 0, false, ""},
                                            {"--out_bai", 0, false, ""},
                                            {"--vcf", 0, true, "<PATH>"},
                                            {"--vcf_bgzf", 0, false, ""},
                                            {"--bed", 0, true, "<PATH>"},
                                            {"--bed_bgzf", 0, false, ""},
                                            {"--soft_mask", 0, false, ""},
                                            {"--bed_status", 0, true, "<LIST>"},
                                            {"--depth", 0, true, "<PATH>"},
                                            {"--depth_bin", 0, true, "<N>"},
                                            {"--depth_bgzf", 0, false, ""},
                                            {"--vcf_tbi", 0, false, ""},
                                            {"--bed_tbi", 0, false, ""},
                                            {"--depth_tbi", 0, false, ""}};
        FastaForm form;
        const Parsed P = parse_args(argc, argv, 2, specs);
        if (P.help || P.version) { fputs(HELP_FUSED, stdout); return 0; }
        std::string perr = P.error;
        if (perr.empty()) {
            if (P.value[4]) orientation = P.value[4];
            opt.debug_path = P.value[7];
            opt.careful = P.value[12] != nullptr;
            regroup = P.value[13] != nullptr;
            (void)(take_f64(P, specs, 5, low, perr) && take_f64(P, specs, 6, high, perr) &&
                   take_f64(P, specs, 8, opt.fraction_invalid, perr) && take_f64(P, specs, 9, opt.fraction_valid, perr) &&
                   take_u32(P, specs, 10, opt.max_errors, perr) && take_u32(P, specs, 11, opt.min_depth, perr) &&
                   take_fasta_form(P, specs, 17, form, perr));
            if (perr.empty() && P.positional.size() > 1) perr = std::string("unexpected argument '") + P.positional[1] + "' found";
        }
        if (!perr.empty()) return usage_error(perr.c_str());
        const char *in1 = P.value[0], *in2 = P.value[1], *out1 = P.value[2], *out2 = P.value[3];
        const char *assembly = P.positional.empty() ? nullptr : P.positional[0];
        if (!assembly || !in1 || !in2)
            return usage_error("the following required arguments were not provided:\n  --in1 <IN1> --in2 <IN2> <ASSEMBLY>");
        if (form.index && !form.out) return refuse_index_without_out();
        if (P.value[22] && !P.value[21]) return refuse_bai_without_sort();
        const char *vcf = P.value[23];
        const bool vcf_bgzf = P.value[24] != nullptr;
        if (vcf_bgzf && !vcf) return refuse_vcf_bgzf_without_vcf();
        BedForm bed;
        DepthForm depth;
        {
            std::string berr;
            if (!take_bed_form(P, 25, bed, berr) || !take_depth_form(P, specs, 29, depth, berr)) return usage_error(berr.c_str());
        }
        TbiForm tbi;
        {
            std::string terr;
            if (!take_tbi_form(P, 32, vcf_bgzf, bed.bgzf, depth.bgzf, tbi, terr)) return usage_error(terr.c_str());
        }
        pp_ctx *ctx = nullptr;
        int rc = pp_ctx_create_async(device, &ctx);
        if (rc) return no_device(device);
        pp_ctx_set_sort_out(ctx, P.value[21] != nullptr, P.value[22] != nullptr);
        pp_ctx_set_regroup(ctx, regroup);
        pp_ctx_set_out_bam(ctx, P.value[14] != nullptr);
        pp_ctx_set_out_sam(ctx, P.value[15] != nullptr);
        pp_ctx_set_text_chain(ctx, P.value[16] != nullptr);
        set_fasta_form(ctx, form);
        pp_ctx_set_vcf(ctx, vcf != nullptr, vcf_bgzf);
        set_bed_form(ctx, bed);
        pp_ctx_set_depth(ctx, depth.path != nullptr, depth.bin, depth.bgzf);
        pp_ctx_set_tbi(ctx, tbi.on[PP_TBI_VCF], tbi.on[PP_TBI_BED], tbi.on[PP_TBI_DEPTH]);
        pp_bytes fasta{nullptr, 0};
        rc = pp_filter_polish_files(ctx, assembly, in1, in2, out1, out2, orientation, low, high, &opt, nullptr, &fasta);
        if (pp_ctx_wait(ctx) != PP_OK) return no_device(device);
        if (rc) {
            fprintf(stderr, "\nError: %s\n", pp_last_error(ctx));
            pp_ctx_destroy(ctx);
            return rc == PP_ERR_PANIC ? 101 : 1;
        }
        if (deliver_vcf(ctx, vcf, tbi.on[PP_TBI_VCF]) || deliver_bed(ctx, bed.path, tbi.on[PP_TBI_BED]) || deliver_depth(ctx, depth.path, tbi.on[PP_TBI_DEPTH]) || deliver_fasta(ctx, form, fasta)) return 1;
        return finish(0);
    }

    if (cmd == "filter") {
        const char *orientation = "auto";
        double low = 0.1, high = 99.9;
        const std::vector<OptSpec> specs = {{"--in1", 0, true, "<IN1>"}, {"--in2", 0, true, "<IN2>"},
                                            {"--out1", 0, true, "<OUT1>"}, {"--out2", 0, true, "<OUT2>"},
                                            {"--orientation", 0, true, "<ORIENTATION>"}, {"--low", 0, true, "<LOW>"},
                                            {"--high", 0, true, "<HIGH>"}, {"--out_bam", 0, false, ""},
                                            {"--out_sam", 0, false, ""}, {"--text_chain", 0, false, ""},
                                            {"--sort_out", 0, false, ""}, {"--out_bai", 0, false, ""}};
        const Parsed P = parse_args(argc, argv, 2, specs);
        if (P.help) { fputs(HELP_FILTER, stdout); return 0; }
        if (P.version) { printf("polypolish-filter v0.6.1\n"); return 0; }
        std::string perr = P.error;
        if (perr.empty()) {
            if (P.value[4]) orientation = P.value[4];
            (void)(take_f64(P, specs, 5, low, perr) && take_f64(P, specs, 6, high, perr));
            if (perr.empty() && !P.positional.empty()) perr = std::string("unexpected argument '") + P.positional[0] + "' found";
        }
        if (!perr.empty()) return usage_error(perr.c_str());
        const char *in1 = P.value[0], *in2 = P.value[1], *out1 = P.value[2], *out2 = P.value[3];
        if (!in1 || !in2 || !out1 || !out2)
            return usage_error("the following required arguments were not provided:\n  --in1 <IN1> --in2 <IN2> --out1 <OUT1> --out2 <OUT2>");
        if (P.value[11] && !P.value[10]) return refuse_bai_without_sort();
        pp_ctx *ctx = nullptr;
        int rc = pp_ctx_create_async(device, &ctx);
        if (rc) return no_device(device);
        pp_ctx_set_sort_out(ctx, P.value[10] != nullptr, P.value[11] != nullptr);
        pp_ctx_set_out_bam(ctx, P.value[7] != nullptr);
        pp_ctx_set_out_sam(ctx, P.value[8] != nullptr);
        pp_ctx_set_text_chain(ctx, P.value[9] != nullptr);
        rc = pp_filter_files(ctx, in1, in2, out1, out2, orientation, low, high, 0, nullptr);
        if (pp_ctx_wait(ctx) != PP_OK) return no_device(device);
        if (rc) {
            fprintf(stderr, "\nError: %s\n", pp_last_error(ctx));
            pp_ctx_destroy(ctx);
            return rc == PP_ERR_PANIC ? 101 : 1;
        }
        return finish(0);
    }
    return usage_error((std::string("unrecognized subcommand '") + cmd + "'").c_str());
}
