// pp_host.h -- host-side utilities shared by the SAM ingest (pp_ingest.cpp) and the command drivers (pp_driver*.cpp,
// pp_filter_host.cpp): huge-page growable arrays, a fork-join parallel_for, a read-only file mapping, the run log's
// helpers, and the declarations of the library's internal entry points.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <ctime>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "polypolish_hip.h"

// ---- internal entry points the host files share (the trailing underscore keeps them out of polypolish_hip.h) ----
extern "C" {
int pp_ctx_set_error_(pp_ctx *ctx, int code, const char *msg);  // pp_ctx is opaque to the host files: its error text is stored through this hook
int pp_ctx_device_(const pp_ctx *ctx);                          // the device a context runs on
int pp_ctx_sort_out_(const pp_ctx *ctx, int *index);            // what pp_ctx_set_sort_out was given (the filter drivers)
int pp_ctx_out_bam_(const pp_ctx *ctx);                         // what pp_ctx_set_out_bam was given (the filter drivers)
int pp_ctx_out_sam_(const pp_ctx *ctx);                         // what pp_ctx_set_out_sam was given (the filter drivers)
int pp_ctx_regroup_(const pp_ctx *ctx);                         // what pp_ctx_set_regroup was given (the file drivers)
int pp_ctx_text_chain_(const pp_ctx *ctx);                      // what pp_ctx_set_text_chain was given (the file drivers)
int pp_ctx_fasta_form_(const pp_ctx *ctx, int64_t *width, int *bgzf);  // what pp_ctx_set_fasta_form was given; 1 when the form is on (the file drivers)
void pp_ctx_keep_fasta_index_(pp_ctx *ctx, const uint8_t *fai, uint64_t n_fai, const uint8_t *gzi, uint64_t n_gzi);  // ... and the indexes of the text they made
int pp_ctx_vcf_form_(const pp_ctx *ctx, int *bgzf);             // what pp_ctx_set_vcf was given; 1 when the VCF is on (the file drivers)
void pp_ctx_keep_vcf_(pp_ctx *ctx, const uint8_t *data, uint64_t n);  // ... and the file they made (NULL: none -- a run begins)
int pp_ctx_bed_form_(const pp_ctx *ctx, uint32_t *status_mask, int *bgzf);  // what pp_ctx_set_bed was given; 1 when the BED is on (the file drivers)
void pp_ctx_keep_bed_(pp_ctx *ctx, const uint8_t *data, uint64_t n);  // ... and the file they made (NULL: none -- a run begins)
uint32_t pp_ctx_soft_mask_(const pp_ctx *ctx);                  // what pp_ctx_set_soft_mask was given (0: off)
int pp_ctx_depth_form_(const pp_ctx *ctx, uint32_t *bin, int *bgzf);  // what pp_ctx_set_depth was given; 1 when the depth track is on (the file drivers)
void pp_ctx_keep_depth_(pp_ctx *ctx, const uint8_t *data, uint64_t n);  // ... and the file they made (NULL: none -- a run begins)
int pp_ctx_tbi_form_(const pp_ctx *ctx, int which);  // what pp_ctx_set_tbi was given for PP_TBI_VCF | _BED | _DEPTH; 1 when that index is on
void pp_ctx_keep_tbi_(pp_ctx *ctx, int which, const uint8_t *data, uint64_t n);  // ... and the index they made (NULL: none -- a run begins)
int pp_ctx_set_fasta_out_name_(pp_ctx *ctx, const char *path);  // the file the caller will write the FASTA to (NULL: stdout); the log names it
const char *pp_ctx_fasta_out_name_(const pp_ctx *ctx);
int pp_sam_empty_qname_rule_(pp_sam *s);                        // pp_sam.hip: read_id as the reference groups behind an empty QNAME (the text front, for the gate)
void pp_ctx_enable_peers_(pp_ctx *const *ctxs, int n);          // peer access between the contexts' devices, best effort (PP_MEM_PEER copies)
void *pp_host_pinned_alloc_(pp_ctx *ctx, uint64_t bytes);       // pinned host memory for the --debug TSV's chunks ...
void pp_host_pinned_free_(void *p);                             // ... and its release
void pp_process_leaving_soon_(int yes);                         // (bin/polypolish only) the process exits right after the command: pph::process_leaving_soon
int pp_dev_ingest_reserve_text_(pp_dev_ingest *D, uint64_t bytes);  // room for the text of the job's largest file, once
// the text of the file the next pp_dev_ingest_sam will take goes up while the one before is tokenized
void pp_dev_ingest_prefetch_(pp_dev_ingest *D, const char *path, uint64_t second_buffer_bytes);
// one context's slice of a SAM file (the multi-GPU driver cuts at read-group boundaries); any defect in the text only says so
int pp_dev_ingest_slice_(pp_dev_ingest *D, const char *path, const char *text, uint64_t size, pp_sam_counts *counts);
// did the last pp_ingest_sam fail where the records before are known?  *cut = bytes of the file holding exactly those groups
int pp_ingest_fail_cut_(const pp_ingest *I, uint64_t *cut);
// ingest only the first `cut` bytes of the file
int pp_ingest_sam_prefix_(pp_ingest *I, const char *path, uint64_t cut, const uint8_t *pass, uint64_t n_pass, pp_sam_counts *counts, char *err, size_t errlen);
// pp_polish_files with per-file filter verdicts (pp_filter_polish_files)
int pp_polish_files_filtered_(pp_ctx *ctx, const char *assembly, const char *const *sams, int n_sams, const pp_polish_options *opt, pp_bytes *fasta,
                              const uint8_t *const *pass, const uint64_t *n_pass);
// pp_shard_split of a view on records [lo, hi) of a larger batch: wo_idx_base = what the file_idx of batch->wo count from
int pp_shard_split_view_(pp_ctx *ctx, const pp_shard_plan *plan, uint32_t dest, const pp_aln_batch *batch, int mem, uint32_t wo_idx_base, pp_shard_part **out);
// pp_polish_gather with the payload copied to rank 0's host_out in one transfer
int pp_polish_gather_to_host_(pp_ctx *ctx, uint8_t *host_out, uint64_t cap, uint64_t *rank_len, uint64_t *rank_contig_off);
}

#ifndef PP_MIRROR_REGISTRY_DECLARED
#define PP_MIRROR_REGISTRY_DECLARED
// The window-order mirrors the library's own producers hand out (pp_ingest_batch, pp_dev_ingest_batch, pp_shard_split's parts),
// as address ranges keyed by their owner: a mirror inside one of them (a part of one: the multi-GPU driver's slice views) is
// taken as it is, any other mirror is compared with the arrays it mirrors before the kernels read the records through it
// (pp_polish_add, run_pipeline).  Implemented in pp_shard.cpp.
void pp_mirror_register_(const void *owner, const void *p, size_t bytes);
void pp_mirror_forget_(const void *owner);
bool pp_mirror_trusted_(const void *p, size_t bytes);
#endif

namespace pph {

// Growable array for the multi-GB buffers of a large job: anonymous mmap backed by transparent huge
// pages where the kernel allows (512x fewer page faults while many threads first-touch it, and a much
// cheaper teardown), grown with mremap, and never zero-filled by us.
template <typename T>
struct HugeBuf {
    static constexpr size_t HUGE = size_t(2) << 20;
    T *p = nullptr;
    size_t n = 0, cap = 0, mapped = 0;  // elements, elements, bytes
    HugeBuf() = default;
    HugeBuf(const HugeBuf &) = delete;
    HugeBuf &operator=(const HugeBuf &) = delete;
    HugeBuf(HugeBuf &&o) noexcept : p(o.p), n(o.n), cap(o.cap), mapped(o.mapped) { o.p = nullptr; o.n = o.cap = o.mapped = 0; }
    ~HugeBuf() { if (p) munmap(p, mapped); }
    T *data() { return p; }
    const T *data() const { return p; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
    T &back() { return p[n - 1]; }
    void reserve(size_t m) {
        if (m <= cap) return;
        size_t bytes = std::max(m, cap * 2) * sizeof(T);
        bytes = (bytes + HUGE - 1) / HUGE * HUGE;
        void *q = p ? mremap(p, mapped, bytes, MREMAP_MAYMOVE)
                    : mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (q == MAP_FAILED) throw std::bad_alloc();
        madvise(q, bytes, MADV_HUGEPAGE);
        p = (T *)q;
        mapped = bytes;
        cap = bytes / sizeof(T);
    }
    void resize(size_t m) { reserve(m); n = m; }
    void push_back(const T &v) {
        if (n == cap) reserve(n + 1);
        p[n++] = v;
    }
};

// f(lo, hi, t): contiguous ranges of [0, n) in order, one per thread index t
template <typename F>
void parallel_for(size_t n, unsigned threads, F f) {
    if (threads <= 1 || n < 2) { f((size_t)0, n, 0u); return; }
    std::vector<std::thread> pool;
    const size_t per = (n + threads - 1) / threads;
    for (unsigned t = 0; t < threads; t++) {
        const size_t lo = std::min(n, (size_t)t * per), hi = std::min(n, lo + per);
        if (lo < hi) pool.emplace_back([=] { f(lo, hi, t); });
    }
    for (auto &th : pool) th.join();
}

// The command-line program leaves with _exit as soon as its output is written: unmapping tens of GB of input mappings
// (0.14 s per 15 GB, and every mmap / hipMalloc of the process waits for the lock meanwhile) and releasing device buffers is
// then the kernel's business at exit.  Library callers never set this: their mappings are unmapped on a background thread.
inline bool &process_leaving_soon() { static bool v = false; return v; }

// seconds since this process was started (its start time in /proc/self/stat against CLOCK_BOOTTIME; 10 ms resolution):
// what a PP_TIMING line of a command driver counts from -- exec, dynamic linking and the HIP runtime's start-up included
inline double seconds_since_process_start() {
    static const double started = [] {
        double st = -1.0;
        if (FILE *f = fopen("/proc/self/stat", "r")) {
            char buf[1024];
            const size_t n = fread(buf, 1, sizeof buf - 1, f);
            fclose(f);
            buf[n] = 0;
            if (const char *p = strrchr(buf, ')')) {  // fields after the command name: state is the 3rd, starttime the 22nd
                int field = 2;
                for (p++; *p && field < 22; p++)  // (every space opens the next field: p ends up on the first digit of the 22nd)
                    if (*p == ' ') field++;
                if (field == 22) st = strtod(p, nullptr) / (double)sysconf(_SC_CLK_TCK);
            }
        }
        return st;
    }();
    struct timespec ts;
    if (started < 0 || clock_gettime(CLOCK_BOOTTIME, &ts) != 0) return -1.0;
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec - started;
}

// PP_INGEST_THREADS, else one thread per 4 MiB of text up to min(cores, 64)
inline unsigned host_threads(size_t text_bytes) {
    if (const char *e = getenv("PP_INGEST_THREADS")) return (unsigned)std::max(1, std::min(64, atoi(e)));
    return std::max(1u, std::min({std::thread::hardware_concurrency(), 64u, (unsigned)(text_bytes / (4u << 20)) + 1u}));
}

// Pre-faulting a file mapping (page-cache pages into this process's page tables) with a few threads.  A host-to-device
// copy out of a mapping nobody has touched faults it in page by page, 4 KiB at a time: 13 GB/s instead of the 56 GB/s
// the link delivers (measured on a 1.2 GB SAM file, tools/microbench/h2d2.hip: 89 ms against 3 + 21 ms).
#ifndef MADV_POPULATE_READ
#define MADV_POPULATE_READ 22

#endif
inline void populate_mapping(void *map, size_t size, unsigned threads = 8) {
    if (!map || !size) return;
    threads = std::max(1u, std::min(threads, (unsigned)(size >> 24) + 1u));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < threads; t++)
        th.emplace_back([=] {
            const size_t page = 4096;
            size_t a = (size / threads * t) & ~(page - 1), b = t + 1 == threads ? size : (size / threads * (t + 1)) & ~(page - 1);
            if (b <= a) return;
            if (madvise((char *)map + a, b - a, MADV_POPULATE_READ) == 0) return;
            volatile char sink = 0;  // kernels before 5.14: touch every page
            for (size_t q = a; q < b; q += page) sink += ((const volatile char *)map)[q];
            (void)sink;
        });
    for (auto &x : th) x.join();
}

// Files opened ahead of their use (the driver does this while the HIP runtime initialises): mapped, and pre-faulted by a
// background thread.  FileText::open_file adopts the mapping of a path that was prefetched.
struct PrefetchedFile {
    std::string path;
    void *map = nullptr;
    size_t size = 0;
    int fd = -1;
    const void *owner = nullptr;  // who asked for it (a job's context): prefetch_drop_all releases only its own
    std::thread worker;
};
inline std::mutex &prefetch_mutex() { static std::mutex m; return m; }
inline std::vector<PrefetchedFile *> &prefetch_list() { static std::vector<PrefetchedFile *> v; return v; }
inline void prefetch_file(const char *path, const void *owner) {
    struct stat st;
    if (::stat(path, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size <= 0) return;  // never open a pipe just to look at it
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size <= 0) { ::close(fd); return; }
    void *map = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (map == MAP_FAILED) { ::close(fd); return; }
    PrefetchedFile *f = new PrefetchedFile;
    f->path = path; f->map = map; f->size = (size_t)st.st_size; f->fd = fd; f->owner = owner;
    f->worker = std::thread([f] { populate_mapping(f->map, f->size); });
    std::lock_guard<std::mutex> lock(prefetch_mutex());
    prefetch_list().push_back(f);
}
inline PrefetchedFile *prefetch_take(const char *path) {  // nullptr if the path was not prefetched
    PrefetchedFile *f = nullptr;
    {
        std::lock_guard<std::mutex> lock(prefetch_mutex());
        auto &v = prefetch_list();
        for (size_t i = 0; i < v.size(); i++)
            if (v[i]->path == path) { f = v[i]; v.erase(v.begin() + (long)i); break; }
    }
    if (f && f->worker.joinable()) f->worker.join();
    return f;
}
inline void prefetch_drop_all(const void *owner) {  // whatever `owner` had prefetched and never opened
    for (;;) {
        PrefetchedFile *f = nullptr;
        {
            std::lock_guard<std::mutex> lock(prefetch_mutex());
            auto &v = prefetch_list();
            for (size_t i = v.size(); i-- > 0;)
                if (v[i]->owner == owner) { f = v[i]; v.erase(v.begin() + (long)i); break; }
            if (!f) return;
        }
        if (f->worker.joinable()) f->worker.join();
        munmap(f->map, f->size);
        ::close(f->fd);
        delete f;
    }
}

// char::is_whitespace (Unicode White_Space: what `splitn(2, char::is_whitespace)` splits a FASTA header at, misc.rs:118-120)
// at the start of the valid UTF-8 text p[0 .. left): the bytes of that character, 0 if it is not whitespace.
// U+0009-000D, 0020, 0085, 00A0, 1680, 2000-200A, 2028, 2029, 202F, 205F, 3000.  (pp_ingest.cpp's load_fasta and pp_fasta_host.h)
inline size_t rust_ws_len(const char *p, size_t left) {
    const unsigned char c = (unsigned char)p[0];
    if (c == ' ' || (c >= 0x09 && c <= 0x0D)) return 1;
    if (c == 0xC2 && left >= 2) {
        const unsigned char d = (unsigned char)p[1];
        return d == 0x85 || d == 0xA0 ? 2 : 0;
    }
    if (left >= 3) {
        const unsigned char d = (unsigned char)p[1], e = (unsigned char)p[2];
        if (c == 0xE1 && d == 0x9A && e == 0x80) return 3;
        if (c == 0xE2 && d == 0x80 && ((e >= 0x80 && e <= 0x8A) || e == 0xA8 || e == 0xA9 || e == 0xAF)) return 3;
        if (c == 0xE2 && d == 0x81 && e == 0x9F) return 3;
        if (c == 0xE3 && d == 0x80 && e == 0x80) return 3;
    }
    return 0;
}

// BufRead::lines() yields an error for a line that is not valid UTF-8, and every loader of the reference turns that into
// "unable to load ..." (src/alignment.rs:238-240, src/filter.rs:119-121, src/misc.rs:109-111).  Lines are ASCII in
// practice: eight bytes at a time until a byte with its top bit set shows up, the full check (overlong forms, surrogates,
// code points beyond U+10FFFF as Rust's str::from_utf8 rejects them) only from there.
inline bool valid_utf8(const char *s, size_t n) {
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t w;
        memcpy(&w, s + i, 8);
        if (w & 0x8080808080808080ull) break;
    }
    while (i < n) {
        const unsigned char c = (unsigned char)s[i];
        if (c < 0x80) { i++; continue; }
        size_t need;
        uint32_t cp;
        if ((c & 0xE0) == 0xC0) { need = 1; cp = c & 0x1Fu; if (cp < 2) return false; }
        else if ((c & 0xF0) == 0xE0) { need = 2; cp = c & 0x0Fu; }
        else if ((c & 0xF8) == 0xF0) { need = 3; cp = c & 0x07u; if (cp > 4) return false; }
        else return false;
        for (size_t k = 1; k <= need; k++) {
            if (i + k >= n) return false;  // truncated sequence
            const unsigned char cc = (unsigned char)s[i + k];
            if ((cc & 0xC0) != 0x80) return false;
            cp = (cp << 6) | (cc & 0x3Fu);
        }
        if (need == 2 && (cp < 0x800 || (cp >= 0xD800 && cp <= 0xDFFF))) return false;
        if (need == 3 && (cp < 0x10000 || cp > 0x10FFFF)) return false;
        i += need + 1;
    }
    return true;
}

// A whole file as read-only bytes: mmap for regular files, read() for pipes.
struct FileText {
    const char *text = nullptr;
    size_t size = 0;
    void *map = nullptr;
    int fd = -1;
    std::vector<char> fallback;
    FileText() = default;
    FileText(const FileText &) = delete;
    FileText &operator=(const FileText &) = delete;
    ~FileText() { close_file(); }
    void close_file() {
        if (map) munmap(map, size);
        if (fd >= 0) ::close(fd);
        map = nullptr;
        fd = -1;
    }
    bool open_file(const char *path) {
        if (PrefetchedFile *f = prefetch_take(path)) {  // opened, mapped and pre-faulted ahead of time
            map = f->map; size = f->size; fd = f->fd;
            text = (const char *)map;
            delete f;
            return true;
        }
        fd = ::open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0) return false;
        if (S_ISREG(st.st_mode) && st.st_size > 0) {
            size = (size_t)st.st_size;
            map = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (map == MAP_FAILED) { map = nullptr; return false; }
            madvise(map, size, MADV_SEQUENTIAL);
            text = (const char *)map;
            return true;
        }
        char tmp[1 << 16];
        ssize_t r;
        while ((r = ::read(fd, tmp, sizeof tmp)) > 0) fallback.insert(fallback.end(), tmp, tmp + r);
        if (r < 0) return false;
        text = fallback.data();
        size = fallback.size();
        return true;
    }
};

// [beg, end) of slice t of `threads` line-aligned slices of the text
inline void line_slices(const char *text, size_t size, unsigned threads, std::vector<const char *> &cut) {
    cut.assign(threads + 1, text + size);
    const char *p = text, *end = text + size;
    for (unsigned t = 0; t < threads; t++) {
        cut[t] = p;
        const char *want = (t + 1 == threads) ? end : text + (size / threads) * (t + 1);
        if (want < p) want = p;
        if (want < end) {
            const char *nl = (const char *)memchr(want, '\n', (size_t)(end - want));
            want = nl ? nl + 1 : end;
        }
        p = want;
    }
    cut[threads] = end;
}

// ---- the run log on stderr ----
struct Log {
    bool quiet;
    void operator()(const char *fmt, ...) const {
        if (quiet) return;
        va_list ap;
        va_start(ap, fmt);
        vfprintf(stderr, fmt, ap);
        va_end(ap);
    }
};

// num-format's Locale::en grouping (polish.rs:99 etc.)
inline std::string commas(uint64_t v) {
    std::string s = std::to_string(v), out;
    const int n = (int)s.size();
    for (int i = 0; i < n; i++) {
        out.push_back(s[i]);
        const int left = n - 1 - i;
        if (left > 0 && left % 3 == 0) out.push_back(',');
    }
    return out;
}

// PP_TIMING=1: "[timing] <prefix><stage, padded to width>  <seconds since this was made>", and with since_process
// "  (process <seconds since the process started>)" behind it
struct Lap {
    const char *prefix;
    int width;
    bool since_process;
    bool on = getenv("PP_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double seconds() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    void operator()(const char *what) const {
        if (!on) return;
        char tail[48] = "";
        if (since_process) snprintf(tail, sizeof tail, "  (process %7.3f s)", seconds_since_process_start());
        fprintf(stderr, "[timing] %s%-*s %8.3f s%s\n", prefix, width, what, seconds(), tail);
    }
};

// ---- text of the run log (the reference pins these three with unit tests; exported as pp_log_text) ----
// qscore, polish.rs:290-300
inline std::string qscore(double identity) {
    if (identity >= 100.0) return "Q\xE2\x88\x9E";
    if (identity <= 0.0) return "Q0";
    char buf[64];
    snprintf(buf, sizeof buf, "Q%.2f", -10.0 * log10(1.0 - identity / 100.0));
    return buf;
}

// format_duration, misc.rs:195-201
inline std::string format_duration_us(uint64_t us) {
    char buf[64];
    snprintf(buf, sizeof buf, "%llu:%02llu:%02llu.%06llu", (unsigned long long)(us / 1000000 / 3600),
             (unsigned long long)(us / 1000000 / 60 % 60), (unsigned long long)(us / 1000000 % 60),
             (unsigned long long)(us % 1000000));
    return buf;
}
inline std::string format_duration(double seconds) { return format_duration_us((uint64_t)(seconds * 1e6)); }

// f64::to_string: the shortest decimal string that reads back as the same double, never in exponent form
inline std::string shortest_decimal(double v) {
    char b[400];
    for (int decimals = 0; decimals <= 340; decimals++) {
        snprintf(b, sizeof b, "%.*f", decimals, v);
        if (strtod(b, nullptr) == v) break;
    }
    return b;
}

// get_percentile_name, filter.rs:262-270
inline std::string percentile_name(double p) {
    const std::string s = shortest_decimal(p);
    const char *suffix = "th";
    if (s.back() == '1' && p != 11.0) suffix = "st";
    else if (s.back() == '2' && p != 12.0) suffix = "nd";
    else if (s.back() == '3' && p != 13.0) suffix = "rd";
    return s + suffix + " percentile";
}

// The rank of get_percentile (filter.rs:249-259) among n values, 1-based: max(ceil(p / 100 * n) as usize, 1), in double as the
// reference computes it (`as usize` saturates).  The value is element rank - 1 of the sorted values, or 0 when rank - 1 >= n.
// One definition for the host reduction of the file drivers (pp_filter_host.cpp) and the device selection (pp_filter_thresholds).
inline size_t percentile_rank(double p, uint64_t n) {
    const double r = ceil(p / 100.0 * (double)n);
    const size_t rank = r <= 0.0 ? 0 : (r >= 1.8e19 ? SIZE_MAX : (size_t)r);
    return rank < 1 ? 1 : rank;
}

// the range checks of --low / --high (check_inputs, filter.rs:47-52): the message, or nullptr
inline const char *percentile_options_error(double low, double high) {
    if (low <= 0.0 || low >= 50.0) return "--low must be greater than 0 and less than 50";
    if (high <= 50.0 || high >= 100.0) return "--high must be greater than 50 and less than 100";
    return nullptr;
}

}  // namespace pph
