// pp_k_vcf.h -- pp_polish_vcf: the polish's edits as VCF text, made on the device from what a finished job leaves there: the assembly
// bases, the emit codes (code_len, pp_k_emit.h), the multi-byte winners' list and the polished bytes.  Part of pp_polish_text.hip
// (included there, after pp_k_debug.h, and nowhere else: it defines __global__ kernels).  Nothing here runs unless a caller asks for
// the VCF: the polish pipeline itself is untouched.  tests/vcf_model.py defines the bytes; pp_vcf_host.h builds the header.  The
// single-workgroup scan of the workgroups' sums is pp_dev.h's k_colscan<1>, the 16-byte cuts of k_vcf_text are pp_cut16.h's.
//
// The seq array is NOT read (a caller may have released it): a position's emitted bytes are the polished output at the scan of the
// emitted lengths.  The passes, VCF_TILE positions a workgroup, VCF_PPT consecutive ones a thread:
//   k_vcf_multi    the emitted length of every position whose code does not hold it (0xFF), from the multi-byte winners' list
//   k_vcf_sum      the emitted bytes per workgroup                         -> k_colscan<1>: where each workgroup's bytes begin
//   k_vcf_mark     a flag per position: EDITED iff it does not emit exactly its assembly byte (codes 1..127: the code itself; a
//                  multi-byte code of one byte: that byte of the polished output)
//   k_vcf_runs     the flags of the two neighbours and the contig table make run STARTS and ENDS (no run joins across a contig
//                  boundary), and the starts per workgroup                 -> k_colscan<1>: the first record of each workgroup
//   k_vcf_recs     every start writes (a, output offset of a), every end (b, output offset of b) into its record's row: a
//                  position's record is the scan of the starts.  No thread walks a run
//   k_vcf_reclen   a thread a record: its case (vcf_fields: the table in vcf_model.py), its line's length, the sums per workgroup
//                                                                          -> k_colscan<1>
//   k_vcf_recoff   where each line begins in the text
//   k_vcf_text     the OUTPUT is cut, as in k_fasta_text: a lane owns 16 bytes of text and writes them with one aligned 16-byte
//                  store; it finds the record of its first byte by bisection and takes every byte from where the record says it
//                  lies -- REF is bases[ref_at, ref_at + reflen), ALT is out[oa, ob) or one anchor byte.  A lane whose 16 bytes lie
//                  inside one REF or ALT takes them from the one or two aligned 16-byte pieces that hold them (wide loads only where
//                  the piece lies wholly inside the array).  One run of the whole assembly is so copied at the memory's rate, by as
//                  many lanes as its text has 16-byte words.
// Device memory beyond the text: 2 flag bytes per position, 4 more when the job has multi-byte winners, 40 bytes per record.
#pragma once
#include "pp_cut16.h"

namespace pp {

constexpr u32 VCF_THREADS = 256, VCF_PPT = 8, VCF_TILE = VCF_THREADS * VCF_PPT;  // positions per workgroup of the position passes
constexpr u32 VCF_LANE = 16, VCF_TEXT_TILES = 4, VCF_TEXT_WG = VCF_THREADS * VCF_LANE * VCF_TEXT_TILES;  // text bytes per store | per workgroup
constexpr u8 VCF_EDITED = 1, VCF_START = 2, VCF_END = 4;

struct VcfJob {
    const u8 *bases, *code, *out;
    const u32 *mlen;  // emitted length of the positions with code 0xFF (nullptr: the job has no multi-byte winner)
    const u64 *contig_off;
    u32 nc;
    u64 G, total_out;
};

struct VcfRec {  // one run [a, b) of edited positions (global), and where its emitted bytes lie in the polished output: [oa, ob)
    u64 a, oa, b, ob;
};

__global__ __launch_bounds__(256) void k_vcf_multi(const MultiEnt *__restrict__ multi, u32 nm, const u8 *__restrict__ code, u64 G,
                                                   u32 *__restrict__ mlen) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nm) return;
    const u32 pos = multi[i].pos;
    if (pos < G && code[pos] == 0xFFu) mlen[pos] = multi[i].eff;
}

// code_len (pp_k_emit.h) with the list's search replaced by the table k_vcf_multi made of it
__device__ __forceinline__ u32 vcf_len(const VcfJob &J, u32 c, u64 p) {
    if (c == 0u) return 0u;
    if (c < 0x80u) return 1u;
    if (c != 0xFFu) return c & 0x7Fu;
    return J.mlen ? J.mlen[p] : 0u;
}

// the codes and emitted lengths of the thread's VCF_PPT positions from p0 on (p0 a multiple of VCF_PPT; zero at and behind G)
__device__ __forceinline__ u32 vcf_lens(const VcfJob &J, u64 p0, u32 c[VCF_PPT], u32 len[VCF_PPT]) {
    static_assert(VCF_PPT == 8, "one 8-byte load of codes per thread");
    uint2 v = make_uint2(0u, 0u);
    if (p0 + VCF_PPT <= J.G) v = *(const uint2 *)(J.code + p0);  // (the code array is 256-byte aligned)
    else
        for (u32 i = 0; i < VCF_PPT; i++)
            if (p0 + i < J.G) (i < 4u ? v.x : v.y) |= (u32)J.code[p0 + i] << (8u * (i & 3u));
    u32 s = 0;
#pragma unroll
    for (u32 i = 0; i < VCF_PPT; i++) {
        c[i] = ((i < 4u ? v.x : v.y) >> (8u * (i & 3u))) & 0xFFu;
        len[i] = p0 + i < J.G ? vcf_len(J, c[i], p0 + i) : 0u;
        s += len[i];
    }
    return s;
}

// exclusive prefix of v over the workgroup's VCF_THREADS threads, *total = its sum (s_w: VCF_THREADS / 64 words, free again on return)
__device__ __forceinline__ u64 vcf_scan(u64 v, u64 *s_w, u64 *total) {
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u64 inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 x = __shfl_up(inc, o, 64);
        if ((int)lane >= o) inc += x;
    }
    if (lane == 63u) s_w[wave] = inc;
    __syncthreads();
    u64 before = 0, sum = 0;
#pragma unroll
    for (u32 i = 0; i < VCF_THREADS / 64u; i++) {
        const u64 w = s_w[i];
        before += i < wave ? w : 0ull;
        sum += w;
    }
    __syncthreads();
    *total = sum;
    return before + inc - v;
}

__global__ __launch_bounds__(VCF_THREADS) void k_vcf_sum(VcfJob J, u64 *__restrict__ bsum) {
    __shared__ u64 s_w[VCF_THREADS / 64];
    const u64 p0 = ((u64)blockIdx.x * VCF_THREADS + threadIdx.x) * VCF_PPT;
    u32 c[VCF_PPT], len[VCF_PPT];
    const u32 s = vcf_lens(J, p0, c, len);
    u64 total;
    (void)vcf_scan(s, s_w, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(VCF_THREADS) void k_vcf_mark(VcfJob J, const u64 *__restrict__ boff, u8 *__restrict__ flag) {
    __shared__ u64 s_w[VCF_THREADS / 64];
    const u64 p0 = ((u64)blockIdx.x * VCF_THREADS + threadIdx.x) * VCF_PPT;
    u32 c[VCF_PPT], len[VCF_PPT];
    const u32 s = vcf_lens(J, p0, c, len);
    u64 total;
    u64 o = boff[blockIdx.x] + vcf_scan(s, s_w, &total);
    if (p0 >= J.G) return;
    uint2 b = make_uint2(0u, 0u);
    if (p0 + VCF_PPT <= J.G && ((uintptr_t)(J.bases + p0) & 7u) == 0u) b = *(const uint2 *)(J.bases + p0);
    else
        for (u32 i = 0; i < VCF_PPT; i++)
            if (p0 + i < J.G) (i < 4u ? b.x : b.y) |= (u32)J.bases[p0 + i] << (8u * (i & 3u));
    uint2 f = make_uint2(0u, 0u);
#pragma unroll
    for (u32 i = 0; i < VCF_PPT; i++) {
        const u32 base = ((i < 4u ? b.x : b.y) >> (8u * (i & 3u))) & 0xFFu;
        bool same = false;
        if (len[i] == 1u) {
            const u32 e = c[i] < 0x80u ? c[i] : (o < J.total_out ? (u32)J.out[o] : 0x100u);
            same = e == base;
        }
        if (p0 + i < J.G && !same) (i < 4u ? f.x : f.y) |= (u32)VCF_EDITED << (8u * (i & 3u));
        o += len[i];
    }
    *(uint2 *)(flag + p0) = f;  // (the flag arrays have room up to a multiple of VCF_PPT)
}

// the last c with contig_off[c] <= p (p < G: it is a contig that holds p)
__device__ __forceinline__ u32 vcf_contig(const u64 *__restrict__ contig_off, u32 nc, u64 p) {
    u32 lo = 0, hi = nc;  // contig_off[lo] <= p < contig_off[hi]
    while (hi - lo > 1u) {
        const u32 mid = (lo + hi) >> 1;
        if (contig_off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(VCF_THREADS) void k_vcf_runs(VcfJob J, const u8 *__restrict__ flag, u8 *__restrict__ flag2, u64 *__restrict__ bcnt) {
    __shared__ u64 s_w[VCF_THREADS / 64];
    const u64 p0 = ((u64)blockIdx.x * VCF_THREADS + threadIdx.x) * VCF_PPT;
    u32 n_start = 0;
    if (p0 < J.G) {
        const uint2 f = *(const uint2 *)(flag + p0);
        u32 prev = p0 ? (u32)flag[p0 - 1] : 0u;
        const u32 behind = p0 + VCF_PPT < J.G ? (u32)flag[p0 + VCF_PPT] : 0u;
        uint2 g = make_uint2(0u, 0u);
        if ((f.x | f.y) != 0u) {  // (nothing edited here: no start, no end)
            u32 c = vcf_contig(J.contig_off, J.nc, p0);
            u64 first = J.contig_off[c], next = J.contig_off[c + 1];
#pragma unroll
            for (u32 i = 0; i < VCF_PPT; i++) {
                const u64 p = p0 + i;
                const u32 me = ((i < 4u ? f.x : f.y) >> (8u * (i & 3u))) & 1u;
                const u32 nx = i + 1u < VCF_PPT ? ((i + 1u < 4u ? f.x : f.y) >> (8u * ((i + 1u) & 3u))) & 1u : behind & 1u;
                if (p < J.G && me) {
                    while (p >= next) {  // (contigs without a base are stepped over)
                        c++;
                        first = next;
                        next = J.contig_off[c + 1];
                    }
                    const bool start = p == first || !(prev & 1u), end = p + 1u == next || !nx;
                    n_start += start ? 1u : 0u;
                    (i < 4u ? g.x : g.y) |= (u32)(VCF_EDITED | (start ? VCF_START : 0) | (end ? VCF_END : 0)) << (8u * (i & 3u));
                }
                prev = me;
            }
        }
        *(uint2 *)(flag2 + p0) = g;
    }
    u64 total;
    (void)vcf_scan(n_start, s_w, &total);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(VCF_THREADS) void k_vcf_recs(VcfJob J, const u8 *__restrict__ flag2, const u64 *__restrict__ boff,
                                                          const u64 *__restrict__ roff, u64 n_rec, VcfRec *__restrict__ rec) {
    __shared__ u64 s_w[VCF_THREADS / 64];
    const u64 p0 = ((u64)blockIdx.x * VCF_THREADS + threadIdx.x) * VCF_PPT;
    u32 c[VCF_PPT], len[VCF_PPT];
    const u32 s = vcf_lens(J, p0, c, len);
    uint2 f = make_uint2(0u, 0u);
    if (p0 < J.G) f = *(const uint2 *)(flag2 + p0);
    u32 n_start = 0;
#pragma unroll
    for (u32 i = 0; i < VCF_PPT; i++) n_start += ((i < 4u ? f.x : f.y) >> (8u * (i & 3u) + 1u)) & 1u;
    u64 total;
    u64 o = boff[blockIdx.x] + vcf_scan(s, s_w, &total);
    u64 r = roff[blockIdx.x] + vcf_scan(n_start, s_w, &total);  // records that start in front of the thread's positions
    if ((f.x | f.y) == 0u) return;
#pragma unroll
    for (u32 i = 0; i < VCF_PPT; i++) {
        const u32 fl = ((i < 4u ? f.x : f.y) >> (8u * (i & 3u))) & 0xFFu;
        if ((fl & VCF_START) && r < n_rec) {
            rec[r].a = p0 + i;
            rec[r].oa = o;
        }
        if (fl & VCF_START) r++;
        o += len[i];
        if ((fl & VCF_END) && r >= 1u && r - 1u < n_rec) {  // (its run's start lies at or in front of it: counted in r)
            rec[r - 1u].b = p0 + i + 1u;
            rec[r - 1u].ob = o;
        }
    }
}

// ---- one record's line: name \t POS \t . \t REF \t ALT \t . \t . \t . \n ---------------------------------------------------------------
struct VcfFields {
    u64 pos;      // 1-based, local to the contig
    u64 ref_at;   // REF = bases[ref_at, ref_at + reflen)
    u64 reflen;
    u64 alt_at;   // ALT = kind 0: out[alt_at, alt_at + altlen) | 1: the one byte bases[alt_at] | 2: "<DEL>"
    u64 altlen;
    u32 kind, nd;
};
__device__ __forceinline__ void vcf_fields(const VcfRec &R, u64 lo, u64 hi, VcfFields &F) {  // [lo, hi): the run's contig
    const u64 alen = R.ob - R.oa;
    if (alen) {
        F.pos = R.a - lo + 1u; F.ref_at = R.a; F.reflen = R.b - R.a; F.kind = 0; F.alt_at = R.oa; F.altlen = alen;
    } else if (R.a > lo) {  // a deletion: anchored on the base in front of it (unedited: the run is maximal)
        F.pos = R.a - lo; F.ref_at = R.a - 1u; F.reflen = R.b - R.a + 1u; F.kind = 1; F.alt_at = R.a - 1u; F.altlen = 1;
    } else if (R.b < hi) {  // ... at the contig's start: on the base behind it
        F.pos = 1; F.ref_at = R.a; F.reflen = R.b - R.a + 1u; F.kind = 1; F.alt_at = R.b; F.altlen = 1;
    } else {                // the whole contig
        F.pos = 1; F.ref_at = R.a; F.reflen = R.b - R.a; F.kind = 2; F.alt_at = 0; F.altlen = 5;
    }
    F.nd = dfmt_ndig(F.pos);
}
constexpr u32 VCF_FIXED = 12;  // the line's tabs, dots and newline

__global__ __launch_bounds__(VCF_THREADS) void k_vcf_reclen(const VcfRec *__restrict__ rec, u64 n_rec, const u64 *__restrict__ contig_off, u32 nc,
                                                            const u64 *__restrict__ name_off, u64 *__restrict__ rec_at, u64 *__restrict__ bsum) {
    __shared__ u64 s_w[VCF_THREADS / 64];
    const u64 r = (u64)blockIdx.x * VCF_THREADS + threadIdx.x;
    u64 l = 0;
    if (r < n_rec) {
        const VcfRec R = rec[r];
        const u32 c = vcf_contig(contig_off, nc, R.a);
        VcfFields F;
        vcf_fields(R, contig_off[c], contig_off[c + 1], F);
        l = (name_off[c + 1] - name_off[c]) + F.nd + F.reflen + F.altlen + VCF_FIXED;
        rec_at[r] = l;
    }
    u64 total;
    (void)vcf_scan(l, s_w, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// rec_at[r]: the line's length -> its first byte in the text (H: the header's bytes); rec_at[n_rec] = the text's length
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_recoff(u64 n_rec, const u64 *__restrict__ boff, u64 H, u64 *__restrict__ rec_at) {
    __shared__ u64 s_w[VCF_THREADS / 64];
    const u64 r = (u64)blockIdx.x * VCF_THREADS + threadIdx.x;
    const u64 l = r < n_rec ? rec_at[r] : 0ull;
    u64 total;
    const u64 at = H + boff[blockIdx.x] + vcf_scan(l, s_w, &total);
    if (r < n_rec) rec_at[r] = at;
    if (r + 1u == n_rec) rec_at[n_rec] = at + l;
}

struct VcfText {
    const u8 *bases, *out, *hdr, *names;
    const u64 *name_off, *contig_off, *rec_at;  // rec_at: n_rec + 1
    const VcfRec *rec;
    u32 nc;
    u64 n_rec, G, total_out, H, n_text;
};
struct VcfLine {  // a record as the text pass sees it
    VcfFields F;
    u64 at, end;  // its bytes in the text
    u64 name_at;
    u64 nlen;
};
__device__ __forceinline__ void vcf_line(const VcfText &X, u64 r, VcfLine &L) {
    const VcfRec R = X.rec[r];
    const u32 c = vcf_contig(X.contig_off, X.nc, R.a);
    vcf_fields(R, X.contig_off[c], X.contig_off[c + 1], L.F);
    L.at = X.rec_at[r];
    L.end = X.rec_at[r + 1u];
    L.name_at = X.name_off[c];
    L.nlen = X.name_off[c + 1] - L.name_at;
}
// byte k of the line
__device__ __forceinline__ u32 vcf_byte(const VcfText &X, const VcfLine &L, u64 k) {
    if (k < L.nlen) return X.names[L.name_at + k];
    k -= L.nlen;
    if (k == 0u) return (u32)'\t';
    k -= 1u;
    if (k < L.F.nd) {
        u32 d = L.F.nd - 1u - (u32)k;  // digits behind this one
        if (L.F.pos <= 0xFFFFFFFFull) {
            u32 v = (u32)L.F.pos;
            for (; d > 0u; d--) v /= 10u;
            return (u32)'0' + v % 10u;
        }
        u64 v = L.F.pos;
        for (; d > 0u; d--) v /= 10u;
        return (u32)'0' + (u32)(v % 10u);
    }
    k -= L.F.nd;
    if (k < 3u) return k == 1u ? (u32)'.' : (u32)'\t';
    k -= 3u;
    if (k < L.F.reflen) return L.F.ref_at + k < X.G ? (u32)X.bases[L.F.ref_at + k] : (u32)'?';
    k -= L.F.reflen;
    if (k == 0u) return (u32)'\t';
    k -= 1u;
    if (k < L.F.altlen) {
        if (L.F.kind == 0u) return L.F.alt_at + k < X.total_out ? (u32)X.out[L.F.alt_at + k] : (u32)'?';
        if (L.F.kind == 1u) return L.F.alt_at < X.G ? (u32)X.bases[L.F.alt_at] : (u32)'?';
        return k == 4u ? (u32)'>' : (0x4C45443Cu >> (8u * (u32)k)) & 0xFFu;  // "<DEL" and ">"
    }
    k -= L.F.altlen;
    return k == 6u ? (u32)'\n' : ((k & 1u) ? (u32)'.' : (u32)'\t');
}

// the largest r in [lo, hi] with rec_at[r] <= t (rec_at[lo] <= t)
__device__ __forceinline__ u64 vcf_record_of(const u64 *__restrict__ rec_at, u64 lo, u64 hi, u64 t) {
    while (lo < hi) {
        const u64 mid = lo + (hi - lo + 1u) / 2u;
        if (rec_at[mid] <= t) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

// the text's allocation is a multiple of 16 bytes (zeros behind the text): every lane that owns a byte stores 16
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_text(VcfText X, u8 *__restrict__ dst) {
    __shared__ u64 s_r[2];
    const u32 tid = threadIdx.x;
    const u64 g0 = (u64)blockIdx.x * VCF_TEXT_WG, g1 = min(X.n_text, g0 + (u64)VCF_TEXT_WG);  // (g0 < n_text: the grid)
    if (tid < 2u) {  // the records of the stretch's first and last byte (none: the stretch is header)
        const u64 t = tid ? g1 - 1u : max(g0, X.H);
        s_r[tid] = X.n_rec && t >= X.H && t < X.n_text ? vcf_record_of(X.rec_at, 0, X.n_rec - 1u, t) : 0ull;
    }
    __syncthreads();
    const u64 r_lo = s_r[0], r_hi = s_r[1];
    for (u32 ti = 0; ti < VCF_TEXT_TILES; ti++) {
        const u64 t0 = g0 + (u64)ti * (VCF_THREADS * VCF_LANE) + (u64)tid * VCF_LANE;
        if (t0 >= X.n_text) break;  // (no lane waits for another below)
        uint4 v;
        if (t0 + VCF_LANE <= X.H) {
            v = *(const uint4 *)(X.hdr + t0);  // (the header's copy is 16-byte aligned)
        } else {
            bool done = false, have = false;
            u64 r = 0;
            VcfLine L;
            if (t0 >= X.H) {
                r = vcf_record_of(X.rec_at, r_lo, r_hi, t0);
                vcf_line(X, r, L);
                have = true;
                // ---- the bulk: 16 bytes of one REF, or of one ALT that lies in the polished output ----
                const u64 k0 = t0 - L.at, kr = L.nlen + 1u + L.F.nd + 3u, ka = kr + L.F.reflen + 1u;
                if (k0 >= kr && k0 + VCF_LANE <= kr + L.F.reflen && L.F.ref_at + L.F.reflen <= X.G) {
                    v = copy16(X.bases + L.F.ref_at + (k0 - kr), X.bases, X.bases + X.G);
                    done = true;
                } else if (L.F.kind == 0u && k0 >= ka && k0 + VCF_LANE <= ka + L.F.altlen && L.F.alt_at + L.F.altlen <= X.total_out) {
                    v = copy16(X.out + L.F.alt_at + (k0 - ka), X.out, X.out + X.total_out);
                    done = true;
                }
            }
            if (!done) {
                // ---- the seams: one byte at a time ----
                u32 w0 = 0, w1 = 0, w2 = 0, w3 = 0;  // (selected by comparison, the loop not unrolled: no indexed register array)
#pragma unroll 1
                for (u32 j = 0; j < VCF_LANE; j++) {
                    const u64 t = t0 + j;
                    u32 b = 0;
                    if (t < X.H) b = X.hdr[t];
                    else if (t < X.n_text) {
                        if (!have) {  // the first record begins where the header ends
                            r = 0;
                            vcf_line(X, r, L);
                            have = true;
                        }
                        if (t >= L.end && r + 1u < X.n_rec) {  // (no line is empty: at most one step per byte)
                            r++;
                            vcf_line(X, r, L);
                        }
                        b = vcf_byte(X, L, t - L.at);
                    }
                    const u32 sh = b << (8u * (j & 3u)), q = j >> 2;
                    w0 |= q == 0u ? sh : 0u;
                    w1 |= q == 1u ? sh : 0u;
                    w2 |= q == 2u ? sh : 0u;
                    w3 |= q == 3u ? sh : 0u;
                }
                v = make_uint4(w0, w1, w2, w3);
            }
        }
        *(uint4 *)(dst + t0) = v;
    }
}

}  // namespace pp
