// pp_k_bed.h -- pp_status_bed / pp_polish_bed: the runs of equal per-position status (PP_ST_*) as BED text, and pp_polish_masked: the
// polished bytes with the bytes of selected positions in lower case; both made on the device.  Part of pp_polish_text.hip (included there,
// behind pp_k_vcf.h, whose scan, contig search, record bisection and emitted-length passes it shares, and nowhere else: it defines
// __global__ kernels).  Nothing here runs unless a caller asks for it: the polish pipeline itself is untouched.  tests/bed_model.py
// defines the bytes; pp_bed_host.h holds the argument checks and one line's arithmetic (bed::line_len, bed::line_byte: constexpr, the
// very functions tools/bed_host_check.cpp runs on the CPU).
//
// The BED passes, BED_TILE positions a workgroup, BED_PPT consecutive ones a thread.  A status byte above 5 is selected by no mask.
//   k_bed_runs     a position STARTS a run iff its status is selected and it is its contig's first position or its predecessor's status
//                  differs; it ENDS one iff it is selected and its contig's last position or its successor's status differs.  The
//                  starts per workgroup                                    -> k_colscan<1>: the first record of each workgroup.
//                  The first status byte above 5, if any, by atomicMin (the host refuses the call)
//   k_bed_recs     every start writes (a, status, contig), every end b, into its record's row: a position's record is the scan of
//                  the starts.  No thread walks a run
//   k_bed_reclen   a thread a record: its line's length, the sums per workgroup -> k_colscan<1>; the positions per status
//   k_vcf_recoff   (pp_k_vcf.h) where each line begins in the text
//   k_bed_text     the OUTPUT is cut, as in k_vcf_text: a lane owns 16 bytes of text and writes them with one aligned 16-byte store;
//                  it finds the record of its first byte by bisection and makes every byte from the record's row.  Lines are short
//                  (a name, two numbers, a word): there is no bulk to copy, every byte is computed
// No byte outside the status array, the contig table and the names is loaded: the status array may have any alignment and end where
// its allocation ends, so a thread takes its 8 bytes with one load only where they are 8-byte aligned and all inside the array.
//
// The mask pass, cut by POSITIONS (the status is per position; where a position's bytes lie in the output is the scan of the emitted
// lengths, k_vcf_multi / k_vcf_sum / k_colscan<1> as pp_polish_vcf runs them):
//   (copy)         the polished bytes are copied whole, device to device, at the memory's rate
//   k_bed_mask     a thread reads the 8 codes and 8 status bytes of its positions (one 8-byte load each) and stores the lower-case form
//                  of every byte 'A'..'Z' a selected position emits -- bytes only, each one written by the one thread that owns its
//                  position, so no store touches a byte of a neighbour.  An unselected position, or one that emits nothing, stores
//                  nothing: with the undecided few selected the pass is two streamed reads and a handful of stores.
#pragma once

namespace pp {

namespace bed = pp_bed_host;

constexpr u32 BED_THREADS = VCF_THREADS, BED_PPT = 8, BED_TILE = BED_THREADS * BED_PPT;  // positions per workgroup of the position passes
constexpr u32 BED_LANE = 16, BED_TEXT_TILES = 4, BED_TEXT_WG = BED_THREADS * BED_LANE * BED_TEXT_TILES;  // text bytes per store | per workgroup
constexpr u32 BED_NO_STATUS = 0xFFu;  // stands for the neighbours a position does not have: selected by no mask, equal to no status

struct BedJob {
    const u8 *status;  // G bytes, any alignment
    const u64 *contig_off;
    u32 nc, mask;
    u64 G;
};

struct BedRec {  // one run [a, b) (global positions) of status st inside contig c
    u32 a, b, st, c;
};

__device__ __forceinline__ bool bed_selected(u32 mask, u32 st) { return st < bed::N_STATUS && ((mask >> st) & 1u); }

// the status bytes of the thread's BED_PPT positions from p0 on (p0 < G), BED_NO_STATUS at and behind G
__device__ __forceinline__ uint2 bed_load(const u8 *__restrict__ status, u64 p0, u64 G) {
    static_assert(BED_PPT == 8, "one 8-byte load of status bytes per thread");
    if (p0 + BED_PPT <= G && ((uintptr_t)(status + p0) & 7u) == 0u) return *(const uint2 *)(status + p0);
    uint2 v = make_uint2(~0u, ~0u);
    for (u32 i = 0; i < BED_PPT; i++)
        if (p0 + i < G) {
            u32 &w = i < 4u ? v.x : v.y;
            w = (w & ~(0xFFu << (8u * (i & 3u)))) | ((u32)status[p0 + i] << (8u * (i & 3u)));
        }
    return v;
}
__device__ __forceinline__ u32 bed_byte_of(const uint2 v, u32 i) { return ((i < 4u ? v.x : v.y) >> (8u * (i & 3u))) & 0xFFu; }

// f(p, st, start, end, c) for every selected position of the thread's, in order; c: its contig
template <class F>
__device__ __forceinline__ void bed_walk(const BedJob &J, u64 p0, F f) {
    if (p0 >= J.G) return;
    const uint2 v = bed_load(J.status, p0, J.G);
    bool any = false;
#pragma unroll
    for (u32 i = 0; i < BED_PPT; i++) any = any || bed_selected(J.mask, bed_byte_of(v, i));
    if (!any) return;  // (nothing selected here: no start, no end)
    u32 prev = p0 ? (u32)J.status[p0 - 1] : BED_NO_STATUS;
    const u32 behind = p0 + BED_PPT < J.G ? (u32)J.status[p0 + BED_PPT] : BED_NO_STATUS;
    u32 c = vcf_contig(J.contig_off, J.nc, p0);
    u64 first = J.contig_off[c], next = J.contig_off[c + 1];
#pragma unroll
    for (u32 i = 0; i < BED_PPT; i++) {
        const u64 p = p0 + i;
        const u32 me = bed_byte_of(v, i);
        const u32 nx = i + 1u < BED_PPT ? bed_byte_of(v, i + 1u) : behind;
        if (p < J.G && bed_selected(J.mask, me)) {
            while (p >= next) {  // (contigs without a position are stepped over)
                c++;
                first = next;
                next = J.contig_off[c + 1];
            }
            f(p, me, p == first || prev != me, p + 1u == next || nx != me, c);
        }
        prev = me;
    }
}

__global__ __launch_bounds__(BED_THREADS) void k_bed_runs(BedJob J, u64 *__restrict__ bcnt, u64 *__restrict__ bad) {
    __shared__ u64 s_w[BED_THREADS / 64];
    const u64 p0 = ((u64)blockIdx.x * BED_THREADS + threadIdx.x) * BED_PPT;
    if (p0 < J.G) {
        const uint2 v = bed_load(J.status, p0, J.G);
        for (u32 i = 0; i < BED_PPT; i++)
            if (p0 + i < J.G && bed_byte_of(v, i) >= bed::N_STATUS) {
                atomicMin(bad, p0 + i);
                break;
            }
    }
    u32 n_start = 0;
    bed_walk(J, p0, [&](u64, u32, bool start, bool, u32) { n_start += start ? 1u : 0u; });
    u64 total;
    (void)vcf_scan(n_start, s_w, &total);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(BED_THREADS) void k_bed_recs(BedJob J, const u64 *__restrict__ roff, u64 n_rec, BedRec *__restrict__ rec) {
    __shared__ u64 s_w[BED_THREADS / 64];
    const u64 p0 = ((u64)blockIdx.x * BED_THREADS + threadIdx.x) * BED_PPT;
    u32 n_start = 0;
    bed_walk(J, p0, [&](u64, u32, bool start, bool, u32) { n_start += start ? 1u : 0u; });
    u64 total;
    u64 r = roff[blockIdx.x] + vcf_scan(n_start, s_w, &total);  // records that start in front of the thread's positions
    bed_walk(J, p0, [&](u64 p, u32 st, bool start, bool end, u32 c) {
        if (start && r < n_rec) {
            rec[r].a = (u32)p;
            rec[r].st = st;
            rec[r].c = c;
        }
        if (start) r++;
        if (end && r >= 1u && r - 1u < n_rec) rec[r - 1u].b = (u32)p + 1u;  // (its run's start lies at or in front of it: counted in r)
    });
}

// rec_at[r]: the line's length; bsum: the lengths per workgroup; counts[st] += the positions of the records of status st
__global__ __launch_bounds__(BED_THREADS) void k_bed_reclen(const BedRec *__restrict__ rec, u64 n_rec, const u64 *__restrict__ contig_off, u32 nc,
                                                            const u64 *__restrict__ name_off, u64 *__restrict__ rec_at, u64 *__restrict__ bsum,
                                                            u64 *__restrict__ counts) {
    __shared__ u64 s_w[BED_THREADS / 64];
    const u64 r = (u64)blockIdx.x * BED_THREADS + threadIdx.x;
    u64 l = 0, n_pos = 0;
    u32 st = bed::N_STATUS;
    if (r < n_rec) {
        const BedRec R = rec[r];
        const u32 c = min(R.c, nc - 1u);
        const u64 lo = contig_off[c];
        l = bed::line_len(name_off[c + 1] - name_off[c], R.a - lo, R.b - lo, R.st);
        rec_at[r] = l;
        st = R.st;
        n_pos = R.b - R.a;
    }
    for (u32 s = 0; s < bed::N_STATUS; s++) {
        const u64 v = wave_sum64(st == s ? n_pos : 0ull);
        if ((threadIdx.x & 63u) == 0u && v) atomicAdd(&counts[s], v);
    }
    u64 total;
    (void)vcf_scan(l, s_w, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

struct BedText {
    const u8 *names;
    const u64 *name_off, *contig_off, *rec_at;  // rec_at: n_rec + 1
    const BedRec *rec;
    u32 nc;
    u64 n_rec, n_text;
};
struct BedLine {  // a record as the text pass sees it
    u64 at, end;  // its bytes in the text
    const u8 *name;
    u64 nlen, a, b;  // a, b: local to the contig
    u32 na, nb, st;
};
__device__ __forceinline__ void bed_line(const BedText &X, u64 r, BedLine &L) {
    const BedRec R = X.rec[r];
    const u32 c = min(R.c, X.nc - 1u);
    const u64 lo = X.contig_off[c];
    L.at = X.rec_at[r];
    L.end = X.rec_at[r + 1u];
    L.name = X.names + X.name_off[c];
    L.nlen = X.name_off[c + 1] - X.name_off[c];
    L.a = R.a - lo;
    L.b = R.b - lo;
    L.na = bed::ndig(L.a);
    L.nb = bed::ndig(L.b);
    L.st = R.st;
}

// the text's allocation is a multiple of 16 bytes (zeros behind the text): every lane that owns a byte stores 16
__global__ __launch_bounds__(BED_THREADS) void k_bed_text(BedText X, u8 *__restrict__ dst) {
    __shared__ u64 s_r[2];
    const u32 tid = threadIdx.x;
    const u64 g0 = (u64)blockIdx.x * BED_TEXT_WG, g1 = min(X.n_text, g0 + (u64)BED_TEXT_WG);  // (g0 < n_text: the grid; n_rec >= 1)
    if (tid < 2u) s_r[tid] = vcf_record_of(X.rec_at, 0, X.n_rec - 1u, tid ? g1 - 1u : g0);  // the records of the stretch's first and last byte
    __syncthreads();
    const u64 r_lo = s_r[0], r_hi = s_r[1];
    for (u32 ti = 0; ti < BED_TEXT_TILES; ti++) {
        const u64 t0 = g0 + (u64)ti * (BED_THREADS * BED_LANE) + (u64)tid * BED_LANE;
        if (t0 >= X.n_text) break;  // (no lane waits for another below)
        u64 r = vcf_record_of(X.rec_at, r_lo, r_hi, t0);
        BedLine L;
        bed_line(X, r, L);
        u32 w0 = 0, w1 = 0, w2 = 0, w3 = 0;  // (selected by comparison, the loop not unrolled: no indexed register array)
#pragma unroll 1
        for (u32 j = 0; j < BED_LANE; j++) {
            const u64 t = t0 + j;
            u32 b = 0;
            if (t < X.n_text) {
                if (t >= L.end && r + 1u < X.n_rec) {  // (no line is empty: at most one step per byte)
                    r++;
                    bed_line(X, r, L);
                }
                b = bed::line_byte(L.name, L.nlen, L.a, L.na, L.b, L.nb, L.st, t - L.at);
            }
            const u32 sh = b << (8u * (j & 3u)), q = j >> 2;
            w0 |= q == 0u ? sh : 0u;
            w1 |= q == 1u ? sh : 0u;
            w2 |= q == 2u ? sh : 0u;
            w3 |= q == 3u ? sh : 0u;
        }
        *(uint4 *)(dst + t0) = make_uint4(w0, w1, w2, w3);
    }
}

// ---- the mask pass: dst is a copy of J.out already ----
// status: the job's own plane (256-byte aligned, G bytes); boff: where each workgroup's emitted bytes begin (k_vcf_sum, k_colscan<1>)
__global__ __launch_bounds__(VCF_THREADS) void k_bed_mask(VcfJob J, const u64 *__restrict__ boff, const u8 *__restrict__ status, u32 mask,
                                                          u8 *__restrict__ dst) {
    __shared__ u64 s_w[VCF_THREADS / 64];
    static_assert(VCF_PPT == BED_PPT, "one 8-byte load of codes and one of status bytes per thread");
    const u64 p0 = ((u64)blockIdx.x * VCF_THREADS + threadIdx.x) * VCF_PPT;
    u32 c[VCF_PPT], len[VCF_PPT];
    const u32 s = vcf_lens(J, p0, c, len);
    u64 total;
    u64 o = boff[blockIdx.x] + vcf_scan(s, s_w, &total);
    if (p0 >= J.G) return;
    const uint2 v = bed_load(status, p0, J.G);
    for (u32 i = 0; i < VCF_PPT; i++) {
        if (len[i] && bed_selected(mask, bed_byte_of(v, i)))
            for (u64 q = o; q < o + len[i] && q < J.total_out; q++) {  // (a multi-byte winner is lower-cased whole)
                const u32 b = J.out[q];
                if (b >= (u32)'A' && b <= (u32)'Z') dst[q] = (u8)(b | 0x20u);
            }
        o += len[i];
    }
}

}  // namespace pp
