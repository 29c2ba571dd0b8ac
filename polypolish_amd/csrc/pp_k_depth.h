// pp_k_depth.h -- pp_depth_bedgraph / pp_polish_depth: a per-position read depth (a double per position) as bedGraph text, made on the
// device: the runs of equal printed depth (bin 0, the -bga form) or the mean printed depth of fixed bins.  Part of pp_polish_text.hip
// (included there, behind pp_k_bed.h: it uses pp_k_debug.h's dfmt_tenths, pp_k_vcf.h's scan, contig search, record bisection and
// k_vcf_recoff, and nowhere else: it defines __global__ kernels).  Nothing here runs unless a caller asks for it: the polish pipeline
// itself is untouched.  tests/depth_model.py defines the bytes; pp_depth_host.h holds the argument checks, the mean's rounding and one
// line's arithmetic (dep::line_len, dep::line_byte, dep::mean_hundredths: constexpr, the very functions tools/depth_host_check.cpp
// runs on the CPU).
//
// The passes, DEP_TILE positions a workgroup, DEP_PPT consecutive ones a thread.  No plane of tenths is stored: a pass that needs a
// position's tenths makes them again from its double (the depth plane is read twice in the runs form, once in the bins form).
//   k_dep_values   every value is judged (its bits at or above those of 2^32, as an unsigned number: a set sign bit, a NaN, an infinity,
//                  2^32 or more), the first bad position by atomicMin (the host refuses the call); the positions of zero tenths, the
//                  largest tenths and their sum, reduced in the workgroup, three atomics a workgroup.
//                  <false> (runs): a position STARTS a run iff it is its contig's first position or its tenths differ from its
//                  predecessor's (the predecessor of a thread's first position is read from memory); the starts per workgroup
//                                                                          -> k_colscan<1>: the first record of each workgroup
//                  <true> (bins): a thread sums the stretches of its positions that share a bin; the stretches go into the
//                  workgroup's LDS row of bins (a wave whose 512 positions share one bin sums over the wave first), and every bin the
//                  workgroup touched takes ONE global atomicAdd of 64 bits -- a bin lies inside one contig, may span many workgroups,
//                  and a workgroup may hold DEP_TILE of them
//   k_dep_recs     (runs) every start writes (a, contig, tenths) into its record's row and closes the row in front of it (b = a)
//                  unless it is its contig's first position; a contig's last position closes its row (b = the contig's end).  A
//                  position's record is the scan of the starts.  No thread walks a run
//   k_dep_binrecs  (bins) a thread a record: its contig by bisection of the bins' table, [a, b) from the bin's number, the mean
//   k_dep_reclen   a thread a record: its line's length, the sums per workgroup -> k_colscan<1>
//   k_vcf_recoff   (pp_k_vcf.h) where each line begins in the text
//   k_dep_text     the OUTPUT is cut, as in k_bed_text: a lane owns 16 bytes of text and writes them with one aligned 16-byte store;
//                  it finds the record of its first byte by bisection and makes every byte from the record's row
// No byte outside the depth array, the tables and the names is loaded: the array is aligned to 8 bytes and may end where its
// allocation ends, so a thread takes its positions with 16-byte loads only where they are 16-byte aligned and all inside the array.
#pragma once

namespace pp {

namespace dep = pp_depth_host;

constexpr u32 DEP_THREADS = VCF_THREADS, DEP_PPT = 8, DEP_TILE = DEP_THREADS * DEP_PPT;  // positions per workgroup of the position passes
constexpr u32 DEP_LANE = 16, DEP_TEXT_TILES = 4, DEP_TEXT_WG = DEP_THREADS * DEP_LANE * DEP_TEXT_TILES;  // text bytes per store | per workgroup

struct DepJob {
    const double *depth;  // G doubles, aligned to 8 bytes
    const u64 *contig_off;
    const u64 *bin_base;  // bins form: the first record of each contig (nc + 1)
    u32 nc, bin;          // bin 0: the runs form
    u64 G;
};

struct DepRec {  // one record: [a, b) (global positions) inside contig c, its value (tenths of a run, hundredths of a bin's mean)
    u32 a, b, c, pad;
    u64 v;
};

// the bits of the thread's DEP_PPT positions from p0 on (p0 < G); zero at and behind G
__device__ __forceinline__ void dep_load(const double *__restrict__ depth, u64 p0, u64 G, u64 bits[DEP_PPT]) {
    static_assert(DEP_PPT % 2u == 0u, "16-byte loads of two positions");
    if (p0 + DEP_PPT <= G && ((uintptr_t)(depth + p0) & 15u) == 0u) {
#pragma unroll
        for (u32 i = 0; i < DEP_PPT; i += 2) {
            const uint4 w = *(const uint4 *)(depth + p0 + i);
            bits[i] = (u64)w.x | ((u64)w.y << 32);
            bits[i + 1] = (u64)w.z | ((u64)w.w << 32);
        }
        return;
    }
#pragma unroll
    for (u32 i = 0; i < DEP_PPT; i++) bits[i] = p0 + i < G ? (u64)__double_as_longlong(depth[p0 + i]) : 0ull;
}
__device__ __forceinline__ bool dep_bad(u64 bits) { return bits >= dep::DEPTH_BAD_BITS; }
// the tenths of a position (0 for a value the call is refused for)
__device__ __forceinline__ u64 dep_tenths(u64 bits) { return dep_bad(bits) ? 0ull : dfmt_tenths(__longlong_as_double((long long)bits)); }

// f(p, tenths, start, first, next, c) for every position of the thread's, in order; [first, next): its contig c
template <class F>
__device__ __forceinline__ void dep_walk(const DepJob &J, u64 p0, const u64 bits[DEP_PPT], F f) {
    if (p0 >= J.G) return;
    u64 prev = p0 ? dep_tenths((u64)__double_as_longlong(J.depth[p0 - 1])) : 0ull;
    u32 c = vcf_contig(J.contig_off, J.nc, p0);
    u64 first = J.contig_off[c], next = J.contig_off[c + 1];
#pragma unroll
    for (u32 i = 0; i < DEP_PPT; i++) {
        const u64 p = p0 + i;
        const u64 me = dep_tenths(bits[i]);
        if (p < J.G) {
            while (p >= next) {  // (contigs without a position are stepped over)
                c++;
                first = next;
                next = J.contig_off[c + 1];
            }
            f(p, me, p == first || prev != me, first, next, c);
        }
        prev = me;
    }
}

__device__ __forceinline__ u64 dep_wave_max64(u64 v) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 x = __shfl_xor(v, o, 64);
        v = x > v ? x : v;
    }
    return v;
}

// word: the first bad position | positions of zero tenths | the largest tenths | the sum of the tenths
template <bool BINS>
__global__ __launch_bounds__(DEP_THREADS) void k_dep_values(DepJob J, u64 *__restrict__ bcnt, u64 *__restrict__ bins, u64 *__restrict__ word) {
    __shared__ u64 s_w[DEP_THREADS / 64];
    __shared__ u64 s_red[3][DEP_THREADS / 64];
    __shared__ u64 s_bin[BINS ? DEP_TILE : 1u];
    __shared__ u64 s_span[2];
    const u32 tid = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * DEP_TILE, p0 = t0 + (u64)tid * DEP_PPT;
    u64 bits[DEP_PPT];
#pragma unroll
    for (u32 i = 0; i < DEP_PPT; i++) bits[i] = 0;
    if (p0 < J.G) {
        dep_load(J.depth, p0, J.G, bits);
        u32 bad_i = DEP_PPT;  // (the bits behind G are zero: never bad)
#pragma unroll
        for (u32 i = DEP_PPT; i-- > 0u;) bad_i = dep_bad(bits[i]) ? i : bad_i;
        if (bad_i < DEP_PPT) atomicMin(word, p0 + bad_i);
    }
    if constexpr (BINS) {
        for (u32 i = tid; i < DEP_TILE; i += DEP_THREADS) s_bin[i] = 0;
        if (tid == 0u) {  // the bins of the tile's first and last position (t0 < G: the grid)
            const u64 t1 = min(J.G, t0 + (u64)DEP_TILE) - 1u;
            const u32 c0 = vcf_contig(J.contig_off, J.nc, t0), c1 = vcf_contig(J.contig_off, J.nc, t1);
            s_span[0] = J.bin_base[c0] + (u32)(t0 - J.contig_off[c0]) / J.bin;  // (32-bit divisions: G is below 2^32)
            s_span[1] = J.bin_base[c1] + (u32)(t1 - J.contig_off[c1]) / J.bin;
        }
        __syncthreads();
    }
    u32 n_start = 0, n_zero = 0;
    u64 vmax = 0, vsum = 0;
    // bins form: the open stretch of the thread's positions -- its bin, its sum, how many positions the bin still takes
    u64 b_open = 0, s_open = 0, b_first = ~0ull, b_room = 0;
    bool one = true;  // the thread's positions share one bin
    dep_walk(J, p0, bits, [&](u64 p, u64 v, bool start, u64 first, u64 next, u32 c) {
        n_start += start ? 1u : 0u;
        n_zero += v == 0u ? 1u : 0u;
        vmax = v > vmax ? v : vmax;
        vsum += v;
        if constexpr (BINS) {
            if (b_first == ~0ull || p == first || b_room == 0u) {  // a bin begins with this position (or the thread does)
                if (b_first != ~0ull) {
                    atomicAdd(&s_bin[b_open - s_span[0]], s_open);
                    one = false;
                }
                const u64 k = (u32)(p - first) / J.bin;  // (a 32-bit division where a stretch begins)
                b_open = J.bin_base[c] + k;
                b_room = min(next, first + (k + 1u) * J.bin) - p;
                s_open = 0;
                if (b_first == ~0ull) b_first = b_open;
            }
            s_open += v;
            b_room--;
        }
    });
    if constexpr (BINS) {
        // a wave whose positions all share one bin: one LDS add for the wave
        const bool have = b_first != ~0ull;
        const u64 b_lane0 = __shfl(b_open, 0, 64);
        if (__all(have && one && b_open == b_lane0)) {
            const u64 s = wave_sum64(s_open);
            if ((tid & 63u) == 0u) atomicAdd(&s_bin[b_open - s_span[0]], s);
        } else if (have) {
            atomicAdd(&s_bin[b_open - s_span[0]], s_open);
        }
        __syncthreads();
        const u64 n_bins = s_span[1] - s_span[0] + 1u;  // (at most DEP_TILE: every bin holds a position of the tile)
        for (u64 i = tid; i < n_bins; i += DEP_THREADS) {
            const u64 s = s_bin[i];
            if (s) atomicAdd(&bins[s_span[0] + i], s);
        }
    }
    // the summary: over the wave, then over the workgroup's waves
    const u64 wz = wave_sum64((u64)n_zero), wm = dep_wave_max64(vmax), ws = wave_sum64(vsum);
    if ((tid & 63u) == 0u) {
        s_red[0][tid >> 6] = wz;
        s_red[1][tid >> 6] = wm;
        s_red[2][tid >> 6] = ws;
    }
    u64 total;
    (void)vcf_scan(n_start, s_w, &total);  // (its barriers order s_red too)
    if (tid == 0u) {
        u64 z = 0, m = 0, s = 0;
#pragma unroll
        for (u32 w = 0; w < DEP_THREADS / 64u; w++) {
            z += s_red[0][w];
            m = s_red[1][w] > m ? s_red[1][w] : m;
            s += s_red[2][w];
        }
        if (z) atomicAdd(&word[1], z);
        if (m) atomicMax(&word[2], m);
        if (s) atomicAdd(&word[3], s);
        if constexpr (!BINS) bcnt[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(DEP_THREADS) void k_dep_recs(DepJob J, const u64 *__restrict__ roff, u64 n_rec, DepRec *__restrict__ rec) {
    __shared__ u64 s_w[DEP_THREADS / 64];
    const u64 p0 = ((u64)blockIdx.x * DEP_THREADS + threadIdx.x) * DEP_PPT;
    u64 bits[DEP_PPT];
#pragma unroll
    for (u32 i = 0; i < DEP_PPT; i++) bits[i] = 0;
    if (p0 < J.G) dep_load(J.depth, p0, J.G, bits);
    u32 n_start = 0;
    dep_walk(J, p0, bits, [&](u64, u64, bool start, u64, u64, u32) { n_start += start ? 1u : 0u; });
    u64 total;
    u64 r = roff[blockIdx.x] + vcf_scan(n_start, s_w, &total);  // records that start in front of the thread's positions
    dep_walk(J, p0, bits, [&](u64 p, u64 v, bool start, u64 first, u64 next, u32 c) {
        if (start) {
            if (p != first && r >= 1u && r - 1u < n_rec) rec[r - 1u].b = (u32)p;  // the run in front of it ends here
            if (r < n_rec) {
                rec[r].a = (u32)p;
                rec[r].c = c;
                rec[r].v = v;
            }
            r++;
        }
        if (p + 1u == next && r >= 1u && r - 1u < n_rec) rec[r - 1u].b = (u32)p + 1u;  // (its run's start lies at or in front of it: counted in r)
    });
}

__global__ __launch_bounds__(DEP_THREADS) void k_dep_binrecs(DepJob J, const u64 *__restrict__ bins, u64 n_rec, DepRec *__restrict__ rec) {
    const u64 r = (u64)blockIdx.x * DEP_THREADS + threadIdx.x;
    if (r >= n_rec) return;
    const u32 c = vcf_contig(J.bin_base, J.nc, r);  // (the last contig whose first record is at or in front of r: it has records)
    const u64 first = J.contig_off[c], next = J.contig_off[c + 1];
    const u64 a = first + (r - J.bin_base[c]) * J.bin, b = min(next, a + J.bin);
    DepRec R;
    R.a = (u32)a;
    R.b = (u32)b;
    R.c = c;
    R.pad = 0;
    R.v = b > a ? dep::mean_hundredths(bins[r], b - a) : 0ull;
    rec[r] = R;
}

// rec_at[r]: the line's length; bsum: the lengths per workgroup.  frac: the decimals of the records' values
__global__ __launch_bounds__(DEP_THREADS) void k_dep_reclen(const DepRec *__restrict__ rec, u64 n_rec, const u64 *__restrict__ contig_off, u32 nc,
                                                            const u64 *__restrict__ name_off, u32 frac, u64 *__restrict__ rec_at, u64 *__restrict__ bsum) {
    __shared__ u64 s_w[DEP_THREADS / 64];
    const u64 r = (u64)blockIdx.x * DEP_THREADS + threadIdx.x;
    u64 l = 0;
    if (r < n_rec) {
        const DepRec R = rec[r];
        const u32 c = min(R.c, nc - 1u);
        const u64 lo = contig_off[c];
        l = dep::line_len(name_off[c + 1] - name_off[c], R.a - lo, R.b - lo, R.v, frac);
        rec_at[r] = l;
    }
    u64 total;
    (void)vcf_scan(l, s_w, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

struct DepText {
    const u8 *names;
    const u64 *name_off, *contig_off, *rec_at;  // rec_at: n_rec + 1
    const DepRec *rec;
    u32 nc, frac;
    u64 n_rec, n_text;
};
struct DepLine {  // a record as the text pass sees it
    u64 at, end;  // its bytes in the text
    const u8 *name;
    u64 nlen, a, b, v;  // a, b: local to the contig
    u32 na, nb, nv;
};
__device__ __forceinline__ void dep_line(const DepText &X, u64 r, DepLine &L) {
    const DepRec R = X.rec[r];
    const u32 c = min(R.c, X.nc - 1u);
    const u64 lo = X.contig_off[c];
    L.at = X.rec_at[r];
    L.end = X.rec_at[r + 1u];
    L.name = X.names + X.name_off[c];
    L.nlen = X.name_off[c + 1] - X.name_off[c];
    L.a = R.a - lo;
    L.b = R.b - lo;
    L.v = R.v;
    L.na = dfmt_ndig(L.a);  // (pp_k_debug.h: in 32-bit arithmetic where the number fits)
    L.nb = dfmt_ndig(L.b);
    L.nv = dep::value_len(L.v, X.frac);
}

// the text's allocation is a multiple of 16 bytes (zeros behind the text): every lane that owns a byte stores 16
__global__ __launch_bounds__(DEP_THREADS) void k_dep_text(DepText X, u8 *__restrict__ dst) {
    __shared__ u64 s_r[2];
    const u32 tid = threadIdx.x;
    const u64 g0 = (u64)blockIdx.x * DEP_TEXT_WG, g1 = min(X.n_text, g0 + (u64)DEP_TEXT_WG);  // (g0 < n_text: the grid; n_rec >= 1)
    if (tid < 2u) s_r[tid] = vcf_record_of(X.rec_at, 0, X.n_rec - 1u, tid ? g1 - 1u : g0);  // the records of the stretch's first and last byte
    __syncthreads();
    const u64 r_lo = s_r[0], r_hi = s_r[1];
    for (u32 ti = 0; ti < DEP_TEXT_TILES; ti++) {
        const u64 t0 = g0 + (u64)ti * (DEP_THREADS * DEP_LANE) + (u64)tid * DEP_LANE;
        if (t0 >= X.n_text) break;  // (no lane waits for another below)
        u64 r = vcf_record_of(X.rec_at, r_lo, r_hi, t0);
        DepLine L;
        dep_line(X, r, L);
        u32 w0 = 0, w1 = 0, w2 = 0, w3 = 0;  // (selected by comparison, the loop not unrolled: no indexed register array)
#pragma unroll 1
        for (u32 j = 0; j < DEP_LANE; j++) {
            const u64 t = t0 + j;
            u32 b = 0;
            if (t < X.n_text) {
                if (t >= L.end && r + 1u < X.n_rec) {  // (no line is empty: at most one step per byte)
                    r++;
                    dep_line(X, r, L);
                }
                b = dep::line_byte(L.name, L.nlen, L.a, L.na, L.b, L.nb, L.v, L.nv, X.frac, t - L.at);
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

}  // namespace pp
