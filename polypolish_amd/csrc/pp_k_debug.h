// pp_k_debug.h -- the --debug TSV, formatted on the device (write_debug_line, src/polish.rs:257-266; get_debug_line /
// get_count_str, src/pileup.rs:137-166).  Part of pp_polish_text.hip (included there, behind pp_dev.h, and nowhere else: it
// defines __global__ kernels).  Nothing here runs unless a caller asks for the TSV (pp_polish_debug_tsv): the polish
// pipeline itself is untouched.
//
// What a line is made of is on the device after a job with debug records: depth, the seven planes of counts / thresholds,
// the status, the emit code, the key records (KeyRec, atomic-append order) and the multi-byte winners (MultiEnt).
//   once per job   k_dfmt_count / k_dfmt_bsum / k_colscan<1> (pp_dev.h) / k_dfmt_apply / k_dfmt_scatter: the key records and the
//                  multi-byte winners grouped by position (count, exclusive scan, scatter): rec_end[p] = one past the
//                  position's last entry of rec[], which holds record ids (< n_keys: a key, else a multi-byte winner)
//   per chunk      k_dfmt_len: the length of every line of [p0, p0 + N), one thread a position, and the workgroups' sums;
//                  k_colscan<1>: their exclusive scan (u64 line offsets); k_dfmt_write: every workgroup stages its lines
//                  in LDS, DFMT_WIN bytes at a time, and stores them with 16-byte stores where the destination allows.
//                  Only the lines that end within the room are written; the workgroup that holds the last of them reports
//                  how many positions and bytes that is.
// A position's items ("Ax12", "ACx3", "-x5", ...) are sorted as whole strings, bytewise: an item's place is the summed
// length of the items before it, found by comparing it with every other item (no list is stored anywhere).  A position
// with more than DFMT_HEAVY items has its items placed by the whole workgroup, one item per lane and round.
#pragma once

namespace pp {

constexpr u32 DFMT_THREADS = 256;  // positions per workgroup of the size and write passes (one per thread)
constexpr u32 DFMT_WIN = 16384;    // bytes of LDS a workgroup stages its lines in, one window after the other
constexpr u32 DFMT_HEAVY = 12;     // positions with more items than this: their items are placed by the whole workgroup
constexpr u32 DFMT_SCAN_PER = 16;  // elements per thread of the index's scan (4096 per workgroup)

struct DfmtJob {
    const double *depth;
    const u32 *counts;  // seven planes of G: A C G T other valid_thr invalid_thr
    const u8 *status, *code, *bases, *seq;
    const u64 *contig_off;
    u32 nc;
    u32 n_keys;
    const u8 *names;
    const u64 *name_off;  // nc + 1
    const u32 *emit;      // (lo, hi) per contig: the positions this context emits; nullptr = all
    const KeyRec *keys;
    const MultiEnt *multi;
    const u32 *rec_end;   // per position
    const u32 *rec;
    u64 G;
};

// ---- the key records and multi-byte winners, grouped by position (once per job) ----------------------------------------
__global__ __launch_bounds__(256) void k_dfmt_count(const KeyRec *__restrict__ keys, u32 nk, const MultiEnt *__restrict__ multi,
                                                    u32 nm, u64 G, u32 *__restrict__ cnt) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (u64)nk + nm) return;
    const u32 pos = i < nk ? keys[i].pos : multi[i - nk].pos;
    if (pos < G) atomicAdd(&cnt[pos], 1u);
}

__global__ __launch_bounds__(256) void k_dfmt_scatter(const KeyRec *__restrict__ keys, u32 nk, const MultiEnt *__restrict__ multi,
                                                      u32 nm, u64 G, u32 *__restrict__ next, u32 *__restrict__ rec) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (u64)nk + nm) return;
    const u32 pos = i < nk ? keys[i].pos : multi[i - nk].pos;
    if (pos < G) rec[atomicAdd(&next[pos], 1u)] = (u32)i;
}

// exclusive scan of n u32 IN PLACE: block sums (DFMT_SCAN_PER x 256 elements a workgroup), one workgroup scans them (k_colscan<1>),
// every workgroup then scans its own elements on top of its base.  (Not pp_dev.h's scan_u32: that one writes a second array, 4
// more bytes per assembly position of a --debug job.)
__global__ __launch_bounds__(256) void k_dfmt_bsum(const u32 *__restrict__ a, u64 n, u64 *__restrict__ bsum) {
    __shared__ u64 s_w[4];
    const u64 base = ((u64)blockIdx.x * 256u + threadIdx.x) * DFMT_SCAN_PER;
    u64 v = 0;
    for (u32 j = 0; j < DFMT_SCAN_PER; j++)
        if (base + j < n) v += a[base + j];
    v = wave_sum64(v);
    if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(256) void k_dfmt_apply(u32 *__restrict__ a, u64 n, const u64 *__restrict__ boff) {
    __shared__ u32 s_w[4];
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 base = ((u64)blockIdx.x * 256u + threadIdx.x) * DFMT_SCAN_PER;
    u32 sum = 0;
    for (u32 j = 0; j < DFMT_SCAN_PER; j++)
        if (base + j < n) sum += a[base + j];
    u32 inc = sum;
    for (int o = 1; o < 64; o <<= 1) {
        const u32 v = __shfl_up(inc, o, 64);
        if ((int)lane >= o) inc += v;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u32 run = (u32)boff[blockIdx.x] + (inc - sum);  // (the total is below 2^32: the host checks)
    for (u32 i = 0; i < wave; i++) run += s_w[i];
    for (u32 j = 0; j < DFMT_SCAN_PER; j++)
        if (base + j < n) {
            const u32 v = a[base + j];
            a[base + j] = run;
            run += v;
        }
}

// ---- one line ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 dfmt_ndig(u64 v) {
    u32 n = 1;
    if (v <= 0xFFFFFFFFull) {
        for (u32 x = (u32)v; x >= 10u; x /= 10u) n++;
        return n;
    }
    for (; v >= 10u; v /= 10u) n++;
    return n;
}

// format!("{:.1}", x) of a depth (x >= 0): 10 x rounded to an integer from its exact binary value, ties to even, as glibc's
// printf and Rust's formatting do -- x = m 2^e exactly, so 10 x = (10 m) 2^e and the rounding is one shift and a comparison
__device__ __forceinline__ u64 dfmt_tenths(double x) {
    const u64 b = (u64)__double_as_longlong(x);
    int E = (int)((b >> 52) & 0x7FFu);
    u64 m = b & ((1ull << 52) - 1);
    if (E == 0) {
        if (m == 0) return 0;
        E = 1;  // subnormal
    } else {
        m |= 1ull << 52;
    }
    const int e = E - 1075;
    const u64 N = m * 10u;  // < 2^57
    if (e >= 0) return e < 7 ? N << e : ~0ull;  // (2^52 and more: never a depth)
    const int s = -e;
    if (s >= 64) return 0;  // 10 x < 2^57 / 2^64: below one half
    const u64 q = N >> s, r = N & ((1ull << s) - 1), half = 1ull << (s - 1);
    return q + ((r > half || (r == half && (q & 1u))) ? 1u : 0u);
}

__device__ __forceinline__ u32 dfmt_status_len(u32 st) {
    // kept changed low_depth none multiple too_close
    return st == 1u ? 7u : st == 2u ? 9u : st == 3u ? 4u : st == 4u ? 8u : st == 5u ? 9u : 4u;
}

struct DfmtItem {
    u64 off;     // the key's bytes in the seq array (single == 0)
    u32 klen, count, dl;
    u32 single;  // the key is this one byte (A C G T, or '-' for the deletion key), else 0
};

// item slot q of a position: 0..3 = A C G T (an item if its count is not zero), 4 + j = its record r0 + j (an item if it is a key)
__device__ __forceinline__ bool dfmt_item(const DfmtJob &J, const u32 cnt[4], u32 r0, u32 q, DfmtItem &it) {
    if (q < 4u) {
        const u32 cq = q == 0u ? cnt[0] : q == 1u ? cnt[1] : q == 2u ? cnt[2] : cnt[3];  // (no indexed access: the array stays in registers)
        if (!cq) return false;
        it.single = (0x54474341u >> (8u * q)) & 0xFFu;  // "ACGT"
        it.off = 0;
        it.klen = 1;
        it.count = cq;
    } else {
        const u32 id = J.rec[r0 + q - 4u];
        if (id >= J.n_keys) return false;  // the position's multi-byte winner
        const KeyRec k = J.keys[id];
        it.single = k.len ? 0u : (u32)'-';
        it.off = k.off;
        it.klen = k.len ? k.len : 1u;
        it.count = k.count;
    }
    it.dl = dfmt_ndig(it.count);
    return true;
}
__device__ __forceinline__ u32 dfmt_item_len(const DfmtItem &it) { return it.klen + 1u + it.dl; }
__device__ __forceinline__ u32 dfmt_item_byte(const DfmtJob &J, const DfmtItem &it, u32 j) {
    if (j < it.klen) return it.single ? it.single : (u32)J.seq[it.off + j];
    if (j == it.klen) return (u32)'x';
    u32 v = it.count;
    for (u32 d = it.klen + it.dl - j; d > 0; d--) v /= 10u;  // digit j - klen - 1, the most significant first
    return (u32)'0' + v % 10u;
}
// is item a (slot qa) before item b (slot qb) in bytewise string order?  (Two items are never the same string; the slot
// decides if they were.)
__device__ __forceinline__ bool dfmt_less(const DfmtJob &J, const DfmtItem &a, u32 qa, const DfmtItem &b, u32 qb) {
    const u32 la = dfmt_item_len(a), lb = dfmt_item_len(b), n = min(la, lb);
    for (u32 j = 0; j < n; j++) {
        const u32 x = dfmt_item_byte(J, a, j), y = dfmt_item_byte(J, b, j);
        if (x != y) return x < y;
    }
    return la != lb ? la < lb : qa < qb;
}

struct DfmtLine {
    u64 rel;     // position in its contig
    u64 tenths;  // 10 x depth, rounded
    u64 nb_off;  // new_base: the multi-byte winner's bytes in the seq array (nb_len > 1 or from a winner), else nb_byte
    u32 c, len, items_len, n_items, r0, r1, inv, val, nb_len, nb_byte, st;
    u32 cnt[4];
    u8 orig, from_seq;
};

// everything about the line of position p but its bytes; len = 0: not a position this context emits
__device__ __forceinline__ void dfmt_line(const DfmtJob &J, u64 p, DfmtLine &L) {
    u32 lo = 0, hi = J.nc;  // contig_off[lo] <= p < contig_off[hi]
    while (hi - lo > 1u) {
        const u32 mid = (lo + hi) >> 1;
        if (J.contig_off[mid] <= p) lo = mid; else hi = mid;
    }
    L.c = lo;
    L.rel = p - J.contig_off[lo];
    L.len = 0;
    if (J.emit && (L.rel < J.emit[2 * lo] || L.rel >= J.emit[2 * lo + 1])) return;
    L.orig = J.bases[p];
    L.st = J.status[p];
    if (L.st > 5u) L.st = 0;
    const u32 code = J.code[p];
    L.tenths = dfmt_tenths(J.depth[p]);
#pragma unroll
    for (u32 q = 0; q < 4u; q++) L.cnt[q] = J.counts[(u64)q * J.G + p];
    L.val = J.counts[5ull * J.G + p];
    L.inv = J.counts[6ull * J.G + p];
    L.r0 = p ? J.rec_end[p - 1] : 0u;
    L.r1 = J.rec_end[p];
    u32 n = 0, bytes = 0, winner = ~0u, valid_key = ~0u;
    for (u32 q = 0; q < 4u + (L.r1 - L.r0); q++) {
        DfmtItem it;
        if (dfmt_item(J, L.cnt, L.r0, q, it)) {
            n++;
            bytes += dfmt_item_len(it);
            if (q >= 4u && it.klen >= 2u && it.count >= L.val) valid_key = J.rec[L.r0 + q - 4u];  // a valid key of two bytes or more
        } else if (q >= 4u) {
            winner = J.rec[L.r0 + q - 4u] - J.n_keys;
        }
    }
    L.n_items = n;
    L.items_len = bytes + (n ? n - 1u : 0u);
    // new_base (polish.rs:257-266 as the host writer had it): code 0 = "-" where the status is "changed", else the assembly's
    // byte; 1..127 = that byte; 128 and up = the multi-byte winner's raw bytes
    L.from_seq = 0;
    L.nb_len = 1;
    if (code == 0u) L.nb_byte = L.st == (u32)PP_ST_CHANGED ? (u32)'-' : (u32)L.orig;
    else if (code < 0x80u) L.nb_byte = code;
    else if (winner != ~0u) {
        const MultiEnt w = J.multi[winner];
        L.from_seq = 1;
        L.nb_off = w.off;
        L.nb_len = w.len;
    } else L.nb_len = 0;
    // A winner of two bytes or more that leaves at most one once its '-' are dropped (polish.rs:188: "C-", "--") has a one-byte
    // code and no entry in the winners' list; new_base is the winner as the reads have it.  Where the status is "changed" exactly
    // one item is valid, the winner: it is that key if a key of two bytes or more is valid.
    if (code < 0x80u && L.st == (u32)PP_ST_CHANGED && valid_key != ~0u) {
        const KeyRec k = J.keys[valid_key];
        L.from_seq = 1;
        L.nb_off = k.off;
        L.nb_len = k.len;
    }
    L.len = (u32)(J.name_off[lo + 1] - J.name_off[lo]) + dfmt_ndig(L.rel) + 1u + (dfmt_ndig(L.tenths / 10u) + 2u) + dfmt_ndig(L.inv) +
            dfmt_ndig(L.val) + L.items_len + dfmt_status_len(L.st) + L.nb_len + 9u;
}

// the part of the output a workgroup has in LDS: bytes [ws, ws + wlen) of the chunk, at s + shift (shift: the destination's
// alignment, so that LDS and destination agree on which bytes share a 16-byte word)
struct DfmtWin {
    u8 *s;
    u64 ws;
    u32 wlen, shift;
    __device__ __forceinline__ void put(u64 x, u32 b) const {
        const u64 d = x - ws;
        if (d < wlen) s[d + shift] = (u8)b;
    }
    __device__ __forceinline__ bool hits(u64 x0, u64 x1) const { return x0 < ws + wlen && x1 > ws; }
};
__device__ __forceinline__ u64 dfmt_put_dec(const DfmtWin &W, u64 x, u64 v) {
    const u32 nd = dfmt_ndig(v);
    if (v <= 0xFFFFFFFFull) {
        u32 w = (u32)v;
        for (u32 i = nd; i-- > 0; w /= 10u) W.put(x + i, (u32)'0' + w % 10u);
    } else {
        for (u32 i = nd; i-- > 0; v /= 10u) W.put(x + i, (u32)'0' + (u32)(v % 10u));
    }
    return x + nd;
}

// the items of a position, each at its place in the field that starts at x (items_len bytes), comma behind it unless it is
// the last; slots q0, q0 + dq, ... of this thread
__device__ __forceinline__ void dfmt_place_items(const DfmtJob &J, const u32 cnt[4], u32 r0, u32 r1, u64 x, u32 items_len,
                                                 const DfmtWin &W, u32 q0, u32 dq) {
    const u32 ns = 4u + (r1 - r0);
    for (u32 q = q0; q < ns; q += dq) {
        DfmtItem a;
        if (!dfmt_item(J, cnt, r0, q, a)) continue;
        u32 off = 0;
        for (u32 q2 = 0; q2 < ns; q2++) {
            DfmtItem b;
            if (q2 == q || !dfmt_item(J, cnt, r0, q2, b)) continue;
            if (dfmt_less(J, b, q2, a, q)) off += dfmt_item_len(b) + 1u;
        }
        const u32 la = dfmt_item_len(a);
        if (!W.hits(x + off, x + off + la + 1u)) continue;
        for (u32 j = 0; j < la; j++) W.put(x + off + j, dfmt_item_byte(J, a, j));
        if (off + la < items_len) W.put(x + off + la, (u32)',');
    }
}

// the line's bytes that fall into the window; its items too unless `heavy` (the workgroup places those)
__device__ __forceinline__ void dfmt_write_line(const DfmtJob &J, const DfmtLine &L, u64 x, const DfmtWin &W, bool heavy) {
    const u64 n0 = J.name_off[L.c], n1 = J.name_off[L.c + 1];
    for (u64 j = n0; j < n1; j++) W.put(x++, J.names[j]);
    W.put(x++, '\t');
    x = dfmt_put_dec(W, x, L.rel);
    W.put(x++, '\t');
    W.put(x++, L.orig);
    W.put(x++, '\t');
    x = dfmt_put_dec(W, x, L.tenths / 10u);
    W.put(x++, '.');
    W.put(x++, (u32)'0' + (u32)(L.tenths % 10u));
    W.put(x++, '\t');
    x = dfmt_put_dec(W, x, L.inv);
    W.put(x++, '\t');
    x = dfmt_put_dec(W, x, L.val);
    W.put(x++, '\t');
    if (!heavy && L.n_items) dfmt_place_items(J, L.cnt, L.r0, L.r1, x, L.items_len, W, 0u, 1u);
    x += L.items_len;
    W.put(x++, '\t');
    // kept changed low_depth none multiple too_close
    const char *s = L.st == 1u ? "changed" : L.st == 2u ? "low_depth" : L.st == 3u ? "none" : L.st == 4u ? "multiple" : L.st == 5u ? "too_close" : "kept";
    for (; *s; s++) W.put(x++, (u32)(u8)*s);
    W.put(x++, '\t');
    if (L.from_seq) {
        for (u32 j = 0; j < L.nb_len; j++) W.put(x++, J.seq[L.nb_off + j]);
    } else if (L.nb_len) {
        W.put(x++, L.nb_byte);
    }
    W.put(x, '\n');
}

// ---- the size pass -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DFMT_THREADS) void k_dfmt_len(DfmtJob J, u64 p0, u32 N, u32 *__restrict__ len, u64 *__restrict__ bsum) {
    __shared__ u64 s_w[DFMT_THREADS / 64];
    const u32 i = blockIdx.x * DFMT_THREADS + threadIdx.x;
    u32 l = 0;
    if (i < N) {
        DfmtLine L;
        dfmt_line(J, p0 + i, L);
        l = L.len;
        len[i] = l;
    }
    const u64 s = wave_sum64(l);
    if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0;
        for (u32 w = 0; w < DFMT_THREADS / 64; w++) t += s_w[w];
        bsum[blockIdx.x] = t;
    }
}

// ---- the write pass ----------------------------------------------------------------------------------------------------
// boff: the workgroups' first bytes (k_colscan<1> over k_dfmt_len's sums); room: bytes of dst that may be written.  res[0] =
// positions whose lines fit (from p0 on), res[1] = their bytes -- written by the thread of the last line that fits (the host
// zeroes res: no line fits, no writer).
__global__ __launch_bounds__(DFMT_THREADS) void k_dfmt_write(DfmtJob J, u64 p0, u32 N, const u32 *__restrict__ len,
                                                             const u64 *__restrict__ boff, u64 room, u8 *__restrict__ dst,
                                                             u64 *__restrict__ res) {
    __shared__ __attribute__((aligned(16))) u8 s_buf[DFMT_WIN + 16];
    __shared__ u32 s_w[DFMT_THREADS / 64];
    __shared__ u64 s_end;
    __shared__ u32 s_nh;
    __shared__ u32 s_hv_t[DFMT_THREADS], s_hv_len[DFMT_THREADS];
    __shared__ u64 s_hv_x[DFMT_THREADS];
    const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const u32 i = blockIdx.x * DFMT_THREADS + t;
    DfmtLine L;
    L.len = 0;
    if (i < N) dfmt_line(J, p0 + i, L);
    const u32 l = L.len;
    u32 inc = l;
    for (int o = 1; o < 64; o <<= 1) {
        const u32 v = __shfl_up(inc, o, 64);
        if ((int)lane >= o) inc += v;
    }
    if (lane == 63) s_w[wave] = inc;
    const u64 blk_start = boff[blockIdx.x];
    if (t == 0) {
        s_end = blk_start;
        s_nh = 0;
    }
    __syncthreads();
    u64 start = blk_start + (inc - l);
    for (u32 w = 0; w < wave; w++) start += s_w[w];
    const u64 end = start + l;
    const bool fits = i < N && end <= room;
    if (fits) {
        const bool last = i + 1u >= N || end + len[i + 1] > room;
        if (last) {
            res[0] = (u64)i + 1u;
            res[1] = end;
        }
        if (l) atomicMax((unsigned long long *)&s_end, (unsigned long long)end);
        if (l && L.n_items > DFMT_HEAVY) {  // its items: the workgroup's (below)
            const u32 k = atomicAdd(&s_nh, 1u);
            const u64 x = start + (J.name_off[L.c + 1] - J.name_off[L.c]) + dfmt_ndig(L.rel) + 1u + (dfmt_ndig(L.tenths / 10u) + 2u) +
                          dfmt_ndig(L.inv) + dfmt_ndig(L.val) + 6u;
            s_hv_t[k] = t;
            s_hv_x[k] = x;
            s_hv_len[k] = L.items_len;
        }
    }
    __syncthreads();
    const u64 blk_end = s_end;
    const u32 nh = s_nh;
    for (u64 ws = blk_start; ws < blk_end; ws += DFMT_WIN) {
        const u32 wlen = (u32)min((u64)DFMT_WIN, blk_end - ws);
        u8 *const a = dst + ws;
        const u32 shift = (u32)((uintptr_t)a & 15u);
        u8 *const abase = a - shift;
        const DfmtWin W{s_buf, ws, wlen, shift};
        if (fits && l && W.hits(start, end)) dfmt_write_line(J, L, start, W, L.n_items > DFMT_HEAVY);
        for (u32 h = 0; h < nh; h++) {
            const u64 x = s_hv_x[h];
            if (!W.hits(x, x + s_hv_len[h])) continue;
            const u64 p = p0 + (u64)blockIdx.x * DFMT_THREADS + s_hv_t[h];
            u32 cnt[4];
#pragma unroll
            for (u32 q = 0; q < 4u; q++) cnt[q] = J.counts[(u64)q * J.G + p];
            const u32 r0 = p ? J.rec_end[p - 1] : 0u, r1 = J.rec_end[p];
            dfmt_place_items(J, cnt, r0, r1, x, s_hv_len[h], W, t, DFMT_THREADS);
        }
        __syncthreads();
        // out: the 16-byte words of the destination that the window touches; whole words with one store each
        const u32 nw = (shift + wlen + 15u) / 16u;
        for (u32 j = t; j < nw; j += DFMT_THREADS) {
            const u32 b0 = 16u * j;
            if (b0 >= shift && b0 + 16u <= shift + wlen) {
                *(uint4 *)(abase + b0) = *(const uint4 *)(s_buf + b0);
            } else {
                for (u32 b = b0; b < b0 + 16u; b++)
                    if (b >= shift && b < shift + wlen) abase[b] = s_buf[b];
            }
        }
        __syncthreads();
    }
}

}  // namespace pp
