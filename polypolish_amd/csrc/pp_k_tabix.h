// pp_k_tabix.h -- the front end of pp_tabix_index (pp_tabix.hip): a tab-separated text in device memory -- borrowed, at any alignment,
// possibly ending where its allocation ends (pp_textin.h: every load is checked against the text's size) -- to one row per LINE of
// {name id, beg, end} for the table stage of pp_k_index.h.  A meta line is a row on no reference (ref = -1), as an unplaced BAM record
// is: the table kernels pass over it, and start[] stays what it is for BAM, one offset per row with a row's end the next row's start.
//   k_tx_meta    per line: is it a data line (first byte not '#'); start[]
//   k_tx_row     one lane per data line: the tabs inside the line's first PP_TBX_LANE_BYTES bytes (four 16-byte loads at the most), and
//                where these close the columns the preset needs, the row (tx_finish).  A line whose columns are not closed inside that
//                bound -- a long name, ID or REF -- goes on the list of long lines: no lane walks a long field while its wave waits
//   k_tx_long    a workgroup per long line: 4,096 bytes a round, sixteen per lane, until the columns are closed; then tx_finish on
//                the same tab positions the lane pass would have found: the bytes do not depend on the pass
//   k_tx_name    a data line against the data line in front: a name run starts where the names differ; beg must not decrease inside
//                a run.  The scan of the run heads numbers the names
//   k_tx_rec     the rows, the bins and the run heads' lines and name lengths;  k_tx_names: the heads' names, packed, for the host
//   k_tx_span    a name's first line's start and last line's end, behind k_ix_ref (meta rows may stand between a name's lines)
//   k_tx_blk     a block offset of 2^48 or more
// The first offender in line order by atomicMin (report), as k_ix_check.
#pragma once
#include "pp_bam_index_host.h"
#include "pp_k_index.h"
#include "pp_textin.h"
#include "polypolish_hip.h"

namespace {

enum : u32 { TX_EMPTY = 1, TX_NAME = 2, TX_COLUMN = 3, TX_NUMBER = 4, TX_POS0 = 5, TX_REF = 6, TX_ENDBEG = 7, TX_END = 8, TX_ORDER = 9 };
constexpr u32 TX_LANE = PP_TBX_LANE_BYTES;
constexpr u32 TX_META = 0xFFFFFFFFu;  // TxRow::name_len of a meta line
static_assert(TX_LANE == 64, "k_tx_row holds the tabs of a line's first bytes in one 64-bit mask");

struct TxLines {  // the lines of the text: line l = [lb(l), le(l)), its '\n' not counted
    const u64 *nl_pos;  // n_nl: where the '\n' stand
    u64 n_nl, size;
    __device__ __forceinline__ u64 lb(u64 l) const { return l ? nl_pos[l - 1u] + 1u : 0ull; }
    __device__ __forceinline__ u64 le(u64 l) const { return l < n_nl ? nl_pos[l] : size; }
};

struct TxRow { u32 name_len, beg, end, kind; };  // kind != 0: the line was refused

// bit i: byte i of the sixteen is a tab
__device__ __forceinline__ u32 tab_mask16(u64 lo, u64 hi) {
    u32 out = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const u64 x = (h ? hi : lo) ^ 0x0909090909090909ull;
        const u64 z = ~(((x & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | x) & 0x8080808080808080ull;  // bit 7 of every zero byte, exact
        out |= (u32)((z * 0x0002040810204081ull) >> 56) << (8 * h);  // (byte k's bit 7 times 2^(7 (7 - k)) is bit 56 + k; no two terms meet)
    }
    return out;
}

// the number in text[a, b): 1 to 10 decimal digits
__device__ __forceinline__ bool tx_number(const u8 *__restrict__ T, u64 a, u64 b, u64 *v) {
    if (b <= a || b - a > 10u) return false;
    u64 x = 0;
    for (u64 i = a; i < b; i++) {
        const u32 d = (u32)T[i] - (u32)'0';
        if (d > 9u) return false;
        x = x * 10u + d;
    }
    *v = x;
    return true;
}

// The row of data line l = [lb, le) from its first tabs: tab[k] for k < n_tab, n_tab capped at what the preset needs (BED 3, VCF 4).
// Both passes end here.
__device__ __forceinline__ void tx_finish(const u8 *__restrict__ T, u64 lb, u64 le, const u64 tab[4], u32 n_tab, int preset, u64 l,
                                          TxRow *__restrict__ row, u64 *__restrict__ status) {
    const bool vcf = preset == PP_TBX_VCF;
    u32 kind = 0;
    u64 b = 0, e = 1;
    if (le == lb) kind = TX_EMPTY;
    else if (n_tab >= 1u && tab[0] == lb) kind = TX_NAME;
    else if (n_tab < (vcf ? 4u : 2u)) kind = TX_COLUMN;
    else if (vcf) {
        u64 p = 0;
        if (!tx_number(T, tab[0] + 1u, tab[1], &p)) kind = TX_NUMBER;
        else if (p == 0) kind = TX_POS0;
        else if (tab[3] - tab[2] == 1u) kind = TX_REF;
        else {
            b = p - 1u;
            e = b + (tab[3] - tab[2] - 1u);
        }
    } else {
        if (!tx_number(T, tab[0] + 1u, tab[1], &b) || !tx_number(T, tab[1] + 1u, n_tab >= 3u ? tab[2] : le, &e)) kind = TX_NUMBER;
        else if (e < b) kind = TX_ENDBEG;
        else if (e == b) e = b + 1u;
    }
    if (!kind && e > (u64)IX_MAX_END) kind = TX_END;
    if (kind) report(status, (l << 8) | kind);
    const u64 name = (n_tab ? tab[0] : le) - lb;
    row[l] = TxRow{(u32)min(name, (u64)0xFFFFFFFEu), kind ? 0u : (u32)b, kind ? 1u : (u32)e, kind};
}

__global__ __launch_bounds__(256) void k_tx_meta(u32 n, const u8 *__restrict__ T, TxLines Ln, u32 *__restrict__ is_data, u64 *__restrict__ start) {
    const u64 l = (u64)blockIdx.x * 256u + threadIdx.x;
    if (l >= n) return;
    const u64 lb = Ln.lb(l), le = Ln.le(l);
    is_data[l] = (le > lb && T[lb] == (u8)'#') ? 0u : 1u;
    if (l == 0) start[0] = 0;
    start[l + 1u] = lb;
    if (l + 1u == n) start[l + 2u] = Ln.size;  // (the last line's end: behind its '\n', or the text's end)
}

__global__ __launch_bounds__(256) void k_tx_row(u32 n, const u8 *__restrict__ T, TxLines Ln, int preset, const u32 *__restrict__ is_data,
                                                const u32 *__restrict__ didx, u32 *__restrict__ dline, TxRow *__restrict__ row,
                                                u32 *__restrict__ long_line, u32 *__restrict__ n_long, u64 *__restrict__ status) {
    const u64 l = (u64)blockIdx.x * 256u + threadIdx.x;
    if (l >= n) return;
    if (!is_data[l]) {
        row[l] = TxRow{TX_META, 0u, 1u, 0u};
        return;
    }
    dline[didx[l]] = (u32)l;
    const u64 lb = Ln.lb(l), le = Ln.le(l);
    const u32 m = (u32)min(le - lb, (u64)TX_LANE);
    u64 mask = 0;
#pragma unroll
    for (u32 k = 0; k < TX_LANE / 16u; k++)
        if (16u * k < m) {
            u64 lo, hi;
            load16_in(T, Ln.size, lb + 16u * k, min(16u, m - 16u * k), &lo, &hi);
            mask |= (u64)tab_mask16(lo, hi) << (16u * k);
        }
    if (m < 64u) mask &= (1ull << m) - 1ull;  // (a wide load reaches over the line's end, into the lines behind it)
    const u32 need = preset == PP_TBX_VCF ? 4u : 3u;
    u64 tab[4];
    u32 n_tab = 0;
#pragma unroll
    for (u32 k = 0; k < 4u; k++) {
        const bool has = mask != 0 && k < need;
        tab[k] = has ? lb + (u32)__builtin_ctzll(mask) : le;
        n_tab += has ? 1u : 0u;
        mask &= mask - 1ull;
    }
    if (n_tab < need && le - lb > (u64)TX_LANE) {  // not closed inside the bound: the workgroup pass
        long_line[atomicAdd(n_long, 1u)] = (u32)l;
        return;
    }
    tx_finish(T, lb, le, tab, n_tab, preset, l, row, status);
}

__global__ __launch_bounds__(256) void k_tx_long(u32 n_long, const u32 *__restrict__ long_line, const u8 *__restrict__ T, TxLines Ln, int preset,
                                                 TxRow *__restrict__ row, u64 *__restrict__ status) {
    __shared__ u64 s_tab[4];
    __shared__ u32 s_w[4];
    const u32 need = preset == PP_TBX_VCF ? 4u : 3u;
    for (u32 i = blockIdx.x; i < n_long; i += gridDim.x) {
        const u64 l = long_line[i], lb = Ln.lb(l), le = Ln.le(l);
        u32 found = 0;  // (the same in every lane)
        for (u64 base = lb; base < le && found < need; base += 256u * 16u) {
            const u64 at = base + 16u * threadIdx.x;
            u32 mask = 0;
            if (at < le) {
                const u32 nb = (u32)min((u64)16u, le - at);
                u64 lo, hi;
                load16_in(T, Ln.size, at, nb, &lo, &hi);
                mask = tab_mask16(lo, hi) & ((1u << nb) - 1u);
            }
            u32 total;
            u32 ord = found + block_scan_excl<256>((u32)__popc(mask), s_w, &total);
            while (mask && ord < need) {
                s_tab[ord++] = at + ((u32)__ffs((int)mask) - 1u);
                mask &= mask - 1u;
            }
            found = min(need, found + total);
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            u64 tab[4];
#pragma unroll
            for (u32 k = 0; k < 4u; k++) tab[k] = k < found ? s_tab[k] : le;
            tx_finish(T, lb, le, tab, found, preset, l, row, status);
        }
        __syncthreads();  // (s_tab is used again)
    }
}

__global__ __launch_bounds__(256) void k_tx_name(u32 n, const u8 *__restrict__ T, TxLines Ln, const TxRow *__restrict__ row, const u32 *__restrict__ didx,
                                                 const u32 *__restrict__ dline, u32 *__restrict__ head, u64 *__restrict__ status) {
    const u64 l = (u64)blockIdx.x * 256u + threadIdx.x;
    if (l >= n) return;
    const TxRow R = row[l];
    if (R.name_len == TX_META) {
        head[l] = 0;
        return;
    }
    const u32 d = didx[l];
    bool same = false;
    if (d > 0) {
        const u32 p = dline[d - 1u];
        const TxRow P = row[p];
        same = P.name_len == R.name_len;
        const u64 x = Ln.lb(l), y = Ln.lb(p);
        for (u32 i = 0; i < R.name_len && same;) {  // (both names lie inside their lines: no load leaves them)
            if (R.name_len - i >= 8u) {
                u64 a, b;
                __builtin_memcpy(&a, T + x + i, 8);
                __builtin_memcpy(&b, T + y + i, 8);
                same = a == b;
                i += 8u;
            } else {
                same = T[x + i] == T[y + i];
                i++;
            }
        }
        if (same && !R.kind && !P.kind && R.beg < P.beg) report(status, (l << 8) | TX_ORDER);
    }
    head[l] = same ? 0u : 1u;
}

__global__ __launch_bounds__(256) void k_tx_rec(u32 n, const TxRow *__restrict__ row, const u32 *__restrict__ head, const u32 *__restrict__ hidx,
                                                IxRec *__restrict__ rec, u32 *__restrict__ bin, u32 *__restrict__ head_line, u32 *__restrict__ head_len) {
    const u64 l = (u64)blockIdx.x * 256u + threadIdx.x;
    if (l >= n) return;
    const TxRow R = row[l];
    const bool data = R.name_len != TX_META;
    const u32 id = hidx[l] + head[l] - 1u;  // (a data line stands in or behind a run's head)
    rec[l] = data ? IxRec{(int32_t)id, (int32_t)R.beg, R.end} : IxRec{-1, 0, 1u};
    bin[l] = (data && !R.kind) ? reg2bin(R.beg, R.end) : 0u;
    if (data && head[l]) {
        head_line[id] = (u32)l;
        head_len[id] = R.name_len;
    }
}

// A name's span for the pseudo-bin.  k_ix_ref takes a reference's first and last record from the rows next to it, which holds where a
// reference's rows stand together (BAM); here meta rows may stand between a name's lines, so the span is written again behind it: from
// the run's head, and from the data line whose next data line is a head or is none.
__global__ __launch_bounds__(256) void k_tx_span(u32 n, const IxRec *__restrict__ rec, const u32 *__restrict__ head, const u32 *__restrict__ didx,
                                                 const u32 *__restrict__ dline, IxWhere W, u64 *__restrict__ ref_beg, u64 *__restrict__ ref_end) {
    const u64 l = (u64)blockIdx.x * 256u + threadIdx.x;
    if (l >= n) return;
    const int32_t ref = rec[l].ref;
    if (ref < 0) return;
    if (head[l]) ref_beg[ref] = W.at(W.start[l + 1u]);
    const u32 d = didx[l];
    if (d + 1u == didx[n] || head[dline[d + 1u]]) ref_end[ref] = W.at(W.start[l + 2u]);
}

// names[name_off[h], name_off[h + 1]) = the name of run head h: a workgroup per head
__global__ __launch_bounds__(256) void k_tx_names(u32 n_head, const u8 *__restrict__ T, TxLines Ln, const u32 *__restrict__ head_line,
                                                  const u64 *__restrict__ name_off, u8 *__restrict__ names) {
    for (u32 h = blockIdx.x; h < n_head; h += gridDim.x) {
        const u64 lb = Ln.lb(head_line[h]), o = name_off[h], len = name_off[h + 1u] - o;
        for (u64 i = threadIdx.x; i < len; i += 256u) names[o + i] = T[lb + i];
    }
}

__global__ __launch_bounds__(256) void k_tx_blk(u64 n, const u64 *__restrict__ blk_off, u64 *__restrict__ status) {
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i < n && blk_off[i] >= pp_bam_index_host::MAX_COFFSET) report(status, i);
}

}  // namespace
