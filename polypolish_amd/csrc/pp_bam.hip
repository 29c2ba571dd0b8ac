// pp_bam.hip -- pp_bam_records: the alignment records of UNCOMPRESSED BAM bytes as a pp_raw_batch, decoded on the device: the front
// end of the record chain names -> filter -> gate -> prepare -> polish for a caller who holds BAM (a file's BGZF blocks are inflated
// on the device by pp_bgzf_inflate, pp_bgzf.hip, whose bytes this takes as PP_MEM_DEVICE).
//
// A BAM record is block_size (4 bytes) | the fixed part (32 bytes: refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID
// next_pos tlen) | read_name (NUL-terminated) | n_cigar_op words len << 4 | op -- the packing of pp_raw_batch.cigar -- | (l_seq+1)/2
// bytes of 4-bit SEQ | l_seq bytes QUAL | typed aux fields up to the block's end.  The block_size chain is serial by the format:
// it is walked on the host (pp_bam_walk, pp_bam_host.h) or, chunk by chunk, on the device (pp_bam_walk_device, pp_bam_walk.hip);
// everything per record runs here:
//   k_bam_scan     pass A, one lane per record: the record's range, its block_size against the lengths it declares, the name's NUL,
//                  the CIGAR ops, the refID -- each checked before anything is read through it, none with a sum that could wrap --
//                  then the fixed fields, the name's range and the walk over the aux fields for NM (last one wins, a negative one
//                  is the reference's panic) and ZP:Z:fail.  A defect is status[0] = record << 8 | kind by atomicMin: the first
//                  record in index order wins; QUIT / PANIC of Alignment::new (alignment.rs:65-78) the same way in status[1]
//   k_bam_place    the SEQ rooms ((l_seq + 31) & ~31 bytes, in units of PP_SEQ_ALIGN), the CIGAR words and the numbering of the aligned
//                  records by the workgroup scan of pp_dev.h (the DPP wave scan, a carry per workgroup): the workgroups' sums, k_colscan over them,
//                  then seq_off, cig_off and the pass byte of every aligned record at its rank
//   k_bam_expand   pass B, the hot kernel: eight lanes per record, 16 source bytes -> 32 ASCII bytes per lane and trip (four nibbles at
//                  a time through two byte permutes over the table =ACMGRSVTWYHKDBN), two 16-byte aligned stores into the room, zeros
//                  behind the read; the source at any alignment, the array's last bytes byte by byte.  The eight lanes also copy the
//                  record's CIGAR words out of their byte-unaligned place.
// No byte outside [0, n_bytes) is loaded: a wide load is issued only where the array has that many bytes left (word_at's rule,
// pp_names.hip); loads inside a record that pass A found inside the array need no second look.
#include "pp_bam_host.h"
#include "pp_dev.h"

struct pp_bam : DevOwner {
    using DevOwner::DevOwner;
    RawArrays a;
    u64 *name_off = nullptr;           // the QNAME ranges, in `bytes`
    u32 *name_len = nullptr;
    const uint8_t *bytes = nullptr;    // DEVICE: the object's copy of host bytes, or the caller's
    uint64_t n_bytes = 0;
    pp_raw_batch view{};
    std::vector<uint8_t> pass;         // HOST: one byte per aligned record, 0 = ZP:Z:fail
    StageMs<3> t;                      // pass A | the scans and the placement | pass B
};

namespace {

constexpr u32 BAM_BLOCK = 1024;  // records per workgroup of the scanning kernel
// status[0]: index of a defective record << 8 | kind, in the order they are looked for
enum : u32 { BA_RANGE = 1, BA_BLOCK = 2, BA_NAME = 3, BA_CIGAR_OP = 4, BA_REF_ID = 5, BA_AUX = 6 };
// status[1]: index of a record Alignment::new refuses << 8 | kind
enum : u32 { BE_PANIC_NM = 1, BE_MISSING_NM = 2 };

struct BamSrc {  // the bytes and the records' places (device memory)
    const u8 *bytes;
    u64 n_bytes;
    const u64 *rec_off;
    const u32 *ref_map;  // n_ref + 1 entries, or nullptr: identity
    u32 n_ref;
};
struct BamRec {  // what pass A writes per record
    uint16_t *flag;
    u32 *contig, *ref_start, *nm, *seq_len, *n_cig, *name_len;
    u64 *name_off;
    u8 *zp;  // 1: the record carries ZP:Z:fail
};

// four bytes at any alignment, inside a range that is known to lie inside the array
__device__ __forceinline__ u32 ld32(const u8 *__restrict__ p, u64 at) {
    u32 w;
    __builtin_memcpy(&w, p + at, 4);
    return w;
}
__device__ __forceinline__ u32 lower(u32 c) { return (c >= (u32)'A' && c <= (u32)'Z') ? c + 32u : c; }

__global__ __launch_bounds__(256) void k_bam_scan(u32 n_rec, BamSrc S, BamRec O, u64 *__restrict__ status) {
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rec) return;
    const u8 *__restrict__ const B = S.bytes;
    const u64 o = S.rec_off[r], N = S.n_bytes;
    u32 code = 0, flag = 0, contig = 0, ref_start = 0, nm = 0xFFFFFFFFu, l_seq = 0, n_cig = 0, name_len = 0, zp_fail = 0;
    u64 name_off = 0;
    bool negative = false;
    do {
        if (o > N || N - o < 4u) { code = BA_RANGE; break; }
        const u32 bs = ld32(B, o);
        if ((u64)bs > N - o - 4u) { code = BA_RANGE; break; }
        if (bs < 32u) { code = BA_BLOCK; break; }
        const u64 c = o + 4u;  // the fixed part: [c, c + bs) lies inside the array
        const int ref_id = (int)ld32(B, c), pos = (int)ld32(B, c + 4u);
        const u32 w8 = ld32(B, c + 8u), w12 = ld32(B, c + 12u), lrn = w8 & 0xFFu, nc = w12 & 0xFFFFu, ls = ld32(B, c + 16u);
        const u64 need = 32ull + lrn + 4ull * nc + ((u64)ls + 1u) / 2u + (u64)ls;
        if ((u64)bs < need) { code = BA_BLOCK; break; }
        if (lrn == 0 || B[c + 32u + lrn - 1u] != 0) { code = BA_NAME; break; }
        const u64 cig = c + 32u + lrn;
        for (u32 j = 0; j < nc; j++)
            if ((ld32(B, cig + 4ull * j) & 15u) > 8u) code = BA_CIGAR_OP;
        if (code) break;
        if (ref_id < -1 || (S.ref_map && ref_id >= 0 && (u32)ref_id >= S.n_ref)) { code = BA_REF_ID; break; }
        // ---- the aux fields: tag tag type value, up to the block's end ----
        u64 p = c + need;
        const u64 e = c + bs;
        while (p < e) {
            if (e - p < 3u) { code = BA_AUX; break; }
            const u32 t0 = B[p], t1 = B[p + 1u], ty = B[p + 2u];
            p += 3u;
            u32 size = 0;
            if (ty == 'A' || ty == 'c' || ty == 'C') size = 1;
            else if (ty == 's' || ty == 'S') size = 2;
            else if (ty == 'i' || ty == 'I' || ty == 'f') size = 4;
            else if (ty == 'Z' || ty == 'H') {
                const u64 start = p;
                while (p < e && B[p] != 0) p++;
                if (p == e) { code = BA_AUX; break; }  // no NUL inside the record
                if (ty == 'Z' && p - start == 4u && lower(t0) == 'z' && lower(t1) == 'p' && lower(B[start]) == 'f' &&
                    lower(B[start + 1u]) == 'a' && lower(B[start + 2u]) == 'i' && lower(B[start + 3u]) == 'l')
                    zp_fail = 1;
                p++;
                continue;
            } else if (ty == 'B') {
                if (e - p < 5u) { code = BA_AUX; break; }
                const u32 sub = B[p], cnt = (u32)B[p + 1u] | (u32)B[p + 2u] << 8 | (u32)B[p + 3u] << 16 | (u32)B[p + 4u] << 24;
                const u32 es = (sub == 'c' || sub == 'C') ? 1u : ((sub == 's' || sub == 'S') ? 2u : ((sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u));
                p += 5u;
                if (es == 0 || (u64)cnt * es > e - p) { code = BA_AUX; break; }
                p += (u64)cnt * es;
                continue;
            } else { code = BA_AUX; break; }  // a type nobody knows: the field's length is unknown, too
            if (e - p < size) { code = BA_AUX; break; }
            if (t0 == 'N' && t1 == 'M' && ty != 'A' && ty != 'f') {  // c C s S i I
                u32 v = 0;
                for (u32 j = 0; j < size; j++) v |= (u32)B[p + j] << (8u * j);
                if (ty == 'c') negative |= (v & 0x80u) != 0;
                if (ty == 's') negative |= (v & 0x8000u) != 0;
                if (ty == 'i') negative |= (v & 0x80000000u) != 0;
                nm = v;
            }
            p += size;
        }
        if (code) break;
        flag = w12 >> 16;
        contig = ref_id < 0 ? (S.ref_map ? S.ref_map[S.n_ref] : 0xFFFFFFFFu) : (S.ref_map ? S.ref_map[ref_id] : (u32)ref_id);
        ref_start = pos < 0 ? 0u : (u32)pos;  // the reference's POS 0 (alignment.rs:58-61)
        l_seq = ls;
        n_cig = nc;
        name_off = c + 32u;
        name_len = lrn - 1u;
    } while (false);
    if (code) {
        report(status, ((u64)r << 8) | code);
        flag = 4u; nm = 0xFFFFFFFFu; zp_fail = 0;  // (the scans behind this kernel read the record: as an empty, unaligned one)
    } else if (negative) report(status + 1, ((u64)r << 8) | BE_PANIC_NM);
    else if (!(flag & 4u) && nm == 0xFFFFFFFFu) report(status + 1, ((u64)r << 8) | BE_MISSING_NM);
    O.flag[r] = (uint16_t)flag;
    O.contig[r] = contig;
    O.ref_start[r] = ref_start;
    O.nm[r] = nm;
    O.seq_len[r] = l_seq;
    O.n_cig[r] = n_cig;
    O.name_off[r] = name_off;
    O.name_len[r] = name_len;
    O.zp[r] = (u8)zp_fail;
}

// PLACE == false: the workgroups' numbers of aligned records, room units (PP_SEQ_ALIGN bytes each) and CIGAR words (blk3: three
// words per workgroup).  PLACE == true: blk3 holds their exclusive scan: seq_off, cig_off, and the pass byte at the aligned rank.
template <bool PLACE>
__global__ __launch_bounds__(BAM_BLOCK) void k_bam_place(u32 n_rec, const uint16_t *__restrict__ flag, const u32 *__restrict__ seq_len,
                                                         const u32 *__restrict__ n_cig, const u8 *__restrict__ zp, u64 *__restrict__ blk3,
                                                         u64 *__restrict__ seq_off, u64 *__restrict__ cig_off, u8 *__restrict__ pass) {
    __shared__ u64 s_w[BAM_BLOCK / 64];
    const u64 r = (u64)blockIdx.x * BAM_BLOCK + threadIdx.x;
    u32 al = 0, units = 0, nc = 0;
    if (r < n_rec) {
        al = (flag[r] & 4u) ? 0u : 1u;
        units = (u32)room_units(seq_len[r]);
        nc = n_cig[r];
    }
    u64 t_al, t_units, t_cig;
    const u64 ex_al = block_scan_excl64<BAM_BLOCK>(al, s_w, &t_al);
    const u64 ex_units = block_scan_excl64<BAM_BLOCK>(units, s_w, &t_units);
    const u64 ex_cig = block_scan_excl64<BAM_BLOCK>(nc, s_w, &t_cig);
    u64 *const mine = blk3 + 3ull * blockIdx.x;
    if (!PLACE) {
        if (threadIdx.x == 0) { mine[0] = t_al; mine[1] = t_units; mine[2] = t_cig; }
        return;
    }
    if (r >= n_rec) return;
    seq_off[r] = (mine[1] + ex_units) * (u64)PP_SEQ_ALIGN;
    cig_off[r] = mine[2] + ex_cig;
    if (al) pass[mine[0] + ex_al] = zp[r] ? 0 : 1;
}

// Two source bytes (h: 16 bits) -> their four bases, high nibble first, as four ASCII bytes.  The nibbles go to a byte each; a
// byte permute picks table[n & 7] out of =ACMGRSV and out of TWYHKDBN, bit 3 of the nibble chooses between the two.
__device__ __forceinline__ u32 expand4(u32 h) {
    const u32 H = (h >> 4) & 0x0F0Fu, L = h & 0x0F0Fu;
    const u32 x = ((H | (H << 8)) & 0x00FF00FFu) | (((L | (L << 8)) & 0x00FF00FFu) << 8);
    const u32 sel = x & 0x07070707u;
    const u32 lo = __builtin_amdgcn_perm(0x56535247u /* GRSV */, 0x4D43413Du /* =ACM */, sel);
    const u32 hi = __builtin_amdgcn_perm(0x4E42444Bu /* KDBN */, 0x48595754u /* TWYH */, sel);
    const u32 m = ((x >> 3) & 0x01010101u) * 0xFFu;
    return (lo & ~m) | (hi & m);
}

// The SEQ nibbles into their rooms and the CIGAR words to their place: eight lanes per record.  Every record was found inside the
// array by k_bam_scan; a 16-byte load that would reach past the array's end is taken byte by byte.
__global__ __launch_bounds__(256) void k_bam_expand(u32 n_rec, const u8 *__restrict__ B, u64 N, const u64 *__restrict__ name_off,
                                                    const u32 *__restrict__ name_len, const u32 *__restrict__ seq_len,
                                                    const u32 *__restrict__ n_cig, const u64 *__restrict__ seq_off,
                                                    const u64 *__restrict__ cig_off, u8 *__restrict__ seq, u32 *__restrict__ cigar) {
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
    const u32 s = (u32)t & 7u;
    if ((t >> 3) >= n_rec) return;
    const u32 r = (u32)(t >> 3);
    const u64 n = seq_len[r], room = room_bytes(n);
    const u32 nc = n_cig[r];
    const u64 cig_src = name_off[r] + name_len[r] + 1u, seq_src = cig_src + 4ull * nc;
    u8 *const out = seq + seq_off[r];  // a multiple of PP_SEQ_ALIGN
    for (u64 i = 32u * s; i < room; i += 256u) {
        const u32 live = (u32)min((u64)32, n - i);  // bases of this chunk (>= 1: i < n, both i and room - n < 32 apart)
        const u64 at = seq_src + (i >> 1);
        u32 w[4];
        if (N - at >= 16u) {
            uint4 v;
            __builtin_memcpy(&v, B + at, 16);  // (any alignment: one global_load_dwordx4)
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {  // the last bytes of the array
            u64 a = 0, b = 0;
            for (u32 j = 0, nb = (live + 1u) >> 1; j < nb; j++) {
                if (j < 8u) a |= (u64)B[at + j] << (8u * j); else b |= (u64)B[at + j] << (8u * (j - 8u));
            }
            w[0] = (u32)a; w[1] = (u32)(a >> 32); w[2] = (u32)b; w[3] = (u32)(b >> 32);
        }
        u32 q[8];
#pragma unroll
        for (u32 k = 0; k < 8u; k++) {
            const u32 c4 = expand4((w[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu);
            // zeros behind the read: word k holds the bases 4k .. 4k + 3 of the chunk
            q[k] = 4u * k + 4u <= live ? c4 : (4u * k >= live ? 0u : (c4 & ((1u << (8u * (live - 4u * k))) - 1u)));
        }
        *(uint4 *)(out + i) = make_uint4(q[0], q[1], q[2], q[3]);
        *(uint4 *)(out + i + 16u) = make_uint4(q[4], q[5], q[6], q[7]);
    }
    u32 *const cd = cigar + cig_off[r];
    for (u32 j = s; j < nc; j += 8u) cd[j] = ld32(B, cig_src + 4ull * j);
}

thread_local char t_bam_msg[256] = "";

const char *defect_text(u32 code) {
    switch (code) {
    case BA_RANGE: return "does not lie inside the bytes";
    case BA_BLOCK: return "has a block_size below what its l_read_name, n_cigar_op and l_seq ask for";
    case BA_NAME: return "has an empty read_name or one without its NUL";
    case BA_CIGAR_OP: return "has a CIGAR op above 8";
    case BA_REF_ID: return "has a refID outside [-1, n_ref)";
    default: return "has an aux field that is cut, of unknown type or without its end inside the record";
    }
}

}  // namespace

extern "C" const char *pp_bam_last_error(void) { return t_bam_msg; }

// (internal hook, not part of the header: pp_bgzf.hip) the same per-thread message, for the host helpers of the BGZF block
extern "C" char *pp_bam_msg_buf_(size_t *cap) {
    *cap = sizeof t_bam_msg;
    return t_bam_msg;
}

extern "C" int pp_bam_header(const uint8_t *bytes, uint64_t n_bytes, uint32_t cap, uint32_t *n_ref, uint64_t *name_off, uint32_t *name_len,
                             uint32_t *ref_len, uint64_t *records_at) {
    t_bam_msg[0] = 0;
    return pp_bam_host::header(bytes, n_bytes, cap, n_ref, (uint64_t *)name_off, name_len, ref_len, (uint64_t *)records_at, t_bam_msg, sizeof t_bam_msg);
}

extern "C" int pp_bam_walk(const uint8_t *bytes, uint64_t n_bytes, uint64_t from, uint64_t *rec_off, uint64_t cap, uint64_t *n_rec,
                           uint64_t *end) {
    t_bam_msg[0] = 0;
    return pp_bam_host::walk(bytes, n_bytes, from, (uint64_t *)rec_off, cap, (uint64_t *)n_rec, (uint64_t *)end, t_bam_msg, sizeof t_bam_msg);
}

extern "C" void pp_bam_free(pp_bam *b) { delete b; }

extern "C" void pp_bam_raw(const pp_bam *b, pp_raw_batch *out) {
    if (out) *out = b ? b->view : pp_raw_batch{};
}

extern "C" uint64_t *pp_bam_read_id(pp_bam *b) { return b ? (uint64_t *)b->a.read_id : nullptr; }

extern "C" void pp_bam_names(const pp_bam *b, const uint8_t **bytes_dev, uint64_t *n_bytes, const uint64_t **off, const uint32_t **len) {
    if (bytes_dev) *bytes_dev = b ? b->bytes : nullptr;
    if (n_bytes) *n_bytes = b ? b->n_bytes : 0;
    if (off) *off = b ? (const uint64_t *)b->name_off : nullptr;
    if (len) *len = b ? b->name_len : nullptr;
}

extern "C" void pp_bam_pass(const pp_bam *b, const uint8_t **zp, uint64_t *n_aligned) {
    if (zp) *zp = (b && !b->pass.empty()) ? b->pass.data() : nullptr;
    if (n_aligned) *n_aligned = b ? b->pass.size() : 0;
}

extern "C" int pp_bam_kernel_ms(const pp_bam *b, float *ms) {
    return b ? b->t.total(b->ctx, "pp_bam_kernel_ms", "when the records were decoded", ms) : PP_ERR_ARG;
}

// (internal hook, not part of the header: tools/bam_timing.py) the same time by stage: pass A | scans and placement | pass B
extern "C" int pp_bam_stage_ms_(const pp_bam *b, float *ms3) { return b ? b->t.stages(ms3) : PP_ERR_ARG; }

extern "C" int pp_bam_records(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_off, uint64_t n_rec, int mem,
                              const uint32_t *ref_map, uint32_t n_ref, pp_bam **out, uint64_t *bad_record) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (bad_record) *bad_record = ~0ull;
    if (!out) return ctx->fail(PP_ERR_ARG, "pp_bam_records: null argument");
    *out = nullptr;
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "pp_bam_records: the bytes must be host memory or memory of the context's device");
    if (n_bytes && !bytes) return ctx->fail(PP_ERR_ARG, "pp_bam_records: null bytes with n_bytes > 0");
    if (mem == PP_MEM_DEVICE && !rec_off) return ctx->fail(PP_ERR_ARG, "pp_bam_records: device bytes need rec_off (the block_size chain is walked on the host: pp_bam_walk)");
    std::vector<uint64_t> walked;
    if (!rec_off) {  // host bytes: the chain from offset 0
        uint64_t n = 0, end = 0;
        char msg[256] = "";
        if (pp_bam_host::walk(bytes, n_bytes, 0, nullptr, 0, (uint64_t *)&n, (uint64_t *)&end, msg, sizeof msg)) {
            if (bad_record) *bad_record = n;
            return ctx->fail(PP_ERR_ARG, "pp_bam_records: %s", msg);
        }
        walked.resize((size_t)n);
        if (n) (void)pp_bam_host::walk(bytes, n_bytes, 0, (uint64_t *)walked.data(), n, (uint64_t *)&n, (uint64_t *)&end, msg, sizeof msg);
        rec_off = walked.data();
        n_rec = n;
    }
    if (n_rec >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "more than 2^32-1 alignments in one batch");
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u32 n = (u32)n_rec;

    std::unique_ptr<pp_bam> P(new pp_bam(ctx));
    CallScratch T;
    StageTimer timer(ctx, ctx->profiling != 0);
    int rc;
    // ---- the bytes on the device ----
    BamSrc S{};
    S.n_bytes = n_bytes;
    S.n_ref = n_ref;
    S.bytes = bytes;
    if (mem == PP_MEM_HOST) {  // the object's copy: the name ranges point into it
        u8 *own;
        if ((rc = P->alloc(own, (size_t)n_bytes))) return rc;
        if (n_bytes) PP_HIPCHK(ctx, hipMemcpyAsync(own, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, st));
        S.bytes = own;
    }
    if ((rc = on_device(ctx, T, mem, (const u64 *)rec_off, n, &S.rec_off))) return rc;
    P->bytes = S.bytes;
    P->n_bytes = n_bytes;
    if (n == 0) {  // no records: an empty batch
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        *out = P.release();
        return PP_OK;
    }
    if (ref_map && (rc = on_device(ctx, T, PP_MEM_HOST, ref_map, (size_t)n_ref + 1, &S.ref_map))) return rc;  // (host memory always)

    // ---- the per-record arrays ----
    RawArrays &A = P->a;
    if ((rc = A.alloc_records(*P, n)) || (rc = P->alloc(P->name_off, n)) || (rc = P->alloc(P->name_len, n))) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(A.read_id, 0, (size_t)n * 8, st));  // read_id: the caller's (pp_names_ids)
    const u32 nb = (n + BAM_BLOCK - 1u) / BAM_BLOCK;
    void *d_zp, *d_pass, *d_blk3, *d_blk3off, *d_status;
    if ((rc = T.get(ctx, &d_zp, (size_t)n)) || (rc = T.get(ctx, &d_pass, (size_t)n)) || (rc = T.get(ctx, &d_blk3, (size_t)nb * 24)) ||
        (rc = T.get(ctx, &d_blk3off, ((size_t)nb + 1) * 24)) || (rc = T.get(ctx, &d_status, 16)))
        return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(d_status, 0xFF, 16, st));

    // ---- pass A, and the sums ----
    BamRec O{A.flag, A.contig, A.ref_start, A.nm, A.seq_len, A.n_cig, P->name_len, P->name_off, (u8 *)d_zp};
    if ((rc = timer.begin(0))) return rc;
    hipLaunchKernelGGL(k_bam_scan, dim3((n + 255u) / 256u), dim3(256), 0, st, n, S, O, (u64 *)d_status);
    if ((rc = timer.end()) || (rc = timer.begin(1))) return rc;
    hipLaunchKernelGGL(k_bam_place<false>, dim3(nb), dim3(BAM_BLOCK), 0, st, n, (const uint16_t *)A.flag, (const u32 *)A.seq_len, (const u32 *)A.n_cig,
                       (const u8 *)d_zp, (u64 *)d_blk3, (u64 *)nullptr, (u64 *)nullptr, (u8 *)nullptr);
    hipLaunchKernelGGL(k_colscan<3>, dim3(1), dim3(1024), 0, st, (const u64 *)d_blk3, (u64)nb, (u64 *)d_blk3off);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 status[2] = {~0ull, ~0ull}, totals[3] = {0, 0, 0};
    if ((rc = fetch(ctx, d_status, status, 2)) || (rc = fetch(ctx, (const u64 *)d_blk3off + 3ull * nb, totals, 3))) return rc;
    if (status[0] != ~0ull) {
        if (bad_record) *bad_record = status[0] >> 8;
        return ctx->fail(PP_ERR_ARG, "pp_bam_records: record %llu %s", (unsigned long long)(status[0] >> 8), defect_text((u32)(status[0] & 0xFFu)));
    }
    if (status[1] != ~0ull) {
        if (bad_record) *bad_record = status[1] >> 8;
        if ((status[1] & 0xFFu) == BE_MISSING_NM) return ctx->fail(PP_ERR_QUIT, "missing NM tag (record %llu)", (unsigned long long)(status[1] >> 8));
        return ctx->fail(PP_ERR_PANIC, "record %llu has a negative NM (the reference panics on parse::<u32>)", (unsigned long long)(status[1] >> 8));
    }
    const u64 n_al = totals[0], total = totals[1] * (u64)PP_SEQ_ALIGN, n_cig_total = totals[2];
    if (total >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "more than 2^40 SEQ bytes in one batch");

    // ---- the places, pass B ----
    if ((rc = P->alloc(A.seq, (size_t)total + 64)) || (rc = P->alloc(A.cigar, (size_t)n_cig_total))) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(A.seq + total, 0, 64, st));
    if ((rc = timer.begin(1))) return rc;
    hipLaunchKernelGGL(k_bam_place<true>, dim3(nb), dim3(BAM_BLOCK), 0, st, n, (const uint16_t *)A.flag, (const u32 *)A.seq_len, (const u32 *)A.n_cig,
                       (const u8 *)d_zp, (u64 *)d_blk3off, A.seq_off, A.cig_off, (u8 *)d_pass);
    if ((rc = timer.end()) || (rc = timer.begin(2))) return rc;
    hipLaunchKernelGGL(k_bam_expand, dim3((unsigned)(((u64)n * 8u + 255u) / 256u)), dim3(256), 0, st, n, S.bytes, n_bytes, (const u64 *)P->name_off,
                       (const u32 *)P->name_len, (const u32 *)A.seq_len, (const u32 *)A.n_cig, (const u64 *)A.seq_off, (const u64 *)A.cig_off, A.seq, A.cigar);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    P->pass.resize((size_t)n_al);
    if (n_al) PP_HIPCHK(ctx, hipMemcpyAsync(P->pass.data(), d_pass, (size_t)n_al, hipMemcpyDeviceToHost, st));
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // host inputs may be released, the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    P->view = A.view(n, total, n_cig_total);
    *out = P.release();
    return PP_OK;
}
