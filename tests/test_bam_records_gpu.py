"""pp_bam_records (pp_bam.hip) against tests/bam_model.py's decode, byte for byte -- the rooms and their zeros, the name ranges and the
pass bytes included -- with the bytes in host memory and in device memory; there the allocation is exactly n_bytes long and the last
record ends at its last byte.  The shape of the generated inputs is pinned on the CPU (tests/test_bam_model_cpu.py).  The malformed
records are refused from the decode's range checks: nothing here depends on a fault.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import bam_model as bm

pytestmark = pytest.mark.gpu
REF_MAP = [0, 1, 2, 9]      # three references and the "*"


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def on_device(b, off):
    """(data, rec_off, keep) for mem = MEM_DEVICE: the bytes in an allocation of exactly their length"""
    import torch
    dev = torch.device("cuda:0")
    tb = torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to(dev) if len(b) else torch.zeros(1, dtype=torch.uint8, device=dev)
    to = torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64).copy()).to(dev) if len(off) else torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    return (tb.data_ptr(), len(b)), (to.data_ptr(), len(off)), (tb, to)


def decoded(pp, ctx, b, off, ref_map, mem):
    if mem == pp.MEM_HOST:
        return pp.BamRecords(ctx, b, off, ref_map, mem), None
    data, rec_off, keep = on_device(b, off)
    return pp.BamRecords(ctx, data, rec_off, ref_map, mem), keep


def check(pp, ctx, b, off, ref_map=None):
    want = bm.decode(b, off, ref_map)
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        rec, keep = decoded(pp, ctx, b, off, ref_map, mem)
        try:
            got = rec.host()
            bm.same(got, want)
            assert rec.zp.dtype == np.uint8 and np.array_equal(rec.zp, want["zp"]), mem
            assert (rec.n_rec, rec.seq_bytes, rec.n_cig_total) == (len(off), len(want["seq"]), len(want["cigar"]))
            raw = rec.raw()
            assert raw["read_id"] == rec.read_id_ptr and (raw["n_rec"], raw["seq_bytes"]) == (len(off), len(want["seq"]))
        finally:
            rec.close()
    return want


def refused(pp, ctx, b, off, code, bad, ref_map=None, text=None):
    try:
        bm.decode(b, off, ref_map)
    except bm.BamError as m:
        assert (m.code, m.bad_record) == (code, bad), "the model refuses the same record"
    else:
        raise AssertionError("the model takes these records")
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        with pytest.raises(pp.PolypolishError) as e:
            decoded(pp, ctx, b, off, ref_map, mem)
        assert (e.value.code, e.value.bad_record) == (code, bad), (mem, e.value)
        if text:
            assert text in e.value.msg


def closing_pad(n, f):
    return lambda i: f(i) if i + 1 < n else 0      # nothing behind the last record: it ends at the array's last byte


@pytest.mark.parametrize("lead", (0, 1))
def test_seams_of_the_expansion(pp, ctx, lead):
    recs = bm.seam_records()
    b, off = bm.lay_out(recs, lead, closing_pad(len(recs), lambda i: (3 * i) % 7))
    check(pp, ctx, b, off)
    back = off[::-1].copy()
    back[5] = back[6]                               # reverse order, one record twice
    want = check(pp, ctx, b, back)
    assert want["name_off"][5] == want["name_off"][6]


def test_aux_walk(pp, ctx):
    cases = bm.aux_records()
    b, off = bm.lay_out([r for _, r, _, _ in cases], 0, closing_pad(len(cases), lambda i: i % 3))
    want = check(pp, ctx, b, off)
    assert want["nm"].tolist() == [nm for _, _, nm, _ in cases]
    assert want["zp"].tolist() == [ok for _, _, _, ok in cases if ok is not None]
    assert [w for w, _, _, ok in cases if ok == 0] == ["ZP:Z:fail", "zp:Z:FAIL", "ZP:Z:fail in front of NM"]


def test_values_and_ref_maps(pp, ctx):
    recs = bm.mixed_records(300, seed=4)
    b, off = bm.lay_out(recs, 3)
    ident = check(pp, ctx, b, off)
    assert (ident["contig"] == bm.NO_CONTIG).any() and set(ident["contig"].tolist()) >= {0, 1, 2}
    perm = check(pp, ctx, b, off, ref_map=[2, 0, 1, 77])
    assert set(perm["contig"].tolist()) == {0, 1, 2, 77} and not np.array_equal(perm["contig"], ident["contig"])
    assert (ident["ref_start"] == 0).sum() > 20, "pos -1 is ref_start 0"


def test_quit_and_panic(pp, ctx):
    good = bm.record(b"g", 0, 0, 0, [(4 << 4)], "ACGT", bm.aux("NM", "C", 0))
    no_nm = bm.record(b"n", 16, 0, 0, [(4 << 4)], "ACGT", bm.aux("AS", "C", 3))
    umax = bm.record(b"u", 0, 0, 0, [(4 << 4)], "ACGT", bm.aux("NM", "I", 0xFFFFFFFF))
    for ty, v in (("c", -1), ("s", -300), ("i", -70000)):
        neg = bm.record(b"m", 4, -1, -1, [], "", bm.aux("NM", ty, v) + bm.aux("NM", "C", 3))
        b, off = bm.lay_out([good, good, neg, no_nm], 1)
        refused(pp, ctx, b, off, pp.ERR_PANIC, 2)
    b, off = bm.lay_out([good, no_nm, good, neg])
    refused(pp, ctx, b, off, pp.ERR_QUIT, 1, text="missing NM tag")
    b, off = bm.lay_out([good] * 5 + [umax])
    refused(pp, ctx, b, off, pp.ERR_QUIT, 5, text="missing NM tag")
    refused(pp, ctx, b, off[::-1].copy(), pp.ERR_QUIT, 0)


def test_every_defect_is_refused_from_the_range_checks(pp, ctx):
    good = [r for _, r, _, _ in bm.aux_records()[:6]]
    no_nm = bm.record(b"n", 0, 0, 0, [(4 << 4)], "ACGT", b"")
    for kind, rec in bm.defect_records():
        b, off = bm.lay_out(good[:3] + [rec] + good[3:], 1, lambda i: i % 4)            # mid-array
        refused(pp, ctx, b, off, pp.ERR_ARG, 3, ref_map=REF_MAP)
        b, off = bm.lay_out(good + [rec], 0, closing_pad(7, lambda i: 1))             # the last record, the array ends with it
        assert int(off[-1]) + len(rec) == len(b)
        refused(pp, ctx, b, off, pp.ERR_ARG, 6, ref_map=REF_MAP)
    # ... with an earlier record that Alignment::new refuses: the defect is reported
    b, off = bm.lay_out([good[0], no_nm, good[1], bm.defect_records()[3][1], good[2]])
    refused(pp, ctx, b, off, pp.ERR_ARG, 3, ref_map=REF_MAP)
    # offsets and records outside the array
    b, off = bm.lay_out(good)
    for o in (len(b) + 1, len(b) - 3, 1 << 63, (1 << 64) - 2):
        bad = off.copy()
        bad[4] = o
        refused(pp, ctx, b, bad, pp.ERR_ARG, 4)
    refused(pp, ctx, b[:-1], off, pp.ERR_ARG, 5)                                      # the last record one byte short
    # a refID behind the references needs a map to be one
    b, off = bm.lay_out(good + [bm.defect_records()[7][1]])
    assert check(pp, ctx, b, off)["contig"][-1] == 3


def test_a_refused_call_returns_no_object(pp, ctx):
    b, off = bm.lay_out([bm.defect_records()[0][1]])
    data = np.frombuffer(b, np.uint8)
    out, bad = C.c_void_p(12345), C.c_uint64(0)
    rc = pp.lib().pp_bam_records(ctx._h, data.ctypes.data, len(data), off.ctypes.data, 1, pp.MEM_HOST, None, 0, C.byref(out), C.byref(bad))
    assert rc == pp.ERR_ARG and out.value is None and bad.value == 0


def test_5000_mixed_records(pp, ctx):
    recs = bm.mixed_records()
    b, off = bm.lay_out(recs, 0, closing_pad(len(recs), lambda i: i % 2))
    want = check(pp, ctx, b, off, ref_map=[1, 2, 0, 50])
    assert len(off) > 4 * bm.BAM_BLOCK and len(want["seq"]) > (1 << 19)


def test_edge_contracts(pp, ctx):
    recs = bm.seam_records()[40:60]
    b, off = bm.lay_out(recs)
    empty = check(pp, ctx, b, off[:0])
    assert len(empty["flag"]) == 0 and len(empty["seq"]) == 0
    check(pp, ctx, b"", off[:0])
    walked = pp.BamRecords(ctx, b)                        # rec_off = None on the host: the library walks the chain
    try:
        bm.same(walked.host(), bm.decode(b, off))
    finally:
        walked.close()
    with pytest.raises(pp.PolypolishError) as e:          # a chain that breaks: the records in front of the break
        pp.BamRecords(ctx, b[:-1])
    assert (e.value.code, e.value.bad_record) == (pp.ERR_ARG, len(off) - 1)
    data, _, keep = on_device(b, off)
    with pytest.raises(pp.PolypolishError) as e:
        pp.BamRecords(ctx, data, None, None, pp.MEM_DEVICE)
    assert e.value.code == pp.ERR_ARG and "rec_off" in e.value.msg
    with pytest.raises(pp.PolypolishError) as e:
        pp.BamRecords(ctx, b, off, None, pp.MEM_PEER)
    assert e.value.code == pp.ERR_ARG


def test_kernel_ms_needs_profiling(pp):
    c = pp.Context(0)
    try:
        b, off = bm.lay_out(bm.seam_records())
        rec = pp.BamRecords(c, b, off)
        with pytest.raises(pp.PolypolishError) as e:
            rec.kernel_ms()
        assert e.value.code == pp.ERR_ARG
        rec.close()
        c.set_profiling(True)
        rec = pp.BamRecords(c, b, off)
        assert rec.kernel_ms() > 0
        rec.close()
    finally:
        c.close()


def test_a_second_decode_on_the_context_keeps_nothing(pp, ctx):
    small, large = bm.seam_records()[:30], bm.mixed_records(2500, seed=8)
    bs, os_ = bm.lay_out(small, 1)
    want = check(pp, ctx, bs, os_)
    bad, ob = bm.lay_out(small[:10] + [bm.defect_records()[8][1]] + small[10:])
    refused(pp, ctx, bad, ob, pp.ERR_ARG, 10)
    assert np.array_equal(check(pp, ctx, bs, os_)["seq"], want["seq"])
    bl, ol = bm.lay_out(large)
    check(pp, ctx, bl, ol)
    assert np.array_equal(check(pp, ctx, bs, os_)["seq"], want["seq"])


# ---- the binding's shared helpers: one handle base, one download, one batch read-back ------------------------------------------------
NO_PROFILING = {     # the library's text when kernel_ms() is asked of an object made without profiling
    "BamOffsets": "pp_bam_offs_kernel_ms: the context had no profiling on when the chain was walked (pp_ctx_set_profiling)",
    "BamRecords": "pp_bam_kernel_ms: the context had no profiling on when the records were decoded (pp_ctx_set_profiling)",
    "Names": "pp_names_kernel_ms: the context had no profiling on at the table's last pp_names_ids (pp_ctx_set_profiling)",
    "GatedBatch": "pp_gated_kernel_ms: the context had no profiling on when the batch was gated (pp_ctx_set_profiling)",
    "PreparedBatch": "pp_prepared_kernel_ms: the context had no profiling on when the batch was prepared (pp_ctx_set_profiling)",
    "SamRecords": "pp_sam_kernel_ms: the context had no profiling on when the text was decoded (pp_ctx_set_profiling)",
    "Regrouped": "pp_regrouped_kernel_ms: the context had no profiling on when the batch was regrouped (pp_ctx_set_profiling)",
    "Bgzf": "pp_bgzf_kernel_ms: the context had no profiling on when the blocks were inflated (pp_ctx_set_profiling)",
    "BamTagged": "pp_bam_out_kernel_ms: the context had no profiling on when the records were tagged (pp_ctx_set_profiling)",
    "BgzfDeflated": "pp_bgzf_out_kernel_ms: the context had no profiling on when the bytes were compressed (pp_ctx_set_profiling)"}
STAGE_HOOKS = {      # the internal per-stage hook of a class, its stages, the first one kernel_ms() counts (PreparedBatch has no hook)
    "BamOffsets": ("pp_bam_offs_stage_ms_", 3, 0), "BamRecords": ("pp_bam_stage_ms_", 3, 0), "Names": ("pp_names_stage_ms_", 5, 0),
    "GatedBatch": ("pp_gated_stage_ms_", 3, 0), "SamRecords": ("pp_sam_stage_ms_", 5, 1), "Regrouped": ("pp_regrouped_stage_ms_", 3, 0),
    "Bgzf": ("pp_bgzf_stage_ms_", 3, 0), "BamTagged": ("pp_bam_out_stage_ms_", 3, 0), "BgzfDeflated": ("pp_bgzf_out_stage_ms_", 3, 0)}


def _fetch(pp, c, addr, n, dt):
    """n items at a device address, through pp_ctx_download spelled by hand"""
    a = np.zeros(int(n), dt)
    if a.size:
        assert addr and pp.lib().pp_ctx_download(c._h, a.ctypes.data, addr, a.nbytes) == 0
    return a


def _fetch_batch(pp, c, ptrs, fields, n, seq_bytes, n_cig_total):
    sizes = {"seq": seq_bytes, "cigar": n_cig_total}
    return {k: _fetch(pp, c, ptrs[k], sizes.get(k, n), dt) for k, dt in fields}


def _same_arrays(got, want):
    assert list(got) == list(want)
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k


@pytest.mark.parametrize("profiling", (False, True))
def test_every_owned_object_reads_back_what_a_hand_written_download_reads(pp, profiling):
    """BamOffsets -> BamRecords -> Names.ids -> gate_records -> prepare_batch on device addresses, over three records -- an aligned
    one, a secondary one of the same read with SEQ "*", an unaligned one (zp is shorter than n_rec) -- and over a BAM that is a
    header only: host() of every object is what pp_ctx_download gives for the same pointers, the values are the models', close()
    twice is harmless, and kernel_ms() needs the context's profiling.  The other five owned classes over the same records and over the
    header alone: SamRecords on their SAM text, Regrouped, BamTagged -> BgzfDeflated -> Bgzf.  With profiling kernel_ms() is the
    sum of the stages the class's hook reports -- pp_sam's without its first, the copy of the text."""
    import bam_tag_model as tm
    import bgzf_deflate_model as dm
    import gate_model as gm
    import names_model as nm
    import regroup_model as rm
    import sam_records_model as sm
    from layout_check import same_records
    M = (8 << 4)
    recs = [bm.record(b"a", 0, 0, 5, [M], "ACGTACGT", bm.aux("NM", "C", 0)), bm.record(b"a", 256, 0, 20, [M], "", bm.aux("NM", "C", 1)),
            bm.record(b"u", 4, -1, -1, [], "ACGT")]
    hdr = bm.header_bytes([("c0", 64)], "@HD\tVN:1.6\n")
    data = hdr + bm.lay_out(recs)[0]
    at = bm.header(data)["records_at"]
    want_off = np.array(bm.walk(data, at)[0], np.uint64)
    want_raw = bm.decode(data, want_off)
    want_raw["read_id"] = np.array(nm.ids({}, [b"a", b"a", b"u"]), np.uint64)
    want_gate = gm.gate(want_raw)
    assert len(want_off) == 3 and len(want_raw["zp"]) == 2 and want_raw["seq_len"].tolist() == [8, 0, 4] and want_gate["counts"] == (2, 2, 1)
    contig_off = np.array([0, 64], np.uint64)
    c = pp.Context(0)
    c.set_profiling(profiling)
    made = []
    try:
        (dp, nb), _, keep = on_device(data, want_off)
        offs = pp.BamOffsets(c, (dp, nb), at, pp.MEM_DEVICE)
        made.append(offs)
        assert (offs.n_rec, offs.end) == (3, len(data))
        got = offs.host()
        assert got.dtype == np.uint64 and np.array_equal(got, want_off) and np.array_equal(got, _fetch(pp, c, offs.ptr, 3, np.uint64))

        rec = pp.BamRecords(c, (dp, nb), (offs.ptr, offs.n_rec), None, pp.MEM_DEVICE)
        made.append(rec)
        table = pp.Names(c)
        made.append(table)
        ids = table.ids(**rec.names(), mem=pp.MEM_DEVICE, out=rec.read_id_ptr)
        assert ids.dtype == np.uint64 and np.array_equal(ids, want_raw["read_id"]) and table.count == 2
        assert np.array_equal(ids, _fetch(pp, c, rec.read_id_ptr, 3, np.uint64))
        raw, names = rec.raw(), rec.names()["names"]
        by_hand = _fetch_batch(pp, c, raw, pp.RAW_FIELDS, 3, rec.seq_bytes, rec.n_cig_total)
        by_hand["name_off"], by_hand["name_len"] = _fetch(pp, c, names[1], 3, np.uint64), _fetch(pp, c, names[2], 3, np.uint32)
        got = rec.host()
        _same_arrays(got, by_hand)
        bm.same(got, want_raw)
        assert rec.zp.dtype == np.uint8 and np.array_equal(rec.zp, want_raw["zp"])

        g = pp.gate_records(c, raw, mem=pp.MEM_DEVICE)
        made.append(g)
        got = g.host()
        _same_arrays(got, _fetch_batch(pp, c, g.ptrs(), pp.REC_FIELDS, g.n_aln, g.seq_bytes, g.n_cig_total))
        gm.same(got, want_gate["recs"])
        assert g.counts == want_gate["counts"] and np.array_equal(g.orig(), want_gate["orig"]) and g.orig().dtype == np.uint32

        p = pp.prepare_batch(c, contig_off, g.n_aln, g.ptrs(), g.seq_bytes, g.n_cig_total, pp.MEM_DEVICE)
        made.append(p)
        ptrs = p.ptrs()
        by_hand = _fetch_batch(pp, c, ptrs, pp.REC_FIELDS, p.n_aln, p.seq_bytes, p.n_cig_total)
        by_hand["seq4"] = _fetch(pp, c, ptrs["seq4"], (p.seq_bytes + 1) // 2, np.uint8)
        by_hand["wo"] = _fetch(pp, c, ptrs["wo"], p.n_aln, pp.WO_DTYPE)
        by_hand["wo_runs"] = np.array([p.n_aln], np.uint64)
        got = p.host()
        _same_arrays(got, by_hand)
        src = want_gate["recs"]     # (same_records wants seq arrays of one length: the prepared rooms may take more than the gate's)
        assert len(got["seq"]) >= len(src["seq"])
        same_records(dict(src, seq=np.concatenate([src["seq"], np.zeros(len(got["seq"]) - len(src["seq"]), np.uint8)])), got)

        # a BAM that is its header only, through the host forms: no record, and an offsets array without entries is still one
        none = pp.BamOffsets(c, hdr, len(hdr))
        made.append(none)
        assert (none.n_rec, none.end) == (0, len(hdr)) and none.host().dtype == np.uint64 and len(none.host()) == 0
        empty = pp.BamRecords(c, hdr, none.host())
        made.append(empty)
        got = empty.host()
        bm.same(got, bm.decode(hdr, []))
        _same_arrays(got, dict(_fetch_batch(pp, c, empty.raw(), pp.RAW_FIELDS, 0, 0, 0), name_off=np.zeros(0, np.uint64), name_len=np.zeros(0, np.uint32)))
        assert (empty.n_rec, empty.seq_bytes, empty.n_cig_total, len(empty.zp)) == (0, 0, 0, 0)

        # ---- the other five classes.  The same three records as SAM text, and a text that is its header only ----
        head = b"@HD\tVN:1.6\n@SQ\tSN:c0\tLN:64\n"
        three = head + (b"a\t0\tc0\t6\t60\t8M\t*\t0\t0\tACGTACGT\t*\tNM:i:0\n" b"a\t256\tc0\t21\t60\t8M\t*\t0\t0\t*\t*\tNM:i:1\n"
                        b"u\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n")
        for text in (three, head):
            sam = pp.SamRecords(c, text)
            made.append(sam)
            want = sm.decode(text)
            by_hand = _fetch_batch(pp, c, sam.raw(), pp.RAW_FIELDS, sam.n_rec, sam.seq_bytes, sam.n_cig_total)
            for k, r in (("name", sam.names()["names"]), ("rname", sam.rnames()["names"])):
                by_hand[k + "_off"], by_hand[k + "_len"] = _fetch(pp, c, r[1], sam.n_rec, np.uint64), _fetch(pp, c, r[2], sam.n_rec, np.uint32)
            by_hand["line"] = _fetch(pp, c, pp.lib().pp_sam_lines(sam._p), sam.n_rec, np.uint32)
            got = sam.host()
            _same_arrays(got, by_hand)
            sm.same(got, want)
            assert sam.zp.dtype == np.uint8 and np.array_equal(sam.zp, want["zp"])
            assert (sam.n_rec, sam.seq_bytes, sam.n_cig_total) == (len(want["flag"]), len(text), len(want["cigar"]))
        for k in ("flag", "ref_start", "nm", "seq_len", "n_cig", "cigar", "zp"):      # (the text says what the BAM records say)
            assert np.array_equal(sm.decode(three)[k], want_raw[k]), k
        assert sam.n_rec == 0 and sm.seq_bytes(sm.decode(three)) == [b"ACGTACGT", b"", b"ACGT"]

        # regrouped: the three records from host memory (uploaded into the object; nothing moves), and the empty decode's null arrays
        rg_empty = None
        for src, raw_in, mem in ((want_raw, {k: want_raw[k] for k, _ in pp.RAW_FIELDS}, pp.MEM_HOST), (bm.decode(hdr, []), empty.raw(), pp.MEM_DEVICE)):
            rg_empty = rg = pp.regroup_records(c, raw_in, mem)
            made.append(rg)
            want = rm.regroup(src)
            got = rg.host()
            _same_arrays(got, _fetch_batch(pp, c, rg.raw(), pp.RAW_FIELDS, rg.n_rec, rg.seq_bytes, rg.n_cig_total))
            rm.same_raw(got, want["raw"])
            assert np.array_equal(got["seq"], src["seq"]) and np.array_equal(got["cigar"], src["cigar"])
            assert rg.counts() == want["counts"] and rg.perm().dtype == np.uint32 and np.array_equal(rg.perm(), want["perm"])
        assert rg_empty.n_rec == 0 and rg_empty.raw() == empty.raw()

        # tagged -> compressed -> inflated again: the three records with the second one failed, and the header alone
        for b, rec_off, src, off, passed, mem in (((dp, nb), (offs.ptr, 3), data, want_off, [1, 0], pp.MEM_DEVICE),
                                                  (hdr, none.host(), hdr, [], None, pp.MEM_HOST)):
            u = tm.tagged(src, len(hdr), off, passed)
            t = pp.BamTagged(c, b, len(hdr), rec_off, passed, mem)
            made.append(t)
            assert t.host().tobytes() == tm.frame(u) and np.array_equal(t.host(), _fetch(pp, c, t.bytes_ptr, t.n_bytes, np.uint8))
            assert t.counts == ((1, 1, 1) if passed else (0, 0, 1))
            z = t.deflate()
            made.append(z)
            want_file, want_blk, want_counts = dm.deflate_file(u)
            assert z.host().tobytes() == want_file and np.array_equal(z.host(), _fetch(pp, c, z.bytes_ptr, z.n_bytes, np.uint8))
            assert z.blk_off().tolist() == want_blk and np.array_equal(z.blk_off(), _fetch(pp, c, z.blk_off_ptr, z.n_blocks + 1, np.uint64))
            assert list(z.counts) == want_counts
            back = pp.Bgzf(c, (z.bytes_ptr, z.n_bytes), (z.blk_off_ptr, z.n_blocks), mem=pp.MEM_DEVICE)
            made.append(back)
            assert back.host().tobytes() == u and np.array_equal(back.host(), _fetch(pp, c, back.bytes_ptr, back.n_bytes, np.uint8))
        no_blocks = pp.Bgzf(c, b"", [])
        made.append(no_blocks)
        assert no_blocks.n_bytes == 0 and len(no_blocks.host()) == 0

        for o in made:
            # (a decode or a regroup of no records runs no kernel and times none: it answers as without profiling)
            if profiling and o is not empty and o is not rg_empty:
                ms = o.kernel_ms()
                assert isinstance(ms, float) and ms >= 0, o
                if type(o).__name__ in STAGE_HOOKS:      # kernel_ms() is the sum of the stages that count, in float as the library adds
                    hook, n_stages, first = STAGE_HOOKS[type(o).__name__]
                    stages = (C.c_float * n_stages)()
                    assert getattr(pp.lib(), hook)(o._p, stages) == 0, o
                    total = np.float32(0)
                    for v in stages[first:]:
                        total = np.float32(total + np.float32(v))
                    assert ms == float(total), (o, ms, list(stages))
            else:
                with pytest.raises(pp.PolypolishError) as e:
                    o.kernel_ms()
                assert (e.value.code, e.value.msg) == (pp.ERR_ARG, NO_PROFILING[type(o).__name__]), o
        del keep
    finally:
        for o in made[::-1]:
            o.close()
            o.close()
            assert not o._p
        c.close()
