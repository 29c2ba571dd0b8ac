"""pp_sam_records (pp_sam.hip) against tests/sam_records_model.py's decode, byte for byte -- the offsets of SEQ, QNAME and RNAME in the
text, the line numbers and the pass bytes included -- with the text in host memory and in device memory; there the allocation is exactly
n_bytes long.  A text the model refuses is refused with the model's code and line.  The shape of the generated inputs is pinned on the
CPU (tests/test_sam_records_model_cpu.py).  Nothing here depends on a fault.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import ingest_model as im
import names_model as nm
import sam_records_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def on_device(b, n=None):
    """(data, keep) for mem = MEM_DEVICE: the bytes in an allocation of exactly their length; n: the text is its first n bytes"""
    import torch
    dev = torch.device("cuda:0")
    t = torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to(dev) if len(b) else torch.zeros(1, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    return (t.data_ptr(), len(b) if n is None else n), t


def decoded(pp, ctx, whole, n, mem):
    """SamRecords on the first n bytes of `whole`, which lies in memory as it is: what follows the text follows it there, too"""
    if mem == pp.MEM_HOST:
        a = np.frombuffer(bytes(whole), np.uint8)
        return pp.SamRecords(ctx, a[:n], mem)
    data, keep = on_device(whole, n)
    rec = pp.SamRecords(ctx, data, mem)
    del keep            # (the caller's text may go when the call has returned)
    return rec


def check(pp, ctx, text, whole=None, want=None):
    """the device against the model on `text` (= the first len(text) bytes of `whole`), both mem forms -> the model's result or error"""
    whole = text if whole is None else whole
    try:
        want = want or sm.decode(text)
    except sm.SamError as m:
        for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
            with pytest.raises(pp.PolypolishError) as e:
                decoded(pp, ctx, whole, len(text), mem)
            assert (e.value.code, e.value.bad_record) == (m.code, m.bad_line), (mem, e.value, m)
        return m
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        rec = decoded(pp, ctx, whole, len(text), mem)
        try:
            got = rec.host()
            sm.same(got, want)
            assert rec.zp.dtype == np.uint8 and np.array_equal(rec.zp, want["zp"]), mem
            assert (rec.n_rec, rec.seq_bytes, rec.n_bytes, rec.n_cig_total) == (len(want["flag"]), len(text), len(text), len(want["cigar"]))
            assert np.array_equal(rec.lines(), want["line"])
            raw = rec.raw()
            assert (raw["n_rec"], raw["seq_bytes"], raw["n_cig_total"]) == (rec.n_rec, len(text), len(want["cigar"]))
            assert not rec.n_rec or (raw["read_id"] == rec.read_id_ptr and raw["contig"] == rec.contig_ptr and raw["seq"])
        finally:
            rec.close()
    return want


@pytest.mark.parametrize("name", sorted(im.CASES))
def test_the_ingest_cases(pp, ctx, name):
    """the texts built to the byte around the staging instances, the newline kernels' edges, CRLF, no final newline, a single line,
    QNAMEs around the eight-byte compare -- and the error cases: a line Alignment::new refuses with its code and line, a group the
    gate would refuse taken as the records it is"""
    c = im.case(name)
    for text in c.texts:
        got = check(pp, ctx, text)
        if c.error and c.error[1] in ("too_few_columns", "missing_NM_tag", "invalid_cigar", "flag", "pos", "nm", "cigar_overflow"):
            assert isinstance(got, sm.SamError) and (got.code, got.kind) == c.error
        elif name == "error_start_past_u32":
            assert isinstance(got, sm.SamError) and (got.code, got.kind) == (sm.LIMIT, "pos_above_u32")
        elif name in ("error_no_sequence_at_eof", "error_empty_cigar", "error_not_in_assembly", "error_empty_group"):
            assert isinstance(got, dict), "the decode takes what only the gate or the polish refuses"


def test_the_sentence_is_the_host_ingest_s(pp, ctx):
    for kind, (text, code, line) in sm.error_texts().items():
        with pytest.raises(pp.PolypolishError) as e:
            pp.SamRecords(ctx, text)
        assert (e.value.code, e.value.bad_record) == (code, line)
        if kind in ("too_few_columns", "missing_NM_tag"):
            assert e.value.msg == f'{kind.replace("_", " ")} in "text" (line {line + 1})'
        elif kind == "invalid_cigar":
            assert e.value.msg.startswith("encountered an invalid CIGAR string for read r5: \"24Q\"")
        else:
            assert f'in "text" (line {line + 1})' in e.value.msg


@pytest.mark.parametrize("n", sm.RECORD_COUNTS)
def test_record_counts_around_the_workgroup(pp, ctx, n):
    want = check(pp, ctx, sm.count_text(n))
    assert len(want["flag"]) == n
    if n in (sm.SAM_BLOCK - 1, sm.SAM_BLOCK, sm.SAM_BLOCK + 1):
        check(pp, ctx, sm.count_text(n, plain=True))


def test_cigars(pp, ctx):
    text, n_cig = sm.cigar_text()
    assert check(pp, ctx, text)["n_cig"].tolist() == n_cig


def test_tags(pp, ctx):
    text, nm_want, zp = sm.tag_text()
    want = check(pp, ctx, text)
    assert want["nm"].tolist() == nm_want and want["zp"].tolist() == zp


@pytest.mark.parametrize("case", sm.array_end_cases(), ids=lambda c: c[0])
def test_the_end_of_the_array(pp, ctx, case):
    """the text is the prefix of a larger array whose next bytes are hostile: the result is the model's on the prefix alone"""
    name, whole, n = case
    got = check(pp, ctx, whole[:n], whole)
    assert isinstance(got, sm.SamError) == (name == "inside_a_line")


def test_limits(pp, ctx):
    cases = sm.limit_texts()
    for kind in ("flag_above_u16", "pos_above_u32", "empty_seq"):
        text, line = cases[kind]
        m = check(pp, ctx, text)
        assert (m.code, m.bad_line) == (pp.ERR_LIMIT, line)
        with pytest.raises(pp.PolypolishError) as e:
            pp.SamRecords(ctx, text)
        assert f"(line {line + 1})" in e.value.msg
    assert isinstance(check(pp, ctx, cases["fits"][0]), dict)
    for text, code, line in sm.two_bad_lines():
        m = check(pp, ctx, text)
        assert (m.code, m.bad_line) == (code, line)
    # n_bytes >= 2^40 is refused before a byte is touched
    a = np.frombuffer(b"@CO\n", np.uint8)
    out, bad = C.c_void_p(12345), C.c_uint64(0)
    assert pp.lib().pp_sam_records(ctx._h, a.ctypes.data, 1 << 40, pp.MEM_HOST, C.byref(out), C.byref(bad)) == pp.ERR_LIMIT and out.value is None


def test_2_32_minus_1_lines_are_refused(pp, ctx):
    import torch
    n = (1 << 32) - 1
    t = torch.full((n,), 10, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(pp.PolypolishError) as e:
        pp.SamRecords(ctx, (t.data_ptr(), n), pp.MEM_DEVICE)
    assert e.value.code == pp.ERR_LIMIT and e.value.bad_record is None
    host = t.cpu().numpy()
    del t
    with pytest.raises(pp.PolypolishError) as e:
        pp.SamRecords(ctx, host, pp.MEM_HOST)
    assert e.value.code == pp.ERR_LIMIT
    rec = pp.SamRecords(ctx, host[:1000], pp.MEM_HOST)      # a thousand empty lines: no record
    assert rec.n_rec == 0
    rec.close()


def test_arg_errors(pp, ctx):
    text = sm.count_text(5)
    a = np.frombuffer(text, np.uint8)
    L = pp.lib()
    out, bad = C.c_void_p(12345), C.c_uint64(0)
    assert L.pp_sam_records(ctx._h, None, 5, pp.MEM_HOST, C.byref(out), C.byref(bad)) == pp.ERR_ARG and out.value is None
    assert L.pp_sam_records(ctx._h, a.ctypes.data, len(a), pp.MEM_HOST, None, C.byref(bad)) == pp.ERR_ARG
    assert L.pp_sam_records(None, a.ctypes.data, len(a), pp.MEM_HOST, C.byref(out), C.byref(bad)) == pp.ERR_ARG
    data, keep = on_device(text)
    for mem in (pp.MEM_PEER, 7):
        with pytest.raises(pp.PolypolishError) as e:
            pp.SamRecords(ctx, data, mem)
        assert e.value.code == pp.ERR_ARG
    del keep
    out = C.c_void_p()
    assert L.pp_sam_records(ctx._h, a.ctypes.data, len(a), pp.MEM_HOST, C.byref(out), None) == 0 and out.value    # bad_line may be NULL
    L.pp_sam_free(out)
    p = np.frombuffer(sm.count_text(5, plain=True), np.uint8)
    assert p[:3].tobytes() == b"r0\t" and L.pp_sam_records(ctx._h, p.ctypes.data, 3, pp.MEM_HOST, C.byref(out), None) == pp.ERR_QUIT and out.value is None


def test_a_byte_outside_ascii(pp, ctx):
    g, T = im.Gen(2), im.Text()
    T.add("@CO\tcomment")
    T.add(g.line())
    odd = bytearray(T.bytes())
    odd[5] = 0xC3
    m = check(pp, ctx, bytes(odd))
    assert (m.code, m.bad_line) == (pp.ERR_NOT_ASCII, None)
    # ... behind n_bytes it is nobody's
    want = check(pp, ctx, T.bytes(), T.bytes() + b"\xc3\xa9\n")
    assert len(want["flag"]) == 1


def test_degenerate_inputs(pp, ctx):
    for text in (b"", b"@HD\tVN:1.6\n@SQ\tSN:c\tLN:5\n", b"\n\n", b"@CO"):
        want = check(pp, ctx, text)
        assert len(want["flag"]) == 0 and len(want["zp"]) == 0
    rec = pp.SamRecords(ctx, b"")
    assert (rec.n_rec, rec.seq_bytes, rec.n_cig_total, len(rec.zp), len(rec.lines())) == (0, 0, 0, 0, 0)
    rec.close()


def test_two_objects_at_once_and_a_call_after_a_refused_one(pp, ctx):
    ta, tb = sm.count_text(65), sm.tag_text()[0]
    a, b = pp.SamRecords(ctx, ta), pp.SamRecords(ctx, on_device(tb)[0], pp.MEM_DEVICE)
    try:
        bad = sm.error_texts()["nm"]
        with pytest.raises(pp.PolypolishError) as e:
            pp.SamRecords(ctx, bad[0])
        assert (e.value.code, e.value.bad_record) == bad[1:]
        sm.same(b.host(), sm.decode(tb))
        sm.same(a.host(), sm.decode(ta))
        check(pp, ctx, ta)
    finally:
        a.close()
        b.close()


def test_kernel_ms_needs_profiling(pp):
    c = pp.Context(0)
    try:
        rec = pp.SamRecords(c, sm.count_text(65))
        with pytest.raises(pp.PolypolishError) as e:
            rec.kernel_ms()
        assert e.value.code == pp.ERR_ARG and "pp_sam_kernel_ms" in e.value.msg
        rec.close()
        c.set_profiling(True)
        rec = pp.SamRecords(c, sm.count_text(65))
        st = rec.stage_ms()
        assert rec.kernel_ms() > 0 and list(st) == ["copy", "newline_index", "scan", "place", "cigar"] and min(st.values()) >= 0
        rec.close()
    finally:
        c.close()


def test_names_and_rnames_fill_read_id_and_contig(pp, ctx):
    g, T = im.Gen(370, (3000, 500)), im.Text()
    qn = ["a", "a", "", "b", "*", "a", "abcdefghi", "abcdefghj", "", "b"]
    rn = ["ctg0", "ctg1", "elsewhere", "*", "ctg1", "ctg0", "elsewhere", "other", "ctg0", "*"]
    T.add("@HD\tVN:1.6")
    for i, (q, r) in enumerate(zip(qn, rn)):
        T.add(unaligned_or(g, i, q, r))
    text = T.bytes()
    want = sm.decode(text)
    assert sm.column(want, "name") == [q.encode() for q in qn] and sm.column(want, "rname") == [r.encode() for r in rn]
    assert want["name_len"].tolist().count(0) == 2
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        rec = decoded(pp, ctx, text, len(text), mem)
        reads, contigs = pp.Names(ctx), pp.Names(ctx, 2)
        try:
            state = {}
            assert contigs.ids(["ctg0", "ctg1"]).tolist() == nm.ids(state, [b"ctg0", b"ctg1"])
            got = contigs.ids(**rec.rnames(), mem=pp.MEM_DEVICE, out32=rec.contig_ptr)
            assert got.tolist() == nm.ids(state, [r.encode() for r in rn]) == [0, 1, 2, 3, 1, 0, 2, 4, 0, 3]
            ids = reads.ids(**rec.names(), mem=pp.MEM_DEVICE, out=rec.read_id_ptr)
            assert ids.tolist() == nm.ids({}, [q.encode() for q in qn])
            h = rec.host()
            assert h["contig"].dtype == np.uint32 and h["contig"].tolist() == got.tolist()
            assert h["read_id"].dtype == np.uint64 and h["read_id"].tolist() == ids.tolist()
            assert reads.name(int(ids[2])) == b"" and contigs.name(4) == b"other"
        finally:
            reads.close()
            contigs.close()
            rec.close()


def unaligned_or(g, i, qname, rname):
    if i % 4 == 3:
        return g.line(name=qname, flag=4, cigar="*", nm=None, rname=rname)
    return g.line(name=qname, rname=rname, contig=0)
