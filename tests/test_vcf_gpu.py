"""pp_polish_vcf (pp_k_vcf.h) through the C ABI, byte for byte against tests/vcf_model.py.  The model is fed from the ORACLE on the same
records (oracle.polish_records, per-position emitted bytes), never from the device; the device's polished bytes are the oracle's
(asserted: the precondition), and apply(assembly, device VCF) gives them back.  The jobs are hand-built (tests/vcf_jobs.py): min_depth
1, reads that all carry the wanted edits, '-' assembly bytes where a run has to reach what no read covers.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import vcf_jobs as vj
import vcf_model as vm

pytestmark = pytest.mark.gpu

# the kernels' tile constants (polypolish_amd/csrc/pp_k_vcf.h: VCF_PPT, VCF_TILE, VCF_LANE, VCF_TEXT_WG), repeated here and checked
# against the library's own report below
PPT, TILE, LANE, TEXT_WG = 8, 2048, 16, 16384
SCAN1_THREADS = 1024  # k_colscan<1> (pp_dev.h): one thread scans ceil(workgroups / 1024) workgroup sums


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def _names(n):
    return [b"contig_%d" % (i + 1) for i in range(n)]


def _expected(pp, orc, off, bases, recs, names, spec=None):
    res = orc.polish_records(off, bases, recs, min_depth=1, positions=True)
    nb = vj.new_bases(res)
    if spec is not None:
        vj.check_oracle_made(bases, spec, nb)
    return res, vm.vcf_from_positions(names, off, bytes(bases), nb, pp.lib().pp_version())


def _first_diff(got, want):
    i = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return len(got), len(want), i, got[max(0, i - 40):i + 40], want[max(0, i - 40):i + 40]


def _same(got, want):
    assert got == want, _first_diff(got, want)


def _applies_back(off, bases, names, vcf, polished, out_off):
    contigs = [(n, bytes(bases[int(off[i]):int(off[i + 1])])) for i, n in enumerate(names)]
    assert [s for _, s in vm.apply(contigs, vcf)] == [polished[int(out_off[i]):int(out_off[i + 1])] for i in range(len(names))]


def _job(pp, ctx, orc, off, bases, spec, names=None, cover=None, **kw):
    """the job on the device and on the oracle; the device's VCF against the model's; returns (vcf bytes, Vcf object's record count)"""
    names = names or _names(len(off) - 1)
    recs = vj.reads(off, bases, spec, cover=cover)
    want_res, want = _expected(pp, orc, off, bases, recs, names, spec)
    res = ctx.polish_records(off, bases, recs, min_depth=1, **kw)
    assert res["polished"] == want_res["polished"], "the device's job is the oracle's"
    v = pp.Vcf(ctx, names)
    try:
        got = v.bytes()
        _same(got, want)
        assert v.n_records == len(vm.parse(got)[1]) and v.n_bytes == len(want)
    finally:
        v.close()
    _applies_back(off, bases, names, got, res["polished"], res["offsets"])
    return got


def _edit(kind, base):
    return {"sub": vj.other(base), "ins": bytes([base]) + vj.other(base, 2), "ins3": bytes([base]) + b"TTG", "del": b"-",
            "delins": b"-" + vj.other(base), "delsame": b"-" + bytes([base])}[kind]


def test_the_tile_constants_are_the_kernels(pp):
    assert pp.vcf_geometry() == (PPT, TILE, LANE, TEXT_WG)


# ---- 1. one edit of each kind at every offset from 0 to two workgroups' worth of positions plus 2 ----------------------------------
# (every third position of one job: the edits of a job stay records of their own; a deletion cannot begin a read, so offset 0 of the
# deleting kinds is the '-' assembly byte of test_contig_boundaries)
@pytest.mark.parametrize("phase", [0, 1, 2])
@pytest.mark.parametrize("kind", ["sub", "ins", "ins3", "del", "delins", "delsame"])
def test_every_offset(pp, ctx, orc, kind, phase):
    off, bases = vj.assembly([2 * TILE + 2 + 64, 300], 5)
    spec = {p: _edit(kind, int(bases[p])) for p in range(phase, 2 * TILE + 3, 3) if p or kind in ("sub", "ins", "ins3")}
    got = _job(pp, ctx, orc, off, bases, spec)
    n = len(vm.parse(got)[1])
    assert n == (0 if kind == "delsame" else len(spec)), "a multi-byte winner that leaves the assembly's byte is no edit"


# ---- 2. runs at the seams -----------------------------------------------------------------------------------------------------------
def test_runs_begin_end_and_straddle_the_workgroup_boundaries(pp, ctx, orc):
    """substitution, deletion and insertion runs that begin on, end on and straddle a boundary of the position passes' workgroups (and
    of the scan's per-thread stretches: one workgroup sum per thread here); one run longer than a workgroup's positions; runs that are
    a whole contig, one of them longer than a workgroup's positions"""
    lens = [5 * TILE + 64, TILE + 900, 5, TILE + 700, 400]
    off0 = np.concatenate([[0], np.cumsum(lens)])
    dash = list(range(int(off0[2]), int(off0[3]))) + list(range(int(off0[3]), int(off0[4])))  # contigs 3 and 4: '-' throughout
    off, bases = vj.assembly(lens, 6, dash=dash)
    spec = {}
    for lo, hi, kind in ((TILE, TILE + 7, "sub"), (2 * TILE - 6, 2 * TILE, "sub"), (3 * TILE - 5, 3 * TILE + 5, "sub"),
                         (4 * TILE - 3, 4 * TILE + 4, "del"), (TILE + 500, TILE + 504, "ins"), (PPT * 31 - 1, PPT * 31 + 1, "del"),
                         (int(off0[1]) + 150, int(off0[1]) + TILE + 450, "sub")):  # the last one: 2,348 positions, across two boundaries
        for p in range(lo, hi):
            spec[p] = _edit(kind, int(bases[p]))
    got = _job(pp, ctx, orc, off, bases, spec)
    recs = vm.parse(got)[1]
    assert max(len(r[2]) for r in recs) == TILE + 700 and (b"contig_4", 1, b"-" * (TILE + 700), b"<DEL>") in recs
    assert (b"contig_3", 1, b"-----", b"<DEL>") in recs and any(len(r[2]) == TILE + 300 for r in recs)


@pytest.mark.parametrize("side", ["last", "both", "first"])
@pytest.mark.parametrize("B", [TILE - 1, TILE, TILE + 1, TILE + PPT])
def test_contig_boundaries_on_and_next_to_a_workgroup_boundary(pp, ctx, orc, B, side):
    """contig 2 begins at global position B; the last position of contig 1 ('-': no read reaches a contig's end), the first of contig 2
    (a substitution, or '-': the deletion at offset 0 with its anchor behind it) or both are edited: records of their own"""
    dash = [B - 1] if side != "first" else []
    sub_first = side != "last"
    off, bases = vj.assembly([B, 600], 7, dash=dash + ([B + 300] if side == "both" else []))
    spec = {B - 40: _edit("ins", int(bases[B - 40])), B + 50: _edit("del", int(bases[B + 50]))}
    if sub_first:
        spec[B] = _edit("sub", int(bases[B]))
    got = _job(pp, ctx, orc, off, bases, spec)
    recs = vm.parse(got)[1]
    if side != "first":
        assert (b"contig_1", B - 1, bytes(bases[B - 2:B]), bytes(bases[B - 2:B - 1])) in recs
    if sub_first:
        assert (b"contig_2", 1, bytes(bases[B:B + 1]), spec[B]) in recs


def test_a_deletion_at_offset_0_and_contigs_of_one_base(pp, ctx, orc):
    lens = [1, 1, 300, 1, 1, 2, 200, 1]
    off0 = np.concatenate([[0], np.cumsum(lens)])
    dash = [0, int(off0[2]), int(off0[2]) + 1, int(off0[3]), int(off0[5]), int(off0[6]), int(off0[7])]
    off, bases = vj.assembly(lens, 8, dash=dash)
    spec = {int(off0[2]) + 100: b"-", int(off0[6]) + 60: _edit("sub", int(bases[int(off0[6]) + 60]))}
    got = _job(pp, ctx, orc, off, bases, spec)
    recs = vm.parse(got)[1]
    assert (b"contig_1", 1, b"-", b"<DEL>") in recs and (b"contig_4", 1, b"-", b"<DEL>") in recs and (b"contig_8", 1, b"-", b"<DEL>") in recs
    b2 = int(off0[2])
    assert (b"contig_3", 1, b"--" + bytes(bases[b2 + 2:b2 + 3]), bytes(bases[b2 + 2:b2 + 3])) in recs  # positions 0..1: the anchor behind
    assert (b"contig_6", 1, b"-" + bytes(bases[int(off0[5]) + 1:int(off0[5]) + 2]), bytes(bases[int(off0[5]) + 1:int(off0[5]) + 2])) in recs
    assert not [r for r in recs if r[0] in (b"contig_2", b"contig_5")]


# ---- 3. POS at its digit seams, a scan whose threads take two workgroup sums each ----------------------------------------------------
def test_pos_digit_seams_on_a_long_contig(pp, ctx, orc):
    """POS 9|10 ... 999,999|1,000,000 (a substitution at POS 10^k - 1, a deletion anchored at POS 10^k) on a 1 Mbp contig with sparse
    reads; with the second contig the assembly has more than 1024 workgroups, so a thread of the scan adds two sums, and a run
    straddles such a thread's boundary"""
    L0 = 1_000_100
    off, bases = vj.assembly([L0, 1_200_000], 9)
    assert (int(off[-1]) + TILE - 1) // TILE > SCAN1_THREADS
    spec, cover = {}, []
    for k in range(1, 7):
        q = 10 ** k
        spec[q - 2] = _edit("sub", int(bases[q - 2]))
        spec[q] = b"-"
        cover.append((max(0, q - 150), min(q + 150, L0)))
    seam = 2 * TILE * ((L0 + 400_000) // (2 * TILE))  # a multiple of two workgroups' positions, inside contig 2
    for p in range(seam - 4, seam + 4):
        spec[p] = _edit("sub", int(bases[p]))
    cover.append((seam - 150, seam + 150))
    cover = sorted(set(cover))
    got = _job(pp, ctx, orc, off, bases, spec, cover=[cover[0]] + [c for i, c in enumerate(cover[1:]) if c[0] >= cover[i][1]])
    pos = [r[1] for r in vm.parse(got)[1] if r[0] == b"contig_1"]
    for k in range(1, 7):
        assert 10 ** k - 1 in pos and 10 ** k in pos
    assert (b"contig_2", seam - 4 - L0 + 1, bytes(bases[seam - 4:seam + 4]), b"".join(spec[p] for p in range(seam - 4, seam + 4))) in vm.parse(got)[1]


# ---- 4. names and where the records begin in the text ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_job(pp, ctx, orc):
    off, bases = vj.assembly([900, 500], 10, dash=[899])
    spec = {p: _edit(k, int(bases[p])) for p, k in ((0, "sub"), (17, "ins"), (300, "del"), (301, "del"), (640, "delins"), (905, "ins3"),
                                                    (1200, "sub"), (1201, "sub"))}
    recs = vj.reads(off, bases, spec)
    res = orc.polish_records(off, bases, recs, min_depth=1, positions=True)
    nb = vj.new_bases(res)
    vj.check_oracle_made(bases, spec, nb)
    return off, bases, recs, res, nb


def _polish(ctx, job, **kw):
    off, bases, recs, res, _ = job
    got = ctx.polish_records(off, bases, recs, min_depth=1, **kw)
    assert got["polished"] == res["polished"]


def _want(pp, job, names):
    off, bases, _, _, nb = job
    return vm.vcf_from_positions(names, off, bytes(bases), nb, pp.lib().pp_version())


def test_names_of_every_length_and_every_alignment_of_the_records(pp, ctx, small_job):
    """names of 1, 255 and more bytes than a workgroup has threads (256); 16 consecutive name lengths move the header's end -- where the
    first record begins -- through every offset modulo the 16 bytes of a store"""
    _polish(ctx, small_job)
    seen = set()
    for n in [1, 255, 257, 700] + list(range(20, 36)):
        names = [b"x" * n, (b"name with spaces;=<> " * 40)[:n] if n > 35 or n == 1 else b"seven b"]  # (in the sweep one name grows)
        v = pp.Vcf(ctx, names)
        got = v.bytes()
        v.close()
        _same(got, _want(pp, small_job, names))
        seen.add(got.index(b"\n" + names[0] + b"\t") % LANE)
    assert seen == set(range(LANE))
    v = pp.Vcf(ctx, ["a", "b"])  # (str names are encoded)
    _same(v.bytes(), _want(pp, small_job, [b"a", b"b"]))
    v.close()


# ---- 5. the same bytes whatever the job's path; job after job; the seq array gone ----------------------------------------------------------
def test_same_bytes_with_debug_on_and_off(pp, ctx, small_job):
    names = _names(2)
    want = _want(pp, small_job, names)
    for debug in (False, True, False):
        _polish(ctx, small_job, debug=debug)
        v = pp.Vcf(ctx, names)
        _same(v.bytes(), want)
        v.close()
    _polish(ctx, small_job, debug=True)
    tsv = ctx.debug_tsv([n.decode() for n in names])
    v = pp.Vcf(ctx, names)  # behind the --debug formatter, and the formatter behind it
    _same(v.bytes(), want)
    v.close()
    assert ctx.debug_tsv([n.decode() for n in names]) == tsv
    assert vm.from_debug_tsv(names, small_job[0], bytes(small_job[1]), b"name\tpos\t\n" + tsv, pp.lib().pp_version()) == want


def test_same_bytes_for_a_prepared_batch_and_a_plain_one(pp, ctx, small_job):
    off, bases, recs, res, _ = small_job
    names = _names(2)
    want = _want(pp, small_job, names)
    prep = pp.prepare_records(ctx, off, recs)
    try:
        ctx.polish_begin(off, bases.ctypes.data, pp.MEM_HOST, min_depth=1)
        ctx.polish_add_ptrs(prep.n_aln, prep.ptrs(), prep.seq_bytes, prep.n_cig_total, pp.MEM_DEVICE)
        ctx.polish_finish()
        assert ctx.took_direct_path()
        assert ctx.result()[0] == res["polished"]
        v = pp.Vcf(ctx, names)
        _same(v.bytes(), want)
        v.close()
    finally:
        prep.close()
    _polish(ctx, small_job)
    assert not ctx.took_direct_path()
    v = pp.Vcf(ctx, names)
    _same(v.bytes(), want)
    v.close()


def test_the_seq_array_overwritten_after_finish(pp, ctx, small_job):
    """the caller's batch lies in device memory of its own and is used in place; once the job is finished its SEQ bytes are overwritten:
    ALT comes from the polished output"""
    import torch
    off, bases, recs, res, _ = small_job
    names = _names(2)
    dev = {k: torch.from_numpy(np.ascontiguousarray(recs[k], dtype=dt).view(np.uint8).copy()).to("cuda:0") for k, dt in pp.REC_FIELDS}
    torch.cuda.synchronize()
    ctx.polish_begin(off, bases.ctypes.data, pp.MEM_HOST, min_depth=1)
    ctx.polish_add_ptrs(len(recs["contig"]), {k: t.data_ptr() for k, t in dev.items()}, len(recs["seq"]), len(recs["cigar"]), pp.MEM_DEVICE)
    ctx.polish_finish()
    assert ctx.result()[0] == res["polished"]
    dev["seq"].fill_(ord("N"))
    torch.cuda.synchronize()
    v = pp.Vcf(ctx, names)
    _same(v.bytes(), _want(pp, small_job, names))
    v.close()


def test_two_jobs_one_after_the_other_on_one_context(pp, orc):
    c = pp.Context(0)
    try:
        for seed, kind, lens in ((21, "sub", [700, 300]), (22, "ins", [3000]), (23, "del", [300, 300, 300])):
            off, bases = vj.assembly(lens, seed)
            spec = {p: _edit(kind, int(bases[p])) for p in range(10 + seed, int(off[-1]) - 250, 37)}
            _job(pp, c, orc, off, bases, spec)
        off, bases = vj.assembly([500], 24)  # ... and a job without an edit: the header alone
        got = _job(pp, c, orc, off, bases, {})
        assert vm.parse(got)[1] == [] and got.endswith(vm.COLUMNS)
    finally:
        c.close()


# ---- 6. the object, the times, the refusals ------------------------------------------------------------------------------------------------
def test_write_deflate_and_times(pp, ctx, small_job, tmp_path):
    import gzip
    names = _names(2)
    want = _want(pp, small_job, names)
    _polish(ctx, small_job)
    v = pp.Vcf(ctx, names)
    with pytest.raises(pp.PolypolishError) as e:
        v.kernel_ms()
    assert e.value.code == pp.ERR_ARG and "pp_ctx_set_profiling" in e.value.msg
    path = str(tmp_path / "a.vcf")
    v.write(path)
    assert open(path, "rb").read() == want
    z = v.deflate()
    assert gzip.decompress(z.host().tobytes()) == want
    z.close()
    v.close()
    ctx.set_profiling(True)
    try:
        v = pp.Vcf(ctx, names)
        st = v.stage_ms()
        assert set(st) == {"mark", "runs", "records", "text"} and all(x >= 0 for x in st.values())
        assert abs(v.kernel_ms() - sum(st.values())) < 1e-3
        _same(v.bytes(), want)
        v.close()
    finally:
        ctx.set_profiling(False)


def _refused(pp, fn, *words):
    with pytest.raises(pp.PolypolishError) as e:
        fn()
    assert e.value.code == pp.ERR_ARG and all(w in e.value.msg for w in words), e.value.msg


def test_refusals(pp, orc, small_job):
    off, bases, recs, res, _ = small_job
    names = _names(2)
    c = pp.Context(0)
    try:
        L = pp.lib()
        _refused(pp, lambda: pp.Vcf(c, names), "pp_polish_vcf", "no finished polish job")
        c.polish_begin(off, bases.ctypes.data, pp.MEM_HOST, min_depth=1)  # an open job is no finished one
        _refused(pp, lambda: pp.Vcf(c, names), "no finished polish job")
        bad = {k: np.array(v, copy=True) for k, v in recs.items()}
        bad["ref_start"][3] = 890  # runs off its contig
        with pytest.raises(pp.PolypolishError):
            c.polish_records(off, bases, bad, min_depth=1)
        _refused(pp, lambda: pp.Vcf(c, names), "no finished polish job", "ended in an error")
        c.polish_records(off, bases, recs, min_depth=1, emit=[(0, 900), (0, 250)])
        _refused(pp, lambda: pp.Vcf(c, names), "pp_polish_set_emit", "edges")
        c.polish_records(off, bases, recs, min_depth=1)
        _refused(pp, lambda: pp.Vcf(c, [b"a\tb", b"c"]), "tab or a newline")
        _refused(pp, lambda: pp.Vcf(c, [b"a", b"c\nd"]), "tab or a newline")
        p = C.c_void_p()
        arr = (C.c_char_p * 2)(b"a", None)
        assert L.pp_polish_vcf(c._h, C.cast(arr, C.c_void_p), C.byref(p)) == pp.ERR_ARG and not p.value and b"name is NULL" in L.pp_last_error(c._h)
        assert L.pp_polish_vcf(c._h, None, C.byref(p)) == pp.ERR_ARG and b"null argument" in L.pp_last_error(c._h)
        arr = (C.c_char_p * 2)(b"a", b"b")
        assert L.pp_polish_vcf(c._h, C.cast(arr, C.c_void_p), None) == pp.ERR_ARG and b"null argument" in L.pp_last_error(c._h)
        assert L.pp_polish_vcf(None, C.cast(arr, C.c_void_p), C.byref(p)) == pp.ERR_ARG
        v = pp.Vcf(c, names)  # ... and the context still makes the text
        _same(v.bytes(), _want(pp, small_job, names))
        v.close()
    finally:
        c.close()
