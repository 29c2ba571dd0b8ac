"""`polypolish filter / filter-polish --sort_out --out_bai` on the golden pair (tests/golden/derived_e2e), as BAM and as SAM text with
--out_bam: the outputs against the models' sorted files (tests/bam_sort_model.py: sorted_stream, bai) byte for byte, the records as a
multiset against the run without the flags, the log against the plain run's, the FASTA against the committed one, `polish --regroup`
on the sorted outputs, the refusals -- none leaves an output behind -- and the same through Python.  The text's QUAL columns are made
as long as their SEQ (sam_bam_model.with_fitting_qual), as tests/test_out_bam_cli_gpu.py does.  Every command test runs bin/polypolish
as a child process.  Needs an MI355X: `-m gpu`."""
import gzip
import os
import re
import struct

import numpy as np
import pytest

import bam_model as bm
import bam_sort_model as sm
import bam_tag_model as tm
import bgzf_deflate_model as D
import sam_bam_model as sb
from test_bam_cli_gpu import put, run
from test_bgzf_chain_gpu import bgzf_file, cut_points

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derived_e2e")


def io(ins, outs):
    return ["--in1", ins[0], "--in2", ins[1], "--out1", outs[0], "--out2", outs[1]]


def the_log(r, outs):
    log = r.stderr.decode()
    for k, p in enumerate(outs):
        log = log.replace(p, f"<out{k + 1}>")
    return re.sub(r"Time to run: .*\n", "", log)


def sorted_files(b, at, off, verdict):
    """the models' sorted stream, compressed file and .bai of one input"""
    s = sm.sort(b, at, off)
    v = sm.carry_pass(s["flag"], s["perm"], verdict)
    u = sm.tagged_head(b, at, s["rec_off"], v, s["head"])
    z, blk, _ = D.deflate_file(u)
    return {"stream": u, "file": z, "bai": sm.bai(b, len(s["head"]), s["rec_off"], v, len(bm.header(s["head"])["names"]), blk), "n_head": len(s["head"])}


@pytest.fixture(scope="module")
def ds(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sort_out_cli"))
    lens = {}
    for ent in open(os.path.join(GOLDEN, "case.fasta")).read().split(">")[1:]:
        name, seq = ent.split("\n", 1)
        lens[name.split()[0]] = len(seq.replace("\n", ""))
    texts = [sb.with_fitting_qual(open(os.path.join(GOLDEN, f"case_{f}.sam"), "rb").read()) for f in (1, 2)]
    sams = [put(os.path.join(d, f"case_{f + 1}.sam"), t) for f, t in enumerate(texts)]
    plain = [os.path.join(d, f"plain_{f}.sam") for f in (1, 2)]
    p = run("filter", *io(sams, plain))
    assert p.returncode == 0, p.stderr.decode()[-800:]
    out = {"dir": d, "fasta": os.path.join(GOLDEN, "case.fasta"), "sams": sams, "texts": texts, "bams": [], "encs": [], "verdicts": [], "from_bam": [], "from_text": [],
           "polished": open(os.path.join(GOLDEN, "polished_after_filter.fasta"), "rb").read()}
    for f, text in enumerate(texts):
        verdict = tm.own_verdicts(text, open(plain[f], "rb").read())
        assert (verdict == 0).any()
        names = [ln.split("\t")[1][3:] for ln in text.decode().split("\n") if ln.startswith("@SQ")]
        enc = bm.encode(text, names, [lens[n] for n in names])
        b, at = enc["header"] + enc["records"], len(enc["header"])
        out["encs"].append((b, at, enc["rec_off"] + np.uint64(at)))
        out["bams"].append(put(os.path.join(d, f"case_{f + 1}.bam"), bgzf_file(b, cut_points(len(b), set()))))
        out["verdicts"].append(verdict)
        out["from_bam"].append(sorted_files(b, at, enc["rec_off"] + np.uint64(at), verdict))
        m = sb.encode(text)
        out["from_text"].append(sorted_files(m["bytes"], m["records_at"], m["rec_off"], verdict))
    return out


def records(u, at):
    return sorted(u[o:o + 4 + bm._le32(u, o)] for o in bm.walk(u, at)[0])


@pytest.mark.parametrize("route", ("bam", "text"))
def test_filter_writes_the_models_sorted_files_and_indexes(ds, route, tmp_path):
    ins, flags, want = (ds["bams"], [], ds["from_bam"]) if route == "bam" else (ds["sams"], ["--out_bam"], ds["from_text"])
    outs = [str(tmp_path / f"sorted_{i}.bam") for i in (1, 2)]
    unsorted = [str(tmp_path / f"unsorted_{i}.bam") for i in (1, 2)]
    r = run("filter", "--sort_out", "--out_bai", *flags, *io(ins, outs))
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()[-800:]
    p = run("filter", *flags, *io(ins, unsorted))
    assert p.returncode == 0, p.stderr.decode()[-800:]
    assert the_log(r, outs) == the_log(p, unsorted), "the log is the plain run's"
    for f in range(2):
        got = open(outs[f], "rb").read()
        u = gzip.decompress(got)
        assert u == want[f]["stream"], f
        assert got == want[f]["file"], f
        assert open(outs[f] + ".bai", "rb").read() == want[f]["bai"], f
        was = gzip.decompress(open(unsorted[f], "rb").read())
        assert records(u, want[f]["n_head"]) == records(was, bm.header(was)["records_at"]), "the same records, tags included"
        assert not os.path.exists(unsorted[f] + ".bai")
        keys = [sm.key_of(*sm.fields(u, o)) for o in bm.walk(u, want[f]["n_head"])[0]]
        assert keys == sorted(keys) and b"SO:coordinate" in u[:want[f]["n_head"]]
    only = [str(tmp_path / f"only_sorted_{i}.bam") for i in (1, 2)]
    assert run("filter", "--sort_out", *flags, *io(ins, only)).returncode == 0
    assert [open(x, "rb").read() for x in only] == [w["file"] for w in want] and not os.path.exists(only[0] + ".bai")
    # the round trip: the sorted outputs polish to what the two commands give
    r = run("polish", "--regroup", ds["fasta"], *outs)
    assert r.returncode == 0 and r.stdout == ds["polished"], r.stderr.decode()[-800:]


@pytest.mark.parametrize("route", ("bam", "text"))
def test_filter_polish_with_the_flags(ds, route, tmp_path):
    ins, flags, want = (ds["bams"], [], ds["from_bam"]) if route == "bam" else (ds["sams"], ["--out_bam"], ds["from_text"])
    outs = [str(tmp_path / f"fused_{i}.bam") for i in (1, 2)]
    plain = [str(tmp_path / f"fused_plain_{i}.bam") for i in (1, 2)]
    r = run("filter-polish", "--sort_out", "--out_bai", *flags, *io(ins, outs), ds["fasta"])
    assert r.returncode == 0 and r.stdout == ds["polished"], r.stderr.decode()[-800:]
    p = run("filter-polish", *flags, *io(ins, plain), ds["fasta"])
    assert p.returncode == 0 and p.stdout == ds["polished"] and the_log(r, outs) == the_log(p, plain)
    for f in range(2):
        assert open(outs[f], "rb").read() == want[f]["file"] and open(outs[f] + ".bai", "rb").read() == want[f]["bai"], f
    r = run("filter-polish", "--sort_out", *flags, "--in1", ins[0], "--in2", ins[1], ds["fasta"])      # no outputs: nothing to sort
    assert r.returncode == 0 and r.stdout == ds["polished"]


def test_refusals_leave_no_output_behind(ds, tmp_path):
    outs = [str(tmp_path / f"never_{i}.bam") for i in (1, 2)]
    gone = lambda: not any(os.path.exists(x) or os.path.exists(x + ".bai") for x in outs)      # noqa: E731
    for cmd, tail in (("filter", []), ("filter-polish", [ds["fasta"]])):
        r = run(cmd, "--out_bai", *io(ds["bams"], outs), *tail)
        assert r.returncode == 1 and "--out_bai needs --sort_out" in r.stderr.decode() and gone(), r.stderr.decode()[-400:]
        r = run(cmd, "--sort_out", *io(ds["sams"], outs), *tail)                                # SAM text in, SAM text out
        assert r.returncode == 1 and "--sort_out takes BAM outputs" in r.stderr.decode() and gone(), r.stderr.decode()[-400:]
        r = run(cmd, "--sort_out", "--out_sam", *io(ds["bams"], outs), *tail)
        assert r.returncode == 1 and "--sort_out takes BAM outputs" in r.stderr.decode() and "--out_sam" in r.stderr.decode() and gone()
    # a record of the SECOND file that the index refuses: it ends behind 2^29
    b, at, off = ds["encs"][1]
    names = bm.header(b)["names"]
    header = bm.header_bytes([(n.decode(), 1 << 30) for n in names], "@HD\tVN:1.6\n")
    body = bytearray(b[at:])
    k = next(i for i, o in enumerate(off) if not b[int(o) + 18] & 4 and sm.fields(b, int(o))[0] == 0) + 0
    struct.pack_into("<i", body, int(off[k]) - at + 8, (1 << 29) - 2)
    data = header + bytes(body)
    bad = put(tmp_path / "far_2.bam", bgzf_file(data, cut_points(len(data), set())))
    r = run("filter", "--sort_out", "--out_bai", *io([ds["bams"][0], bad], outs))
    msg = r.stderr.decode()
    assert r.returncode == 1 and "--sort_out" in msg and f'"{bad}"' in msg and "2^29" in msg and "record " in msg, msg[-800:]
    assert gone(), "neither file and neither index"
    assert run("filter", "--sort_out", *io([ds["bams"][0], bad], outs)).returncode == 0, "without the index the far record is sorted like any other"


def test_the_python_face(ds, tmp_path):
    import polypolish_amd as pp
    ctx = pp.Context(0)
    try:
        outs = [str(tmp_path / f"py_{i}.bam") for i in (1, 2)]
        rep = ctx.filter_files(ds["bams"][0], ds["bams"][1], outs[0], outs[1], sort_out=True, out_bai=True)
        assert rep["after"] == int(sum(v.sum() for v in ds["verdicts"]))
        assert [open(x, "rb").read() for x in outs] == [w["file"] for w in ds["from_bam"]]
        assert [open(x + ".bai", "rb").read() for x in outs] == [w["bai"] for w in ds["from_bam"]]
        again = [str(tmp_path / f"py_plain_{i}.bam") for i in (1, 2)]
        ctx.filter_files(ds["bams"][0], ds["bams"][1], again[0], again[1])
        assert not os.path.exists(again[0] + ".bai") and b"SO:coordinate" not in gzip.decompress(open(again[0], "rb").read())[:200], "the flags held for one call"
        fasta, _ = ctx.filter_polish_files(ds["fasta"], ds["sams"][0], ds["sams"][1], outs[0], outs[1], out_bam=True, sort_out=True, out_bai=True)
        assert fasta == ds["polished"] and [open(x, "rb").read() for x in outs] == [w["file"] for w in ds["from_text"]]
        with pytest.raises(pp.PolypolishError) as e:
            ctx.filter_files(ds["bams"][0], ds["bams"][1], outs[0], outs[1], out_bai=True)
        assert e.value.code == pp.ERR_ARG and "--out_bai needs --sort_out" in str(e.value)
        with pytest.raises(pp.PolypolishError) as e:
            ctx.filter_files(ds["sams"][0], ds["sams"][1], outs[0], outs[1], sort_out=True)
        assert e.value.code == pp.ERR_QUIT
    finally:
        ctx.close()
