"""A plain model of pp_batch_regroup (include/polypolish_hip.h): "the raw records of one file -> the same records with every read's
records brought together".  Test infrastructure: tests/test_regroup_model_cpu.py pins it to gate_model / ingest_model and to the
oracle on a coordinate-sorted dataset, tests/test_regroup_gpu.py runs the device link (pp_regroup.hip) against it.  It does not call
the library.

perm is the stable order of the records by the index of the first record with the same read_id; the same rule on SAM lines
(regroup_text, by QNAME) is what a name-grouped file of those records looks like, and sort_coordinate is what `samtools sort` makes
of a file."""
import numpy as np

PER_RECORD = ("flag", "read_id", "contig", "ref_start", "nm", "seq_off", "seq_len", "cig_off", "n_cig")


def first_occurrence(keys):
    """rep[i] = the index of the first record whose key equals record i's"""
    keys = np.asarray(keys)
    if not len(keys):
        return np.zeros(0, np.int64)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    return first[inverse.reshape(-1)].astype(np.int64)


def perm(read_id):
    """output record j is raw record perm[j]: groups in the order of their first record, file order inside a group"""
    return np.argsort(first_occurrence(np.asarray(read_id, np.uint64)), kind="stable").astype(np.uint32)


def regroup(raw):
    """-> {"raw": the nine per-record arrays gathered through perm, seq and cigar as they are; "perm"; "counts": (distinct read_ids,
    records that changed place)}"""
    p = perm(raw["read_id"])
    out = {k: np.ascontiguousarray(np.asarray(raw[k])[p]) for k in PER_RECORD}
    out["seq"], out["cigar"] = raw["seq"], raw["cigar"]
    n_groups = len(np.unique(np.asarray(raw["read_id"], np.uint64)))
    return {"raw": out, "perm": p, "counts": (n_groups, int((p != np.arange(len(p), dtype=np.uint32)).sum()))}


def carry_pass(flag, p, passed):
    """one byte per ALIGNED record of the raw batch -> the same verdicts in the numbering of the regrouped batch"""
    aligned = (np.asarray(flag) & 4) == 0
    rank = np.cumsum(aligned) - aligned                 # aligned rank of every raw record
    took = p[aligned[p]]                                # the raw records behind the regrouped batch's aligned records, in its order
    return np.asarray(passed, np.uint8)[rank[took]]


def _split(text):
    """(header lines, record lines) of SAM bytes, each line without its end"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    lines = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]
    return [ln for ln in lines if not ln or ln[:1] == b"@"], [ln for ln in lines if ln and ln[:1] != b"@"]


def regroup_text(text):
    """the header, then the record lines in the order of perm over their QNAMEs; -> (bytes, the lines' perm)"""
    head, recs = _split(text)
    names = np.array([ln.split(b"\t", 1)[0] for ln in recs], dtype=object)
    ids = {}
    p = perm(np.array([ids.setdefault(n, len(ids)) for n in names], np.uint64))
    return b"".join(ln + b"\n" for ln in head + [recs[i] for i in p.tolist()]), p


def sort_coordinate(text, contig_order):
    """the header, then the record lines stable by (contig, POS); records with FLAG & 4 or RNAME * last, in file order"""
    head, recs = _split(text)
    index = {n.encode() if isinstance(n, str) else n: i for i, n in enumerate(contig_order)}

    def key(ln):
        f = ln.split(b"\t", 4)
        if int(f[1]) & 4 or f[2] == b"*":
            return (len(index) + 1, 0)
        return (index.get(f[2], len(index)), int(f[3]))
    return b"".join(ln + b"\n" for ln in head + sorted(recs, key=key))


def same_raw(got, want):
    """the nine per-record arrays byte for byte"""
    for k in PER_RECORD:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (k, a[:8], b[:8])


def sorted_dataset(d):
    """The dataset of the BAM chain tests (tests/test_bam_chain_gpu.py), each SAM coordinate-sorted: {"fasta", "contigs", "sams": the
    name-grouped originals, "sorted" / "regrouped": per file the sorted text and regroup_text of it (bytes), "sorted_paths" /
    "regrouped_paths": the same as files under d, "moved": per file the perm of the sorted lines}"""
    import os

    import synth
    ds = synth.rich_dataset(d, seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    contigs = [(c.name, c.assembly) for c in ds["contigs"]]
    out = {"fasta": ds["fasta"], "contigs": contigs, "sams": [ds["sam1"], ds["sam2"]], "sorted": [], "regrouped": [], "sorted_paths": [],
           "regrouped_paths": [], "moved": []}
    for f, path in enumerate(out["sams"]):
        text = sort_coordinate(open(path, "rb").read(), [name for name, _ in contigs])
        again, p = regroup_text(text)
        for kind, data in (("sorted", text), ("regrouped", again)):
            out[kind].append(data)
            out[kind + "_paths"].append(os.path.join(d, f"{kind}_{f + 1}.sam"))
            with open(out[kind + "_paths"][-1], "wb") as fh:
                fh.write(data)
        out["moved"].append(p)
    return out
