"""tests/names_model.py -- the plain model of pp_names -- pinned to what the library already does on the host: the read numbers of
pp_filter_load are "the ranks of the first record of each name" over file 1 then file 2, which is the model's rule, and a table
seeded with the contig names gives the RNAME ids pp_filter_records asks for.  No GPU."""
import numpy as np

import gate_model as gm
import names_model as nm
import synth


def test_the_model_numbers_reads_as_the_host_loader_does(tmp_path):
    import polypolish_amd as pp
    ds = synth.rich_dataset(str(tmp_path), seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3)
    loaded = pp.FilterLoaded(ds["sam1"], ds["sam2"])
    try:
        state = {}
        for f, path in enumerate((ds["sam1"], ds["sam2"])):
            names = nm.sam_column(open(path, "rb").read())
            want = loaded.files[f]["read"]
            assert len(names) == len(want) > 1000
            got = np.array(nm.ids(state, names), np.uint32)
            assert np.array_equal(got, want), (f, np.flatnonzero(got != want)[:8])      # exact, file 2 included: no partition needed
        assert len(state) == loaded.n_reads
        # the two files share most names and each has some of its own (unaligned mates): file 2's numbering is not file 1's shifted
        only2 = set(nm.sam_column(open(ds["sam2"], "rb").read())) - set(nm.sam_column(open(ds["sam1"], "rb").read()))
        assert 0 < len(only2) < loaded.n_reads // 2
    finally:
        loaded.close()


CONTIGS = [("contig_1", "ACGT" * 50), ("contig_2", "TTGA" * 50)]


def _line(qname, rname, pos):
    return f"{qname}\t0\t{rname}\t{pos}\t60\t20M\t*\t0\t0\t{'ACGT' * 5}\t*\tNM:i:0"


def test_a_table_seeded_with_the_contigs_tells_unknown_references_apart():
    text = ("@HD\tVN:1.6\n" + "\n".join([_line("r0", "contig_2", 5), _line("r1", "plasmid_A", 9), _line("r2", "contig_1", 1),
                                        _line("r3", "plasmid_B", 9), _line("r4", "plasmid_A", 30), _line("r5", "contig_2", 40)]) + "\n").encode()
    n_contigs = len(CONTIGS)
    state = {}
    assert nm.ids(state, [name.encode() for name, _ in CONTIGS]) == list(range(n_contigs))
    rnames = nm.sam_column(text, column=2)
    got = nm.ids(state, rnames)
    raw, _ = gm.raw_from_text(CONTIGS, text)
    known = raw["contig"] != gm.NO_CONTIG
    assert known.tolist() == [True, False, True, False, False, True]
    assert np.array_equal(np.array(got)[known], raw["contig"][known]) and max(np.array(got)[known]) < n_contigs
    a, b = got[1], got[3]
    assert a != b and a >= n_contigs and b >= n_contigs and got[4] == a
    # the trap the table removes: one shared "no contig" value makes the two unknown references compare equal
    assert raw["contig"][1] == raw["contig"][3] == gm.NO_CONTIG


def test_the_empty_qname_rule_groups_as_raw_from_text_does():
    qn = ["a", "", "b", "b", "", "", "c", "b", "", "b", "d", "d"]
    flags = [0, 0, 0, 256, 0, 4, 0, 0, 0, 0, 4, 0]
    text = ("\n".join(f"{q}\t{f}\tcontig_1\t{3 + i}\t60\t20M\t*\t0\t0\t{'ACGT' * 5}\t*\tNM:i:0" for i, (q, f) in enumerate(zip(qn, flags))) + "\n").encode()
    raw, _ = gm.raw_from_text(CONTIGS, text)
    ids = np.array(nm.ids({}, [q.encode() for q in qn]), np.uint64)
    mine = dict(raw, read_id=nm.empty_qname_rule(ids, qn, raw["flag"]))
    assert gm.groups(mine) == gm.groups(raw) and len(gm.groups(raw)) < len(gm.groups(dict(raw, read_id=ids)))
    plain = ["a", "b", "b", "c"]                                # no empty name: nothing changes
    assert np.array_equal(nm.empty_qname_rule(np.array([0, 1, 1, 2], np.uint64), plain, np.zeros(4, np.uint16)), [0, 1, 1, 2])


def test_the_case_builders_hold_what_their_names_say():
    call, quads, pairs = nm.seam_case()
    names = nm.names_of(call)
    assert {int(o) & 7 for o in call[1]} == set(range(8)) and len(quads) == 8 * len(nm.SEAM_LENS)
    for i1, i2, i3, i4 in quads:
        assert names[i1] == names[i2] and (int(call[1][i1]) - int(call[1][i2])) & 7
        end1, end2 = int(call[1][i1]) + len(names[i1]), int(call[1][i2]) + len(names[i2])
        assert call[0][end1] != call[0][end2]                   # different bytes behind the two copies
        if i3 is not None:
            assert names[i3][:-1] == names[i1][:-1] and names[i3] != names[i1] and names[i4] == names[i1][:-1]
    for (i, j), k in zip(pairs, nm.PAIR_BYTES * 2):
        assert [x != y for x, y in zip(names[i], names[j])] == [q == k for q in range(16)]
    assert len(set(nm.order_case())) == 1200 and len(nm.order_case()) == 5000
    assert len({n for c in nm.growth_calls() for n in c}) == 20000
    assert nm.names_of(nm.shifted(call, 3)) == names
    call, want = nm.numbered_case(3000, 700)
    assert nm.ids({}, nm.names_of(call)) == want.tolist() and int(want.max()) < 700 and nm.names_of(call)[0][:1] == b"r"
