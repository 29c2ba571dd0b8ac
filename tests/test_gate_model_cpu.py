"""tests/gate_model.py -- the plain model of pp_batch_gate -- pinned to ingest_model.model(), the model of the text ingests:
gate(raw_from_text(t), passed = zp AND verdicts) is model(t), file by file, on every named case of ingest_model's table whose
lines all parse, and on the generated inputs of the GPU test -- whose shape (enough good and rejected records, "*" fills on both
strands, a group start on every listed rank) is asserted here, on the CPU, so that the GPU test checks what it says it does."""
import numpy as np
import pytest

import gate_model as gm
import ingest_model as im


@pytest.mark.parametrize("name", sorted(im.CASES))
def test_gate_of_the_raw_records_is_the_model_of_the_text(name):
    c = im.case(name)
    parsed = 0
    for f, text in enumerate(c.texts):
        want = gm.expect_from_model(c, f, None)
        try:
            raw, zp = gm.raw_from_text(c.contigs, text)
        except gm.NotRaw as e:
            # not a parse-clean file: the model must say so itself, with a defect of a line (or a value no raw batch holds)
            assert want[0] == "error" or e.args[0].startswith("value"), (name, f, want)
            continue
        parsed += 1
        passed = gm.passed_for(c, f, zp)
        try:
            got = gm.gate(raw, c.max_errors, c.careful, passed)
        except gm.GateError as e:
            if want[0] == "contig":   # the model stops at the unknown RNAME; the gate goes on to the wrong verdict count behind it
                assert e.kind == "verdict_count" and len(passed) != int(((raw["flag"] & 4) == 0).sum()), (name, f, e)
                continue
            assert want[0] == "error" and (e.code, e.kind) == (want[1], want[2]), (name, f, want, e)
            if e.kind != "verdict_count":
                first = gm.groups(raw)
                assert any(g[0] == e.bad_record for g in first)
            continue
        if want[0] == "contig":
            assert (got["recs"]["contig"] == gm.NO_CONTIG).any()
            continue
        if want[0] == "empty":
            assert got["counts"] == (0, 0, 0) and len(got["orig"]) == 0
            continue
        assert want[0] == "ok", (name, f, want)
        gm.same(got["recs"], want[1]["recs"])
        assert [got["counts"]] == [tuple(x) for x in want[1]["counts"]]
        al = np.flatnonzero((raw["flag"] & 4) == 0)
        assert np.isin(got["orig"], al).all() and (np.diff(got["orig"].astype(np.int64)) > 0).all()
    if c.error is None:
        assert parsed == len(c.texts), "a case that is meant to pass has lines that do not parse"


def test_the_first_failing_group_and_its_first_record():
    rng = np.random.default_rng(1)
    rows = [gm._row(rng, 10 + i) for i in range(30)]
    rows[7] = gm._row(rng, 17, flag=4, runs=[])
    rows[8] = gm._row(rng, 18, seq=b"", runs=[24 << 4])                  # group {8, 9}: no sequence
    rows[9] = gm._row(rng, 18, seq=b"", runs=[24 << 4], flag=256)
    rows[20] = gm._row(rng, 30, runs=[])                                  # empty CIGAR further down
    raw = gm.pack_raw(rows)
    with pytest.raises(gm.GateError) as e:
        gm.gate(raw)
    assert (e.value.code, e.value.kind, e.value.bad_record) == (im.QUIT, "no_sequence", 8)
    got = gm.gate(gm.pack_raw(rows[:20]), careful=True)                   # the same group under --careful is silent
    assert got["counts"] == (19, 17, 18)
    with pytest.raises(gm.GateError) as e:
        gm.gate(gm.pack_raw(rows[10:]))
    assert (e.value.code, e.value.kind, e.value.bad_record) == (im.PANIC, "empty_cigar", 10)


def test_reverse_complement_of_all_128_ascii_values():
    from oracle import pyref
    s = bytes(range(128))
    assert gm.revcomp_upper(s).decode() == pyref.reverse_complement(gm.upper(s).decode("latin-1"))


def _shape(rows, passed):
    raw = gm.pack_raw(rows)
    got = gm.gate(raw, 10, False, passed)
    grp = gm.groups(raw)
    al = {r: a for a, r in enumerate(r for g in grp for r in g)}
    good = set(got["orig"].tolist())
    fills = {(int(raw["flag"][r]) ^ int(raw["flag"][next(x for x in g if raw["seq_len"][x])])) & 16
             for g in grp for r in g if r in good and raw["seq_len"][r] == 0}
    return raw, got, {"good": len(good), "rejected": len(al) - len(good), "fills": fills, "starts": {al[g[0]] for g in grp}}


def test_the_generated_inputs_have_the_shape_the_gpu_test_relies_on():
    rows, passed = gm.seam_rows()
    raw, got, s = _shape(rows, passed)
    assert len(rows) <= 20_000 and s["good"] >= 200 and s["rejected"] >= 200
    assert s["fills"] == {0, 16}, "a '*' fill on the same and on the opposite strand"
    assert set(gm.START_RANKS) <= s["starts"]
    assert raw["flag"][0] & 4 and raw["flag"][len(rows) - 1] & 4, "unaligned records first and last"
    assert {1, 15, 16, 17, 31, 32, 33, 160} <= set(got["recs"]["seq_len"].tolist())
    assert int(raw["seq_off"][0]) % 2 == 1 and int((raw["seq_off"] + raw["seq_len"]).max()) == len(raw["seq"])
    rows = gm.big_group_rows()
    raw, got, s = _shape(rows, None)
    big = max(gm.groups(raw), key=len)
    assert len(big) == 3000 and [r for r in big if raw["seq_len"][r]] == [big[2500]]
    assert s["fills"] == {0, 16} and (got["recs"]["k"] == 2000).sum() == 2000
    assert big[0] // gm.GATE_BLOCK != big[-1] // gm.GATE_BLOCK
