"""CPU: pins tests/bam_tag_model.py, the model the device's pp_bam_tagged is held against byte for byte (tests/test_bam_tagged_gpu.py,
tests/test_bam_tag_chain_gpu.py): frame() against zlib's own level-0 blocks where zlib writes ONE stored block, every block of a framed
file through the BGZF model, tagged() against the oracle's filter on the dataset of tests/test_bgzf_chain_gpu.py, and the records of
U' field for field through the BAM model."""
import os

import numpy as np
import pytest

import bam_model as bm
import bam_tag_model as tm
import bgzf_model as zm
import filter_model as fm

U_LENS = (0, 1, tm.PAYLOAD - 1, tm.PAYLOAD, tm.PAYLOAD + 1, 2 * tm.PAYLOAD - 1, 2 * tm.PAYLOAD, 2 * tm.PAYLOAD + 1)


@pytest.mark.parametrize("n", (1, 12))
def test_frame_is_zlib_s_level_0_block_where_zlib_writes_one_stored_block(n):
    d = zm.noise(n, seed=n)
    assert tm.stored_block(d) == zm.block(d, 0)
    assert tm.frame(d) == zm.block(d, 0) + zm.EOF_BLOCK


def test_frame_of_nothing_is_the_eof_block():
    assert tm.frame(b"") == zm.EOF_BLOCK and len(zm.EOF_BLOCK) == 28


@pytest.mark.parametrize("u_len,fail_last", [(n, f) for n in U_LENS for f in (False, True) if n > 1 or not f])
def test_every_block_of_a_framed_stream_inflates_to_its_piece(u_len, fail_last):
    data, at, off, passed = tm.stream_of(u_len, fail_last)
    u = tm.tagged(data, at, off, passed)
    assert len(u) == u_len
    f = tm.frame(u)
    n_blocks = (u_len + tm.PAYLOAD - 1) // tm.PAYLOAD
    assert len(f) == u_len + 31 * n_blocks + 28
    blk, out, end, ok = zm.walk(f)
    assert ok and end == len(f) and blk == tm.blk_off(n_blocks, len(f)).tolist()
    for b, o in enumerate(blk[:-1]):
        assert zm.inflate_block(f, o) == u[b * tm.PAYLOAD:(b + 1) * tm.PAYLOAD]
        total, _, pay_len, _, isize = zm.unwrap(f, o)
        assert total == isize + 31 and pay_len == isize + 5, "one stored block"
    assert zm.inflate_block(f, blk[-1]) == b"" and tm.unframe(f) == u


def mixed_input(n=600, seed=5):
    """records of every kind with a header in front, verdicts at random: (bytes, records_at, rec_off, passed)"""
    recs = bm.mixed_records(n, seed)
    body, off = bm.lay_out(recs)
    n_al = sum(1 for r in recs if not r[18] & 4)
    passed = (np.random.default_rng(seed).random(n_al) < 0.6).astype(np.uint8)
    return tm.HEADER + body, len(tm.HEADER), off + np.uint64(len(tm.HEADER)), passed


def test_every_field_of_u_is_the_input_s_and_zp_is_cleared_where_the_verdict_or_the_input_says_so():
    data, at, off, passed = mixed_input()
    u = tm.tagged(data, at, off, passed)
    assert bm.header(u)["records_at"] == at and u[:at] == data[:at]
    got_off, end, ok = bm.walk(u, at)
    assert ok and end == len(u) and len(got_off) == len(off)
    want, got = bm.decode(data, off), bm.decode(u, got_off)
    assert (want["zp"] == 0).any() and (passed == 0).any() and ((want["zp"] == 0) & (passed == 0)).any()
    assert np.array_equal(got["zp"], want["zp"] & passed)
    keys = [k for k in bm.KEYS if k != "name_off"]      # (the names move with their records)
    bm.same(got, want, keys)
    names = lambda b, d: [bytes(b[int(o):int(o) + int(k)]) for o, k in zip(d["name_off"], d["name_len"])]      # noqa: E731
    assert names(u, got) == names(data, want)
    # a failing record grew by exactly the eight bytes, every other one kept its length
    lens = np.diff(np.array(got_off + [end]))
    al = (want["flag"] & 4) == 0
    grew = np.zeros(len(off), np.int64)
    grew[al] = 8 * (passed == 0)
    assert np.array_equal(lens, np.array([4 + tm._le32(data, int(o)) for o in off]) + grew)


def test_subsets_duplicates_and_unaligned_records():
    data, at, off, _ = mixed_input(60, 9)
    pick = np.concatenate([off[::-1][:20], off[5:6], off[5:6]])
    n_al = sum(1 for o in pick if not data[int(o) + 18] & 4)
    u = tm.tagged(data, at, pick, np.zeros(n_al, np.uint8))
    got_off, end, ok = bm.walk(u, at)
    assert ok and len(got_off) == len(pick)
    for g, o in zip(got_off, pick):
        o, bs = int(o), tm._le32(data, int(o))
        if data[o + 18] & 4:
            assert u[g:g + 4 + bs] == data[o:o + 4 + bs]
        else:
            assert u[g + 4:g + 4 + bs] == data[o + 4:o + 4 + bs] and u[g + 4 + bs:g + 12 + bs] == tm.TAG and tm._le32(u, g) == bs + 8


def test_the_model_refuses_what_the_contract_refuses():
    data, at, off, passed = mixed_input(20, 2)
    for kind, o in ((tm.CUT, len(data) + 1), (tm.CUT, len(data) - 3), (tm.PAST, int(off[-1])), (tm.SMALL, int(off[-1]))):
        bad = bytearray(data)
        if kind == tm.PAST:
            bad = bad[:-1]
        if kind == tm.SMALL:
            bad[o:o + 4] = (31).to_bytes(4, "little")
        with pytest.raises(tm.TagError) as e:
            tm.tagged(bytes(bad), at, np.concatenate([off[:2], [o], off[2:4], [o]]).astype(np.uint64), passed)
        assert (e.value.code, e.value.kind, e.value.bad_record) == (tm.ARG, kind, 2), kind
    with pytest.raises(tm.TagError) as e:
        tm.tagged(data, at, off, passed[:-1])
    assert e.value.kind == "n_pass"
    with pytest.raises(tm.TagError):
        tm.tagged(data, len(data) + 1, off[:0], None)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, orc):
    import synth
    d = str(tmp_path_factory.mktemp("bam_tag_model"))
    ds = synth.rich_dataset(d, seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    outs = [os.path.join(d, f"filtered_{i}.sam") for i in (1, 2)]
    orc.filter_files(ds["sam1"], ds["sam2"], outs[0], outs[1])
    return {"sams": [ds["sam1"], ds["sam2"]], "outs": outs, "contigs": [(c.name, len(c.assembly)) for c in ds["contigs"]]}


def test_tagged_equals_the_encoding_of_the_oracle_s_filtered_files(dataset):
    names = [n for n, _ in dataset["contigs"]][::-1]
    lens = [k for _, k in dataset["contigs"]][::-1]
    some_failed = some_came_tagged = False
    for sam, out in zip(dataset["sams"], dataset["outs"]):
        text, filtered = open(sam, "rb").read(), open(out, "rb").read()
        enc, want = bm.encode(text, names, lens), bm.encode(filtered, names, lens)
        verdicts = tm.own_verdicts(text, filtered)
        # (a line that came with ZP:Z:fail and passes keeps its one tag: failed_lines cannot tell it from one the filter failed)
        assert ((verdicts == 0) <= (fm.failed_lines(filtered) == 0)).all()
        some_failed |= bool((verdicts == 0).any())
        some_came_tagged |= bool(((verdicts == 1) & (fm.failed_lines(filtered) == 0)).any())
        u = tm.tagged(enc["header"] + enc["records"], len(enc["header"]), enc["rec_off"] + np.uint64(len(enc["header"])), verdicts)
        assert u == want["header"] + want["records"]
        assert tm.unframe(tm.frame(u)) == u
    assert some_failed and some_came_tagged
