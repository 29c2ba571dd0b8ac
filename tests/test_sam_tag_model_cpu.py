"""The model of the SAM-text write side (tests/sam_tag_model.py) pinned in two ways, without a device: to pp_filter_write_text, the host
routine that defines pp_sam_tagged's bytes (the library loads without a GPU), on hand-built texts -- every line ending and last-line
form, empty lines, "@" lines, no tab, FLAGs that do not parse or sit at the edge of u32, FLAG & 4 set and clear, a line already tagged,
bytes >= 0x80, the empty text, a wrong n_pass and its sentence --, and to the oracle's `filter` on the small dataset of
tests/test_bam_tag_model_cpu.py with the verdicts of the filter's own model (tests/filter_records_model.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import filter_records_model as frm
import gate_model as gm
import names_model as nm
import polypolish_amd as pp
import sam_tag_model as sm


def host_write(tmp_path, text, pass_):
    """pp_filter_write_text -> (rc, the file's bytes, (passed, failed), the error text)"""
    out = os.path.join(str(tmp_path), "host_out.sam")
    v = np.ascontiguousarray(pass_ if pass_ is not None else [], dtype=np.uint8)
    ok, bad, err = C.c_uint64(), C.c_uint64(), C.create_string_buffer(600)
    rc = pp.lib().pp_filter_write_text(text, len(text), v.ctypes.data if len(v) else None, len(v), out.encode(), C.byref(ok), C.byref(bad), err, 600)
    return rc, open(out, "rb").read(), (ok.value, bad.value), err.value.decode()


def same_as_host(tmp_path, text, pass_):
    rc, got, counts, err = host_write(tmp_path, text, pass_)
    assert rc == 0, err
    want, n_ok, n_fail, n_lines = sm.tagged(text, pass_)
    assert got == want, (text[:80], got[:80], want[:80])
    assert counts == (n_ok, n_fail)
    assert n_lines == want.count(b"\n")
    return want


def verdict_sets(n, seed=0):
    rng = np.random.default_rng(seed + n)
    return [np.ones(n, np.uint8), np.zeros(n, np.uint8), (np.arange(n) % 2).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8)]


def test_the_vocabulary_says_what_the_model_says():
    assert len(sm.VOCABULARY) >= 30 and {al for _, al in sm.VOCABULARY} == {True, False}
    for line, al in sm.VOCABULARY:
        assert b"\n" not in line and sm.aligned(line) == al, line


@pytest.mark.parametrize("k", range(len(sm.VOCABULARY)), ids=lambda k: f"line{k}")
def test_every_line_of_the_vocabulary_with_every_ending_and_as_the_last_line(tmp_path, k):
    line, al = sm.VOCABULARY[k]
    other = sm.record(name=b"other")
    for ending in (b"\n", b"\r\n", b"", b"\r"):                  # the last two: a last line without a newline
        for text in (line + ending, other + b"\n" + line + ending, line + ending + (other + b"\n" if b"\n" in ending else b"")):
            n = sm.n_aligned(text)
            if line and not line.endswith(b"\r"):                # (an empty last line is no line; the line's own "\r" may be the one dropped)
                assert line in sm.contents(text) and n == (1 if al else 0) + text.count(b"other")
            for v in verdict_sets(n):
                assert same_as_host(tmp_path, text, v)[-1:] in (b"", b"\n")


def test_line_endings_and_last_line_forms(tmp_path):
    r = sm.record()
    cases = {b"": b"", b"\n": b"\n", b"\n\n\n": b"\n\n\n", b"\r\n": b"\n", b"\r": b"\n", b"\r\r": b"\r\n", b"\r\r\n": b"\r\n", b"\n\r": b"\n\n",
             r: r + b"\n", r + b"\r": r + b"\n", r + b"\r\n": r + b"\n", r + b"\n\n" + r: r + b"\n\n" + r + b"\n",
             b"@HD\tVN:1\r\n\r\n" + r + b"\r": b"@HD\tVN:1\n\n" + r + b"\n"}
    for text, want in cases.items():
        assert same_as_host(tmp_path, text, np.ones(sm.n_aligned(text), np.uint8)) == want, text
    assert sm.tagged(b"", None) == (b"", 0, 0, 0) and sm.tagged(b"\n\n", None) == (b"\n\n", 0, 0, 2)
    assert sm.tagged(r + b"\r", [0]) == (r + sm.TAG + b"\n", 0, 1, 1)
    assert same_as_host(tmp_path, r + sm.TAG + b"\r\n" + r, [0, 1]) == r + sm.TAG + sm.TAG + b"\n" + r + b"\n", "a second tag"


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mixed_texts(tmp_path, seed):
    text, n = sm.mixed_text(700, seed)
    assert n == sm.n_aligned(text) and 100 < n < 650 and b"\r\n" in text and any(b >= 0x80 for b in text)
    for v in verdict_sets(n, seed):
        same_as_host(tmp_path, text, v)
    same_as_host(tmp_path, text + b"\n", np.ones(n, np.uint8))


def test_a_wrong_number_of_verdicts_and_its_sentence(tmp_path):
    text, n = sm.mixed_text(50, 9)
    for k in (n - 1, n + 1, 0):
        rc, _, _, err = host_write(tmp_path, text, np.ones(k, np.uint8))
        assert rc == pp.ERR_ARG and err == f"{k} verdicts for {n} aligned records"
        with pytest.raises(sm.TagError) as e:
            sm.tagged(text, np.ones(k, np.uint8))
        assert str(e.value) == err
    rc, _, _, err = host_write(tmp_path, b"", [1])
    assert rc == pp.ERR_ARG and err == "1 verdicts for 0 aligned records"


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, orc):
    import synth
    d = str(tmp_path_factory.mktemp("sam_tag_model"))
    ds = synth.rich_dataset(d, seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    outs = [os.path.join(d, f"filtered_{i}.sam") for i in (1, 2)]
    orc.filter_files(ds["sam1"], ds["sam2"], outs[0], outs[1])
    return {"sams": [ds["sam1"], ds["sam2"]], "outs": outs, "contigs": [(c.name, c.assembly) for c in ds["contigs"]]}


def model_verdicts(contigs, texts):
    """the filter model's verdicts for the two texts: their records decoded by the gate's model, the QNAMEs interned in one table"""
    table, raws = {}, []
    for text in texts:
        raw, _ = gm.raw_from_text(contigs, text)
        raw["read_id"] = np.array(nm.ids(table, nm.sam_column(text, 0, aligned_only=False)), np.uint64)
        raws.append(raw)
    return frm.command(raws)["pass"]


def test_the_oracle_s_filter_writes_tagged_of_the_model_s_verdicts(dataset):
    texts = [open(p, "rb").read() for p in dataset["sams"]]
    verdicts = model_verdicts(dataset["contigs"], texts)
    some_failed = some_came_tagged = False
    for text, out, v in zip(texts, dataset["outs"], verdicts):
        want, n_ok, n_fail, _ = sm.tagged(text, v)
        assert want == open(out, "rb").read()
        assert (n_ok, n_fail) == (int(np.sum(v != 0)), int(np.sum(v == 0)))
        some_failed |= n_fail > 0
        some_came_tagged |= sm.TAG in text
    assert some_failed and some_came_tagged
