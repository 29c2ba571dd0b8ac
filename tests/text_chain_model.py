"""What pp_sam_records_lines and pp_sam_first_empty_line (pp_sam.hip) are held against: the first n lines of a SAM text as bytes, and
the first empty line, both on the line splitting of tests/ingest_model.py (line_spans: a line ends at its "\\n", a last line without one
at the end of the text; a "\\r" in front of the "\\n" belongs to the line's end).  tests/test_text_chain_model_cpu.py pins both to
ingest_model._lines."""
import ingest_model as im


def prefix(text, n_lines):
    """the bytes of the first n_lines lines, line ends included: what pp_sam_records_lines decodes.  n_lines at or beyond the line
    count: the text itself."""
    starts, _ = im.line_spans(text)
    if n_lines >= len(starts):
        return bytes(text)
    return bytes(text[:int(starts[n_lines])])


def first_empty_line(text):
    """the 0-based index of the first line without a byte, or with "\\r" only; None when there is none"""
    starts, ends = im.line_spans(text)
    for i, (s, e) in enumerate(zip(starts.tolist(), ends.tolist())):
        if text[s:e] in (b"", b"\r"):
            return i
    return None


def n_lines(text):
    return len(im.line_spans(text)[0])
