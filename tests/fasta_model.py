"""A plain model of pp_fasta_records (polypolish_amd/csrc/pp_fasta.hip): load_fasta_not_gzipped + check_load_fasta (src/misc.rs:102-133,
56-75) as pp_assembly_load restates them, this project's deviations included -- a byte >= 0x80 in a sequence line that is valid UTF-8 is
a LIMIT refusal, and a '\\r' that is the text's last byte is dropped like one in front of a '\\n'.  One loop over the lines, nothing clever:

    parse(text) -> (names, descriptions, offsets, bases)     lists of bytes, a list of ints (n + 1), bytes
                   or raises FastaError(code, bad_line, words): bad_line the 0-based index among ALL lines (None behind the walk), words
                   the message with the path cut out of it

tests/test_fasta_model_cpu.py pins it to pp_assembly_load and to the oracle's loader; tests/test_fasta_records_gpu.py holds the device
against it."""

QUIT, LIMIT = 1, 5

# char::is_whitespace: the Unicode White_Space property
WHITE_SPACE = [0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) + [0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
_WS = [chr(c).encode("utf-8") for c in WHITE_SPACE]

NOT_FORMATTED = "is not correctly formatted"
UNABLE = "unable to load"
NOT_ASCII = "contains a non-ASCII byte in a sequence line (not supported by this implementation)"
NO_SEQUENCES = "contains no sequences"
EMPTY_SEQUENCE = "has an empty sequence"
DUPLICATED = "has a duplicated name"


class FastaError(Exception):
    def __init__(self, code, bad_line, words):
        super().__init__(f"{code} line {bad_line}: {words}")
        self.code, self.bad_line, self.words = code, bad_line, words


def lines_of(text):
    """BufRead::lines() as the loader's LineReader: split at '\\n', no line behind a final newline, one '\\r' dropped at a line's end"""
    text = bytes(text)
    out = text.split(b"\n")
    if out and out[-1] == b"":
        out.pop()
    return [l[:-1] if l.endswith(b"\r") else l for l in out]


def valid_utf8(b):
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def split_header(line):
    """(name, description) of a header line (valid UTF-8, line[0] == '>'): text[1..].splitn(2, char::is_whitespace)"""
    i = 1
    while i < len(line):
        for w in _WS:
            if line.startswith(w, i):
                return line[1:i], line[i + len(w):]
        i += 1
    return line[1:], b""


def parse(text):
    names, descs, offsets, bases = [], [], [0], bytearray()
    name, desc = b"", b""

    def push():
        names.append(name)
        descs.append(desc)
        offsets.append(len(bases))

    for li, line in enumerate(lines_of(text)):
        if not line:
            continue
        if line[0] == 0x3E:
            if not valid_utf8(line):
                raise FastaError(QUIT, li, UNABLE)
            if name:
                push()
            name, desc = split_header(line)
        else:
            if not name:
                raise FastaError(QUIT, li, UNABLE if not valid_utf8(line) else NOT_FORMATTED)
            if any(c >= 0x80 for c in line):
                raise FastaError(QUIT, li, UNABLE) if not valid_utf8(line) else FastaError(LIMIT, li, NOT_ASCII)
            bases += line.upper()  # (ASCII here: make_ascii_uppercase)
    if name:
        push()
    if not names:
        raise FastaError(QUIT, None, NO_SEQUENCES)
    for i in range(len(names)):
        if offsets[i + 1] == offsets[i]:
            raise FastaError(QUIT, None, EMPTY_SEQUENCE)
    if len(set(names)) != len(names):
        raise FastaError(QUIT, None, DUPLICATED)
    return names, descs, offsets, bytes(bases)


def words_of(message, path):
    """a loader's message with the quoted path cut out: what FastaError.words holds"""
    return message.replace('"' + path + '"', "").strip()


# ---- the generated texts both test files share -------------------------------------------------------------------------------------
def _ws_cases():
    out = {}
    for cp in WHITE_SPACE:
        if cp in (0x0A, 0x0D):
            continue  # (a line end: cases of their own below)
        w = chr(cp).encode("utf-8")
        out[f"ws_{cp:04x}_behind_name"] = b">c" + w + b"first" + w + b"second\nACGT\n"
        out[f"ws_{cp:04x}_behind_gt"] = b">" + w + b"unnamed\n>d x\nAC\n"
        out[f"r_ws_{cp:04x}_behind_gt_then_bases"] = b">" + w + b"unnamed\nAC\n"
    return out


CASES = {
    "lf": b">a one\nACGT\nacgt\n>b\nTTTT\n",
    "crlf": b">a one\r\nACGT\r\nacgt\r\n>b\r\nTTTT\r\n",
    "no_final_newline": b">a\nACGT\n>b\nTT",
    "cr_inside_a_line": b">a\nAC\rGT\nAA\n",
    "cr_first_in_a_line": b">a\n\rACGT\n",
    "two_cr_at_a_line_end": b">a\nACGT\r\r\n",
    "cr_last_byte_no_newline": b">a\nACGT\r",
    "cr_alone_last_line": b">a\nACGT\n\r",
    "cr_in_header": b">a x\ry\r\nAC\n",
    "empty_lines": b"\n\n>a\n\n\nAC\n\r\n\n\nGT\n\n>b\n\nA\n\n\n",
    "lower_and_iupac": b">a\nacgtnryswkmbvdh\nACGTNRYSWKMBVDH.-?*\n",
    "blanks_inside": b">a\nAC GT\t\n  \n x\n",
    "unnamed_before_header": b">\n>a\nAC\n> only a description\n>b\nGT\n",
    "unnamed_at_end": b">a\nAC\n>\n",
    "unnamed_at_end_with_description": b">a\nAC\n> d",
    "gt_only_last_byte": b">a\nAC\n>",
    "description_keeps_blanks": b">a  two  blanks \nAC\n",
    "header_nbsp_c2_at_line_end": b">a\xc2\xa0\nAC\n",
    "gt_inside_sequence": b">a\nAC>GT\n",
    "name_not_whitespace": ">n\u200bx\u00ad y\nAC\n".encode("utf-8"),
    # ---- refusals ----
    "r_empty_text": b"",
    "r_only_newlines": b"\n\n\r\n",
    "r_no_header": b"ACGT\n",
    "r_no_header_after_empty": b"\n\nACGT\n>a\nAC\n",
    "r_bases_behind_unnamed": b">a\nAC\n>\nGT\n",
    "r_bases_behind_unnamed_ws": b">a\nAC\n> x\nGT\n",
    "r_header_not_utf8": b">a\xff\nAC\n",
    "r_header_truncated_utf8": b">a\nAC\n>b\xe2\x80\nAC\n",
    "r_sequence_not_utf8": b">a\nAC\xffGT\n",
    "r_sequence_non_ascii": b">a\nAC\xc3\xa9GT\n",
    "r_headless_not_utf8": b"AC\xff\n",
    "r_headless_non_ascii": b"AC\xc3\xa9\n",
    "r_only_headers_named": b">a\n>b\n",
    "r_only_unnamed": b">\n> x\n",
    "r_empty_sequence_first": b">a\n>b\nAC\n",
    "r_empty_sequence_last": b">a\nAC\n>b\n",
    "r_empty_sequence_cr_only": b">a\n\r\n>b\nAC\n",
    "r_duplicate": b">a x\nAC\n>b\nGT\n>a y\nTT\n",
    "r_empty_then_duplicate": b">a\nAC\n>a\n",
    # ---- two refusals in one text: the earlier line wins ----
    "r_non_ascii_then_bad_header": b">a\nA\xc3\xa9\n>b\xff\nAC\n",
    "r_bad_header_then_non_ascii": b">a\xff\nA\xc3\xa9\n",
    "r_headless_then_non_ascii": b"AC\n>a\nA\xc3\xa9\n",
    "r_non_ascii_then_headless": b">a\nA\xc3\xa9\n>\nAC\n",
    "r_not_utf8_then_limit": b">a\nA\xff\nA\xc3\xa9\n",
    "r_limit_then_not_utf8": b">a\nA\xc3\xa9\nA\xff\n",
    "r_bad_header_then_headless": b">\xff\nAC\n",
    "r_line_refusal_before_duplicate": b">a\nAC\n>a\nA\xc3\xa9\n",
}
CASES.update(_ws_cases())
