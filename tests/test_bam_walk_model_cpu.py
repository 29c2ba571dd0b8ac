"""tests/bam_walk_model.py -- the plain model of the device walk over the BAM block_size chain -- pinned to bam_model.walk: on a few
hundred seeded layouts at small chunk, zone and group sizes (records of 36 bytes up to three chunks and more, junk leads, truncations,
planted block sizes below 32, any start), and on the hand-built inputs of tests/test_bam_walk_gpu.py at the library's own geometry,
where it also says that each input takes the path it was built for.  No GPU."""
import numpy as np
import pytest

import bam_model as bm
import bam_walk_model as wm


def agree(b, start, C, Z, G):
    want_off, want_end, ok = bm.walk(b, start)
    n_rec, end, kind, off, stats = wm.walk(b, start, C, Z, G)
    assert (kind == wm.OK) == ok and n_rec == len(want_off) and end == want_end, (n_rec, len(want_off), end, want_end, kind)
    if ok:
        assert off == want_off
        assert stats[wm.CHAIN] == (0 if start == len(b) else (len(b) + C - 1) // C - start // C)
        assert stats[wm.CHAIN] == stats[wm.ZONE] + stats[wm.SLOW] + stats[wm.PASS] + (start < len(b))
    else:
        assert off is None
    return kind, stats


@pytest.mark.parametrize("C,Z,G", ((64, 32, 2), (128, 64, 3), (256, 32, 4), (4096, 1024, 2)))
def test_seeded_layouts(C, Z, G):
    rng = np.random.default_rng(C + Z + G)
    seen = np.zeros(4, np.int64)
    for _ in range(80):
        lens = [int(rng.choice([36, 37, 40, 63, 64, 65, 100, 300, C - 1, C, C + 1, 3 * C + 5, G * C + 40])) for _ in range(int(rng.integers(0, 60)))]
        lead = int(rng.integers(0, 3 * C))
        b = bytearray(wm.junk(lead, rng) + b"".join(wm.rec(max(36, ln), int(rng.integers(0, 256))) for ln in lens))
        mode = int(rng.integers(0, 4))
        if mode == 1 and len(b) > lead:
            del b[-int(rng.integers(1, min(40, len(b) - lead) + 1)):]
        if mode == 2 and lens:
            at = lead + sum(max(36, ln) for ln in lens[:int(rng.integers(0, len(lens)))])
            b[at:at + 4] = int(rng.integers(0, 32)).to_bytes(4, "little")
        seen += agree(bytes(b), lead, C, Z, G)[1]
        agree(bytes(b), int(rng.integers(0, len(b) + 2)), C, Z, G)
    assert (seen > 0).all(), seen      # zone, slow path and pass-through all met


def geometry():
    """the library's chunk, zone and group sizes where it is built, else the ones it is written with"""
    try:
        import polypolish_amd as pp
        return pp.bam_walk_geometry()
    except (ImportError, OSError, AttributeError):
        return 16384, 1024, 64


def test_hand_built_inputs_take_their_paths():
    C, Z, G = geometry()
    for name, b, start, check in wm.cases(C, Z, G):
        kind, stats = agree(b, start, C, Z, G)
        assert kind == wm.OK, name
        assert check is None or check(stats), (name, stats)


def test_planted_breaks_are_found_where_they_are_planted():
    C, Z, G = geometry()
    for name, b, start, kind, check, at in wm.breaks(C, Z, G):
        n_rec, end, got, off, stats = wm.walk(b, start, C, Z, G)
        assert (got, end) == (kind, at), (name, got, end, at)
        assert agree(b, start, C, Z, G)[0] == kind
        assert check is None or check(stats), (name, stats)


def test_ordinary_records_never_leave_the_fast_path():
    C, Z, G = geometry()
    b = ordinary(C, G)
    kind, stats = agree(b, 0, C, Z, G)
    assert kind == wm.OK and stats[wm.CHAIN] > 2 * G and stats[wm.SLOW] == 0
    assert stats[wm.ZONE] == stats[wm.CHAIN] - 1 - stats[wm.PASS]


def ordinary(C, G):
    """bm.mixed_records() back to back, as often as it takes to reach into the third group"""
    body = bm.lay_out(bm.mixed_records(n=3000))[0]
    return body * (2 * G * C // len(body) + 1) + body[:0]


def test_tiny_inputs():
    for n, kind in ((0, wm.OK), (1, wm.CUT), (3, wm.CUT), (4, wm.PAST), (35, wm.PAST), (36, wm.OK)):
        assert agree(wm.rec(36)[:n], 0, *geometry())[0] == kind
    assert wm.walk(b"", 1)[2] == wm.START and wm.walk(wm.rec(40), 41)[:3] == (0, 41, wm.START)
