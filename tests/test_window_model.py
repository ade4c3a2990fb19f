"""The needed-rectangle rule of the window decode (include/icer_hip_dec_window.h, tests/window_model.py) is SUFFICIENT: with
the packets of every chain the rule drops deleted from the stream, the decoder oracle's image still equals the full decode
inside the window.  All seven filters, 1 to 4 stages, 1 / 3 / 8 segments, 16 and 8 bit, odd sizes (the odd lines of an 8-bit
decoder among them) from 33 x 17 to 160 x 121; windows: interior, every edge and corner, single pixels, the whole image,
straddling the border, wholly outside.  CPU only."""
import numpy as np
import pytest

from oracle.binding import Oracle
from tests import reduced_cases as rc_
from tests import window_model as wm
from tests.decoder_batch_cases import oracle_decode
from tests.recon_model import dim_high, dim_low

SIZES = [(33, 17), (64, 48), (97, 99), (131, 70), (160, 121)]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def sizes_for(stages, segments, pick):
    """two of SIZES whose deepest LL is at least 3 wide and whose smallest subband holds `segments` samples, chosen by `pick`"""
    ok = [(w, h) for w, h in SIZES if min(dim_low(w, stages), dim_low(h, stages)) >= 3 and dim_high(w, stages) * dim_high(h, stages) >= 2 * segments]
    assert ok, (stages, segments)
    return [ok[pick % len(ok)], ok[(pick + 2) % len(ok)]]


def check_rule(orc, w, h, ch, stages, filt, segments, bits, seed=1):
    """-> (windows checked, chains dropped in all)"""
    stream = rc_.encode(orc, rc_.planes(w, h, ch, seed, bits), stages, filt, segments, None, bits)
    full = oracle_decode(orc, stream, ch, stages, filt, segments, w * h, bits)
    assert full[:3] == (0, w, h)
    table = wm.chain_table(orc, stream, ch, stages, segments, bits, w, h)
    checked = dropped = 0
    for win in wm.windows_for(w, h):
        x0, y0, ww, wh = c = wm.clip(win, w, h)
        keep = wm.kept(table, w, h, stages, c, filt, bits)
        if ww * wh == 0:
            assert keep == [], (win, "an empty window needs nothing")
            continue
        assert keep, win
        got = oracle_decode(orc, wm.strip(stream, keep, ch), ch, stages, filt, segments, w * h, bits)
        assert got[:3] == (0, w, h), (win, got[:3])
        for p, q in zip(got[3], full[3]):
            a, b = (v[: w * h].reshape(h, w)[y0: y0 + wh, x0: x0 + ww] for v in (p, q))
            assert np.array_equal(a, b), f"{w}x{h} filt {filt} stages {stages} segments {segments} bits {bits} window {win}: {np.count_nonzero(a != b)} samples differ"
        checked += 1
        dropped += len(table) - len(keep)
    return checked, dropped


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("segments", [1, 3, 8])
@pytest.mark.parametrize("stages", [1, 2, 3, 4])
@pytest.mark.parametrize("filt", range(7))
def test_rule_is_sufficient(orc, filt, stages, segments, bits):
    checked = dropped = 0
    for w, h in sizes_for(stages, segments, filt + stages):
        a, b = check_rule(orc, w, h, 1, stages, filt, segments, bits)
        checked, dropped = checked + a, dropped + b
    assert checked >= 24
    if segments > 1 and bits == 16:              # (an 8-bit decoder takes its odd lines whole: an odd-sized image may need every chain)
        assert dropped > 0, "no window dropped a chain: the case shows nothing"


@pytest.mark.parametrize("filt,bits,w,h", [(0, 16, 97, 99), (2, 16, 97, 99), (6, 8, 96, 100)])     # (8 bit: even, or every line is whole)
def test_rule_is_sufficient_yuv(orc, filt, bits, w, h):
    checked, dropped = check_rule(orc, w, h, 3, 3, filt, 3, bits)
    assert checked >= 12 and dropped > 0


def test_the_rule_itself():
    """the table of the header, on lines where it can be read off by hand"""
    # filter A, n = 20 (nl = nh = 10), samples [6, 9): pairs 3 .. 4 -> highs [3, 4], lows [2, 5]
    assert wm.axis(20, 6, 9, True, 16) == ((2, 6), (3, 5))
    # ... the last sample of an odd line (n = 21, nl = 11, nh = 10): the last low and its neighbour, no high
    assert wm.axis(21, 20, 21, True, 16) == ((9, 11), (0, 0))
    # the other filters: to the end of the line
    assert wm.axis(20, 6, 9, False, 16) == ((1, 10), (3, 10))
    # whole: short lines, and the odd lines of an 8-bit decoder
    assert wm.axis(7, 2, 3, True, 16) == ((0, 4), (0, 3)) and wm.axis(21, 2, 3, True, 8) == ((0, 11), (0, 10))
    assert wm.axis(20, 5, 5, True, 16) == ((0, 0), (0, 0))
    assert wm.clip((5, 6, 100, 2), 40, 30) == (5, 6, 35, 2) and wm.clip((40, 0, 3, 3), 40, 30) == (40, 0, 0, 0)
