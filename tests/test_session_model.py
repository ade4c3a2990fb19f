"""tests/session_model.py on the fixtures of tests/test_combine_model.py and tests/test_recut_mock.py, CPU only: nested quota
cuts fed as increments (made with tests/combine_model.py), and an ROI cut followed by a quota cut.  After every step the model
delivers what the decoder decodes from the corresponding union stream -- the decoder oracle, and the reference's own decoder
where it is built."""
import numpy as np
import pytest

from tests import combine_model as cm
from tests import roi_cases as rc
from tests import session_model as sm
from tests.decoder_batch_cases import oracle_decode
from tests.sweep_cut_cases import reads_on
from tests.test_combine_model import CLASSES, model_of, moved_viewport, nested_frames
from tests.test_recut_mock import GEOMETRIES, expected          # noqa: F401  (expected: fixture)


def session(orc, g, **kw):
    return sm.SessionModel(orc, g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits, **kw)


def same(a, b):
    return a[:3] == b[:3] and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))


def decode(orc, g, stream):
    return oracle_decode(orc, stream, g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits)


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_nested_cuts_fed_as_increments(expected, oracle, name):
    g, specs = GEOMETRIES[name]
    m = model_of(g)
    checked = 0
    for spec, streams in nested_frames(expected, g, specs):
        if any(reads_on(oracle, g, s, 0) for s in streams):     # (what any decoder makes of such packets depends on what follows each)
            continue
        mod = session(oracle, g)
        held = b""
        for i, cut in enumerate(streams):
            inc = cm.combine(m, held, cut, cm.DIFFERENCE)[1] if held else cut
            got = mod.feed(0, inc)
            assert same(got, decode(oracle, g, cut)), (name, spec, CLASSES[i])
            assert cm.units(m, mod.stream_of(0)) == cm.units(m, cut)
            held = cut
        assert mod.dropped == 0 and mod.decoded == len(cm.units(m, streams[-1]))
        # a duplicate changes nothing and is dropped whole; an increment alone (no chain holds its top planes) is dropped too
        before = mod.decode(0)
        assert same(mod.feed(0, streams[1]), before) and mod.dropped == len(cm.units(m, streams[1]))
        fresh = session(oracle, g)
        inc = cm.combine(m, streams[0], streams[1], cm.DIFFERENCE)[1]
        fresh.feed(0, inc)
        kept = cm.units(m, fresh.stream_of(0))
        assert kept < cm.units(m, inc), "an increment alone was accepted whole"
        checked += 1
    assert checked, "every frame of this geometry reads on"


@pytest.mark.parametrize("name", ["G1", "G2", "G3", "G4"])
def test_roi_cut_then_quota_cut(expected, oracle, name):
    g = rc.GEOMETRIES[name]
    m, H, W = moved_viewport(expected, name)
    inc = cm.combine(m, H, W, cm.DIFFERENCE)[1]
    union = cm.combine(m, H, W, cm.UNION)[1]
    mod = session(oracle, g)
    assert same(mod.feed(0, H), decode(oracle, g, H)), name
    got = mod.feed(0, inc)
    assert cm.units(m, mod.stream_of(0)) == cm.units(m, union), name
    assert same(got, decode(oracle, g, union)) and same(got, decode(oracle, g, H + inc)), name
    assert mod.dropped == 0


def test_refusals_and_the_size_of_an_empty_slot(expected, oracle):
    g, specs = GEOMETRIES["gray16"]
    g2, specs2 = GEOMETRIES["gray8"]
    _, streams = nested_frames(expected, g, specs)[0]
    mod = session(oracle, g)
    assert mod.feed(0, b"", 9, 7)[1:3] == (9, 7)                  # (no packet yet: the caller's values)
    got = mod.feed(0, streams[0])
    assert got[:3] == (0, g.w, g.h)
    other = expected(g2, specs2[0], 1 << 20)[1]
    assert mod.feed(0, other) == (sm.INVALID_INPUT, g.w, g.h, None) and same(mod.decode(0), got)
    small = sm.SessionModel(oracle, g.channels, g.stages, g.filt, g.segments, g.w * g.h - 1, g.bits)
    assert small.feed(0, streams[0]) == (sm.QUOTA, g.w, g.h, None) and not small.slots[0].T


def test_against_the_reference_decoder(expected, oracle, reference):
    g, specs = GEOMETRIES["gray16"]
    m = model_of(g)
    spec, streams = next((s, x) for s, x in nested_frames(expected, g, specs) if not any(reads_on(oracle, g, c, 0) for c in x))
    mod = session(oracle, g)
    got = mod.feed(0, streams[0])
    got = mod.feed(0, cm.combine(m, streams[0], streams[1], cm.DIFFERENCE)[1])
    ref = reference.decompress_raw(streams[1], g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits)
    assert same(got, ref), spec
