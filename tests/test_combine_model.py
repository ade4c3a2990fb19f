"""The rule of icerx_combine_device_async (tests/combine_model.py) on the oracle's streams, CPU only: what a server sends to a
client that holds cut H and wants cut W (the difference), what the client then holds (H followed by the increment, or the
union), and that the decoder oracle reads both as the wanted stream.

  nested cuts      H < W of one frame at the quota classes progressive < cut < lossless: union(H, difference(H, W)) is W byte for
                   byte, the increment is exactly len(W) - len(H) > 0 bytes, H + increment decodes as W does
  moved viewport   two ROI cuts of one frame with different rectangles: each side has units the other lacks, the union holds the
                   units of both without a hole in any family, H + increment decodes as the union does
  damage           a payload byte flipped in one packet of H: the difference additionally holds exactly that unit's packet of W"""
import numpy as np
import pytest

from tests import combine_model as cm
from tests import encoder_batch_cases as ebc
from tests import reduced_model as red
from tests import roi_cases as rc
from tests import roi_model as rm
from tests import target_model as tm
from tests.decoder_batch_cases import oracle_decode
from tests.sweep_cut_cases import reads_on
from tests.test_recut_mock import GEOMETRIES, QUOTA_EXCEEDED, expected          # noqa: F401  (expected: fixture)

CLASSES = ("progressive", "cut", "lossless")


def model_of(g):
    return tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments, g.bits)


def nested_frames(expected, g, specs):
    """the frames of a batch that every quota below the lossless one cuts, so that the three streams differ: [(spec, [stream
    per class])]"""
    out = []
    for s in specs:
        res = [expected(g, s, ebc.quota(g, c)) for c in CLASSES]
        if [r[0] for r in res] == [QUOTA_EXCEEDED, QUOTA_EXCEEDED, 0]:
            out.append((s, [r[1] for r in res]))
    assert out, "no frame of this batch is cut at both quotas"
    return out


def decode(oracle, g, stream):
    code, w, h, planes = oracle_decode(oracle, stream, g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits)
    return code, w, h, [p.tobytes() for p in planes]


def moved_viewport(expected, name):
    """(model, held, wanted): the ROI cuts of the first frame of batch 0 at samples // 4 and shift 3, rectangle kinds `segment`
    and `border`"""
    g, m = rc.GEOMETRIES[name], rc.model(name)
    lossless = expected(g, rc.BATCHES[name][0][0], rc.quotas(name)[0])
    assert lossless[0] == 0
    held, wanted = (rm.roi_stream(m, lossless[1], rc.rectangle(m, kind), 3, g.samples // 4)[0] for kind in ("segment", "border"))
    return m, held, wanted


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_nested_cuts(expected, oracle, name):
    g, specs = GEOMETRIES[name]
    m = model_of(g)
    decoded = 0
    for spec, streams in nested_frames(expected, g, specs):
        for X in streams:
            assert cm.combine(m, X, X, cm.UNION)[:2] == (0, X), (name, spec)
            assert cm.combine(m, X, X, cm.DIFFERENCE) == (0, b"", 0, 0), (name, spec)
            assert cm.combine(m, b"", X, cm.DIFFERENCE)[:2] == (0, X), (name, spec)
        for i in range(len(streams)):
            for j in range(i + 1, len(streams)):
                H, W = streams[i], streams[j]
                tag = (name, spec, CLASSES[i], CLASSES[j])
                assert cm.units(m, H) < cm.units(m, W), tag
                code, inc, packets, from_a = cm.combine(m, H, W, cm.DIFFERENCE)
                assert (code, from_a) == (0, 0) and packets == len(cm.units(m, W)) - len(cm.units(m, H)), tag
                assert 0 < len(inc) == len(W) - len(H), tag
                code, union, packets, from_a = cm.combine(m, H, inc, cm.UNION)
                assert code == 0 and union == W, (tag, ebc.first_difference(union, W))
                assert (packets, from_a) == (len(cm.units(m, W)), len(cm.units(m, H))), tag
                # (the documented exception of tests/reduced_model.py: where a chain of W reads on into the bytes behind its
                # packet, what a decoder makes of W depends on the order of the packets; the bytes of the increment do not)
                if reads_on(oracle, g, W, 0):
                    continue
                decoded += 1
                want = decode(oracle, g, W)
                assert want[:3] == (0, g.w, g.h) and decode(oracle, g, H + inc) == want, tag
    assert decoded, "no pair of this geometry went through the decoder"


@pytest.mark.parametrize("name", ["G1", "G2", "G3", "G4"])
def test_moved_viewport(expected, oracle, name):
    g = rc.GEOMETRIES[name]
    m, H, W = moved_viewport(expected, name)
    uh, uw = cm.units(m, H), cm.units(m, W)
    assert uh - uw and uw - uh, (name, len(uh), len(uw))
    if name == "G4":
        assert (len(uh), len(uw), len(uw - uh), len(uh - uw)) == (412, 409, 102, 105)
    code, inc, packets, from_a = cm.combine(m, H, W, cm.DIFFERENCE)
    assert (code, packets, from_a) == (0, len(uw - uh), 0) and cm.units(m, inc) == uw - uh, name
    code, union, packets, from_a = cm.combine(m, H, W, cm.UNION)
    assert (code, packets, from_a) == (0, len(uh | uw), len(uh - uw)) and cm.units(m, union) == uh | uw, name
    assert cm.combine(m, H, inc, cm.UNION)[:2] == (0, union), name
    assert rm.kept_planes_are_top_runs(m, union), f"{name}: a hole in a family of the union"
    want = decode(oracle, g, union)
    assert want[:3] == (0, g.w, g.h) and decode(oracle, g, H + inc) == want, name


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_a_damaged_copy_gets_its_packet_again(expected, name):
    g, specs = GEOMETRIES[name]
    m = model_of(g)
    spec, (_, H, W) = nested_frames(expected, g, specs)[0]
    level = max(red.levels_of(H))
    hurt = red.flip_in_packet(H, level, False, which=1)
    (unit,) = cm.units(m, H) - cm.units(m, hurt)
    plain, again = cm.combine(m, H, W, cm.DIFFERENCE), cm.combine(m, hurt, W, cm.DIFFERENCE)
    assert again[0] == 0 and again[2] == plain[2] + 1 and cm.units(m, again[1]) == cm.units(m, plain[1]) | {unit}, (name, spec)
    packet = cm.table(m, W)[0][unit]
    assert cm.table(m, again[1])[0][unit] == packet and len(again[1]) == len(plain[1]) + len(packet), (name, spec)
    # the client appends the increment behind its damaged copy: the union of the two is the wanted stream
    assert cm.combine(m, hurt, again[1], cm.UNION)[:2] == (0, W), (name, spec)


def test_statuses():
    g, _ = GEOMETRIES["gray16"]
    m = model_of(g)
    junk = np.random.default_rng(1).integers(0, 256, 500).astype(np.uint8).tobytes()
    for op in (cm.UNION, cm.DIFFERENCE):
        assert cm.combine(m, b"", junk, op) == (cm.OUT_OF_DATA, b"", 0, 0)
        assert cm.combine(m, b"", b"", op, inside=False) == (cm.INVALID_INPUT, b"", 0, 0)
