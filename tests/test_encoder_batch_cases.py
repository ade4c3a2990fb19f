"""The frame kinds of tests/encoder_batch_cases.py reach the paths their names promise, in the oracle and, where the reference
build exists, with the reference's own streams: the GPU batch tests that use them stay inside the parity claim and cannot
quietly turn into trivial content."""
import numpy as np
import pytest

from tests import encoder_batch_cases as ebc
from tests.test_oracle_decoder import packets

GEOMS = [ebc.Geometry(64, 48, 1, 2, f, 3) for f in (0, 2, 5)] + [ebc.Geometry(96, 80, 1, 3, f, 4) for f in (1, 6)]
LOSSLESS = lambda g: ebc.quota(g, "lossless")


def magnitudes(planes):
    return [p.astype(np.uint32) & 0x7FFF for p in planes]


@pytest.mark.parametrize("g", GEOMS, ids=str)
def test_sixteen_bit_kinds_take_their_paths(oracle, g):
    exp = ebc.Expected(oracle)
    q = LOSSLESS(g)
    for seed in (0, 1):
        r = {k: exp(g, (k, seed), q) for k in ebc.KINDS16}
        for k in ebc.CODED16:
            assert r[k][0] == 0, (k, r[k][0])
        # overflow: the transform itself leaves int16
        planes = ebc.oracle_planes(g, ("overflow", seed))
        assert r["overflow"][0] == -1 and r["overflow"][1] == b""
        assert oracle.dwt(planes[0], g.stages, g.filt)[0] == -1
        # mean: the transform is fine, the LL mean check fails
        planes = ebc.oracle_planes(g, ("mean", seed))
        assert r["mean"][0] == -1 and r["mean"][1] == b""
        assert oracle.dwt(planes[0], g.stages, g.filt)[0] == 0
        # wide: coded, with coefficients above the ninth bit plane
        assert max(int(m.max()) for m in magnitudes(r["wide"][2])) >= 1 << 9
        for k in ("smooth", "dot", "flat"):
            assert max(int(m.max()) for m in magnitudes(r[k][2])) < 1 << 9, k
        # blank: one packet per coding unit ((3 stages + 1) subbands x segments x 9 planes), each a header and a few bytes
        pk = packets(r["blank"][1])
        assert len(pk) == (3 * g.stages + 1) * g.segments * 9 and all(28 < len(p) <= 28 + 8 for p in pk), [len(p) for p in pk[:9]]
        assert len(r["dot"][1]) > len(r["blank"][1])
        # sparse: about one sample in ten
        frac = np.count_nonzero(ebc.oracle_planes(g, ("sparse", seed))[0]) / (g.w * g.h)
        assert 0.06 < frac < 0.14, frac
    # a blank frame codes alike under every filter
    assert r["blank"][1] == ebc.Expected(oracle)(g._replace(filt=(g.filt + 1) % 7), ("blank", 1), q)[1]


def test_yuv_kinds_take_their_paths(oracle):
    g = ebc.Geometry(64, 48, 3, 2, 0, 3)
    exp = ebc.Expected(oracle)
    q = LOSSLESS(g)
    for kind in ebc.CODED16:
        assert exp(g, (kind, 0), q)[0] == 0, kind
    for kind in ebc.ABORTED16:
        assert exp(g, (kind, 0), q)[:2] == (-1, b""), kind
    # one channel overflows, the others would be coded: the frame is aborted
    for spec in ((("smooth", "overflow", "smooth"), 0), (("blank", "blank", "mean"), 0)):
        assert exp(g, spec, q)[:2] == (-1, b""), spec
    planes = ebc.oracle_planes(g, (("smooth", "overflow", "smooth"), 0))
    assert [oracle.dwt(p, g.stages, g.filt)[0] for p in planes] == [0, -1, 0]


@pytest.mark.parametrize("g", [ebc.Geometry(64, 48, 1, 2, 0, 3, bits=8), ebc.Geometry(96, 80, 3, 3, 0, 4, bits=8)], ids=str)
def test_uint8_kinds_take_their_paths(oracle, g):
    exp = ebc.Expected(oracle)
    q = LOSSLESS(g)
    for kind in ("blank8", "noise6", "smooth6"):
        assert exp(g, (kind, 0), q)[0] == 0, kind
    assert exp(g, ("full8", 0), q)[:2] == (-1, b"")


def test_front_end_inputs_are_coded(oracle):
    exp = ebc.Expected(oracle)
    for g, kinds in ((ebc.Geometry(64, 48, 1, 2, 0, 3, raw="gray8"), ebc.RAW_GRAY), (ebc.Geometry(64, 48, 3, 2, 0, 3, raw="rgb8"), ebc.RAW_RGB)):
        streams = set()
        for kind in kinds:
            rc, stream, _ = exp(g, (kind, 0), LOSSLESS(g))
            assert rc == 0, (g.raw, kind)
            streams.add(stream)
        assert len(streams) == len(kinds)              # four different inputs, four different streams
    white = ebc.oracle_planes(ebc.Geometry(8, 8, 3, raw="rgb8"), ("white", 0))
    assert [int(p[0, 0]) for p in white] == [255, 128, 128]


def test_quota_classes():
    g = ebc.Geometry(256, 192)
    S = g.w * g.h
    assert ebc.quota(g, "cut") >= S // 2 > ebc.quota(g, "progressive")          # (progressive mode: quota < w * h * C / 2)
    assert [ebc.quota(g, c) for c in ("tiny27", "tiny28", "tiny60")] == [27, 28, 60]


CASES_VS_REF = [(ebc.Geometry(64, 48, 1, 2, 0, 3), ebc.KINDS16), (ebc.Geometry(96, 80, 1, 3, 5, 4), ebc.KINDS16),
                (ebc.Geometry(64, 48, 3, 2, 2, 3), ebc.KINDS16 + (("smooth", "overflow", "smooth"), ("blank", "blank", "mean"))),
                (ebc.Geometry(64, 48, 1, 2, 0, 3, bits=8), ebc.KINDS8), (ebc.Geometry(96, 80, 3, 3, 1, 4, bits=8), ebc.KINDS8),
                (ebc.Geometry(64, 48, 1, 2, 0, 3, raw="gray8"), ebc.RAW_GRAY), (ebc.Geometry(64, 48, 3, 2, 0, 3, raw="rgb8"), ebc.RAW_RGB)]


@pytest.mark.parametrize("g,kinds", CASES_VS_REF, ids=[str(c[0]) for c in CASES_VS_REF])
def test_kinds_give_the_reference_builds_streams(oracle, reference, g, kinds):
    exp = ebc.Expected(oracle)
    if g.bits == 16 and not g.raw:              # the reference's own stages transform: overflows on `overflow`, not on `mean`
        assert reference.dwt(ebc.oracle_planes(g, ("overflow", 0))[0], g.stages, g.filt)[0] == -1
        assert reference.dwt(ebc.oracle_planes(g, ("mean", 0))[0], g.stages, g.filt)[0] == 0
    for kind in kinds:
        for cls in ("lossless", "cut", "progressive", "tiny60"):
            q = ebc.quota(g, cls)
            planes = ebc.oracle_planes(g, (kind, 0))
            fn = reference.compress_u8 if g.bits == 8 else reference.compress
            rc, stream, _ = fn(planes, g.stages, g.filt, g.segments, q)
            want = exp(g, (kind, 0), q)
            assert (rc, stream) == want[:2], (kind, cls, rc, want[0], len(stream), len(want[1]))
