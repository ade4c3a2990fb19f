"""What the region-of-interest encode, the two re-cuts by resolution and the reduced and display decodes are asked for over the
sample of tests/geometry_sweep_cases.py (icerx_encode_device_roi, icerx_recut_device_cuts_async, icerx_recut_device_roi_async,
icerx_decoder_create_reduced, the display decode), shared by tests/test_geometry_sweep_cuts.py (CPU) and
tests/test_gpu_geometry_sweep_cuts.py.  Nothing here runs on a device, and nothing here is a definition: the expected values
come from tests/roi_model.py, tests/reduced_model.py (derive, expected), model_cuts / scaled_rect of
tests/test_recut_roi_mock.py, tests/display_model.py and the two oracles.

For the case of index i in the sample, (g, specs):

  rectangles   one per frame, roi_cases.rectangle: frames 0, 1, 2 get `segment`, `border`, `last`; every second case (odd i)
               is rotated by 3 and gets `outside`, `empty`, `full`, so that all six kinds occur over the sample.
  shifts       0, 3, 16 -- one icerx_encode_device_roi call each.
  ROI quotas   the lossless quota, half and a fifth of the longest lossless stream of the batch, and 28.
  cuts         one list for the cuts call (reduce, quota) and the ROI re-cut (reduce, quota, shift): every r in 0 .. stages - 1
               with a generous quota (above the longest derive(M, r)) and half of it at shift 0 and at shift 3.  The generous cut
               keeps every unit whatever the order, so its shift, 16, only has to be survived.  Six stages would make 18 cuts
               and a call takes 16: there the two coarsest r lose the half at shift 0 and their generous cut takes shift 0.
  conditions   non-vacuity, stated on the models alone (depends_on_rectangle): with the `last` rectangle -- one pixel, the
               kind that leaves most units in the background however small the reduced image -- frame 0's lossless stream cut
               at half the length of derive(M, r) differs between shift 3 and shift 0, and the foreground is a proper part:
               more than the LL units, fewer than all.  At r = 0 that holds in every geometry of more than one
               segment (MIN_R0 of them in the sample), at r >= 1 in at least MIN_REDUCED of the (geometry, r) pairs.  A seed
               that misses them is replaced; the conditions stay.
  decodes      r in {0, 1, stages - 1}, each distinct r once; the display decode at r = stages - 1.  SweepBatch holds what the
               decoder oracle gives for derive(M, r).  One exception, the one include/icer_hip_dec.h makes for the reduced
               decode: a chain whose packets do not decode within their own payloads (12-bit content, the `wide` kind) reads on
               into the bytes that follow, and those differ between M and derive(M, r).  reads_on finds such frames with the
               decoder oracle alone; a decoder made with reduce = r >= 1 owes them the oracle's rc and size and no samples.
               The decode of a re-cut's output, which is derive(M, r) byte for byte, owes every frame everything.

No case and no r is left out.  Under quirk P1 (three geometries of the sample) the plan of the geometry at 1/2^r size does not
always have the rectangles the payloads were coded with; the reduced plan's rectangles decide foreground, as the definition
says (a reduce-0 call of a plain recutter for the geometry at 1/2^r size on derive(M, r)), and the decoder oracle ends such a
stream with ICER_TOO_MANY_SEGMENTS (-3) at every r, the words decoded so far left in place: that is the expected value."""
from __future__ import annotations

import functools

import numpy as np

from tests import encoder_batch_cases as ebc
from tests import geometry_sweep_cases as gsc
from tests import reduced_cases as rc_
from tests import reduced_model as red
from tests import roi_cases as rc
from tests import target_model as tm

SHIFTS = (0, 3, 16)
MAX_CUTS = 16                                                         # ICERX_MAX_LADDER
GENEROUS_SHIFT = 16
MIN_R0 = 26                                                           # geometries of more than one segment in the sample
MIN_REDUCED = 50                                                      # of the 56 (geometry, r >= 1) pairs
TOO_MANY_SEGMENTS = -3


def model_of(g: ebc.Geometry) -> tm.Model:
    return tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments, g.bits)


def reduced_geometry(g: ebc.Geometry, r: int) -> ebc.Geometry:
    w, h = red.reduced_size(g.w, g.h, r)
    return g._replace(w=w, h=h, stages=g.stages - r)


@functools.lru_cache(maxsize=None)
def models(g: ebc.Geometry):
    """the model of the geometry at 1/2^r size for every r in 0 .. stages - 1 (tm.Refused would be a case left out: none is)"""
    return tuple(model_of(reduced_geometry(g, r)) for r in range(g.stages))


def n_ll(m: tm.Model) -> int:
    return sum(u[2] == tm.LL for u in m.units)


def rect_kinds(index: int):
    first = 2 + 3 * (index % 2)
    return [rc.RECT_KINDS[(first + f) % len(rc.RECT_KINDS)] for f in range(3)]


def rectangles(index: int, g: ebc.Geometry):
    """(x, y, w, h) per frame"""
    return [rc.rectangle(models(g)[0], k) for k in rect_kinds(index)]


def condition_rectangle(g: ebc.Geometry):
    return rc.rectangle(models(g)[0], "last")


def identity(g: ebc.Geometry, kind: str, shift: int, n_fg: int, n_units: int) -> bool:
    """the ROI order is the priority order: the stream is the plain call's"""
    return shift == 0 or kind in ("empty", "outside") or n_fg == n_units or g.segments == 1


def roi_quotas(g: ebc.Geometry, lossless_streams):
    top = max(len(s) for s in lossless_streams)
    return [ebc.quota(g, "lossless"), top // 2, top // 5, 28]


@functools.lru_cache(maxsize=4)
def _derived(streams: tuple, stages: int):
    return tuple(tuple(red.derive(s, r) for s in streams) for r in range(stages))


def derived_masters(g: ebc.Geometry, streams):
    """[r][f] = derive(M_f, r) for every r in 0 .. stages - 1 (remembered for the case at hand)"""
    return _derived(tuple(streams), g.stages)


def cuts(g: ebc.Geometry, lossless_streams):
    """[(reduce, quota, shift)] of the ROI re-cut; the cuts call takes the same list without the shifts"""
    out = []
    spare = MAX_CUTS - 3 * g.stages
    derived = derived_masters(g, lossless_streams)
    for r in range(g.stages):
        top = max(len(d) for d in derived[r])
        if spare < 0 and r >= g.stages + spare:                       # (six stages: the two coarsest r)
            out += [(r, top + 9, 0), (r, top // 2, 3)]
        else:
            out += [(r, top + 9, GENEROUS_SHIFT), (r, top // 2, 0), (r, top // 2, 3)]
    assert len(out) <= MAX_CUTS and {c[0] for c in out} == set(range(g.stages))
    return out


def generous(cut_list):
    """{r: index of the generous cut at r} (the first cut of every r)"""
    out = {}
    for i, c in enumerate(cut_list):
        out.setdefault(c[0], i)
    return out


def model_of_cuts(g: ebc.Geometry, streams, rects, cut_list):
    """(want[c][f] = (rc, stream, K, foreground units), derived[r][f] = derive(M_f, r)): model_cuts on derive(M, r) with the
    model of the geometry at 1/2^r size and the scaled rectangle -- plain integers on the host, no recutter"""
    from tests.test_recut_roi_mock import model_cuts, scaled_rect
    derived = derived_masters(g, streams)
    want = [[None] * len(streams) for _ in cut_list]
    for r, shift in sorted({(c[0], c[2]) for c in cut_list}):
        idx = [k for k, c in enumerate(cut_list) if (c[0], c[2]) == (r, shift)]
        for f in range(len(streams)):
            res = model_cuts(models(g)[r], derived[r][f], scaled_rect(rects[f], g.w, g.h, r), shift, [cut_list[k][1] for k in idx])
            for k, w in zip(idx, res):
                want[k][f] = w
    return want, derived


def decode_reduces(g: ebc.Geometry):
    return sorted({0, min(1, g.stages - 1), g.stages - 1})


def reads_on(orc, g: ebc.Geometry, derived: bytes, r: int) -> bool:
    """some chain of derive(M, r) does not decode within its own payloads: the decoder oracle's result changes with the bytes
    put behind every packet (the packet walk steps over them)"""
    from tests.decoder_batch_cases import oracle_decode
    rw, rh = red.reduced_size(g.w, g.h, r)
    packets = [derived[o: o + n] for o, n in red.walk(derived)]
    res = [oracle_decode(orc, b"".join(p + fill for p in packets), g.channels, g.stages - r, g.filt, g.segments, rw * rh, g.bits)
           for fill in (b"", b"\x00" * 16, b"\xff" * 16)]
    return not all(x[:3] == res[0][:3] and all(np.array_equal(a, b) for a, b in zip(x[3], res[0][3])) for x in res[1:])


class SweepBatch(rc_.ReducedBatch):
    """the masters of a case for a decoder made with (stages, reduce = r): want[k] is the decoder oracle on derive(M, r), the
    frame stride is the reduced image to the sample, exact[k] says whether frame k's samples are owed (see `decodes` above)"""

    def __init__(self, orc, g: ebc.Geometry, streams, r: int, from_masters=True):
        rw, rh = red.reduced_size(g.w, g.h, r)
        super().__init__(orc, g.channels, g.bits, g.filt, g.stages, g.segments, streams, r, rw * rh, [(g.w, g.h, "lossless")] * len(streams))
        code = TOO_MANY_SEGMENTS if gsc.is_p1(g) else 0
        assert [x[:3] for x in self.want] == [(code, rw, rh)] * len(streams), (gsc.case_id(g), r, [x[:3] for x in self.want])
        self.exact = [r == 0 or not from_masters or not reads_on(orc, g, red.derive(s, r), r) for s in streams]

    def check(self, rcs, ws, hs, frame, label=""):
        assert list(rcs) == self.rcs(), (label, list(rcs), self.rcs())
        for k, (_, w, h, planes) in enumerate(self.want):
            assert (ws[k], hs[k]) == (w, h), (label, k, ws[k], hs[k], w, h)
            for c in range(self.channels if self.exact[k] else 0):
                got = np.asarray(frame(k, c))[: w * h]
                if not np.array_equal(got, planes[c][: w * h]):
                    bad = np.flatnonzero(got != planes[c][: w * h])
                    raise AssertionError(f"{label}: frame {k} channel {c}: {bad.size} samples differ from the decoder oracle's, first at "
                                         f"{bad[0]} ({got[bad[0]]} != {planes[c][bad[0]]})")


def check_display(b: SweepBatch, got, plain, junk, label=""):
    """got = (rcs, ws, hs, rows) of a display call into junk-filled rows, plain = (rcs, ws, hs, frame(k, c)) of the plain call of
    the same decoder: the same rcs and sizes; every image is tests/display_model.py of the plain call's planes and, where the
    samples are owed, of the decoder oracle's; nothing behind an image"""
    from tests.display_model import display_of
    rcs, ws, hs, rows = got
    assert (list(rcs), list(ws), list(hs)) == (list(plain[0]), list(plain[1]), list(plain[2])), label
    b.check(rcs, ws, hs, plain[3], label)
    ch = b.channels
    for k, (_, w, h, planes) in enumerate(b.want):
        image, rest = rows[k][: ch * w * h], rows[k][ch * w * h:]
        assert (rest == junk).all(), (label, k, "written behind the image")
        assert np.array_equal(image, display_of([plain[3](k, c)[: w * h] for c in range(ch)], ch).reshape(-1)), (label, k, "the plain call")
        if b.exact[k]:
            assert np.array_equal(image, display_of([p[: w * h] for p in planes], ch).reshape(-1)), (label, k, "the decoder oracle")


def depends_on_rectangle(g: ebc.Geometry, r: int, lossless0: bytes) -> bool:
    """the non-vacuity condition at r, on the model alone"""
    from tests.test_recut_roi_mock import model_cuts, scaled_rect
    m = models(g)[r]
    derived = red.derive(lossless0, r)
    rect = scaled_rect(condition_rectangle(g), g.w, g.h, r)
    (a,), (b,) = (model_cuts(m, derived, rect, s, [len(derived) // 2]) for s in (0, 3))
    return a[1] != b[1] and n_ll(m) < b[3] < m.n_units


def check_conditions(lossless0_of):
    """lossless0_of(g, spec) -> frame 0's lossless oracle stream.  Returns (geometries that meet the condition at r = 0,
    (geometry, r >= 1) pairs that meet it, pairs in all) after asserting the conditions"""
    at0, reduced, pairs = [], 0, 0
    for g, specs in gsc.cases():
        s = lossless0_of(g, specs[0])
        if depends_on_rectangle(g, 0, s):
            at0.append(g)
        for r in range(1, g.stages):
            pairs += 1
            reduced += depends_on_rectangle(g, r, s)
    several = [g for g, _ in gsc.cases() if g.segments > 1]
    missing = [gsc.case_id(g) for g in several if g not in at0]
    assert not missing, f"no cut at r = 0 depends on the rectangle in {missing}"
    assert len(several) >= MIN_R0, len(several)
    assert reduced >= MIN_REDUCED, (reduced, pairs)
    return len(at0), reduced, pairs
