"""The geometry sweep of the ROI encode, the re-cuts by resolution and by region and the reduced and display decodes, on the GPU
(tests/sweep_cut_cases.py over the sample of tests/geometry_sweep_cases.py: 1 to 6 stages, all seven filters, 1 to 32 segments,
gray and YUV, 16 and 8 bits, grids kept under quirk P1, 28 to 8 463 units).  Per geometry, three frames, one encoder and one
recutter made with max_reduce = stages - 1:

  masters      the encoder's lossless streams are the oracle's;
  ROI encode   icerx_encode_device_roi at shifts 0, 3, 16 with four quotas: every (rc, stream, K) and foreground count is
               roi_model.roi_streams of the master; shift 0, `empty`, `outside`, a foreground of every unit and one segment
               give the streams of separate icerx_encode_device calls; no unit timed out;
  re-cuts      every cut of icerx_recut_device_cuts_async and icerx_recut_device_roi_async is model_cuts on derive(M, r) with
               the model of the geometry at 1/2^r size and the scaled rectangle, computed on the host -- no second recutter;
               reduce-0 ROI cuts are the ROI encode's streams, shift-0 ROI cuts the cuts call's;
  decodes      the generous cut of every r goes into Decoder(stages - r).decode_torch without the host; the masters go through
               Decoder(reduce=r) at r in {1, stages - 1}; both give what the decoder oracle gives for derive(M, r) -- rc, size
               and every sample, rc -3 and the words decoded so far under quirk P1 (the reduced decode of 12-bit content that
               reads on behind its packets: sweep_cut_cases.SweepBatch); one display decode at r = stages - 1, packed RGB888 or
               gray8, against tests/display_model.py.
Every comparison is exact.  The helpers of tests/test_gpu_roi.py, test_gpu_recut_cuts.py and test_gpu_recut_roi.py check the
sentinel rows, the odd strides and that the inputs are left alone.  The CPU side is tests/test_geometry_sweep_cuts.py."""
import numpy as np
import pytest

from icer_compression_amd import decoder
from tests import encoder_batch_cases as ebc
from tests import geometry_sweep_cases as gsc
from tests import reduced_model as red
from tests import roi_model as rm
from tests import sweep_cut_cases as scc
from tests import test_gpu_display as tgd
from tests import test_gpu_ladder as tl
from tests import test_gpu_recut as tg
from tests import test_gpu_recut_cuts as tgc
from tests import test_gpu_recut_roi as tgo
from tests import test_gpu_reduced as tgx
from tests import test_gpu_roi as tgr
from tests.test_display_mock import JUNK
from tests.test_gpu_recut import expected, torch             # noqa: F401  (fixtures)
from tests.test_recut_cuts_mock import check_packets

pytestmark = pytest.mark.gpu

CASES = gsc.cases()


def check_roi_encode(enc, t, g, m, specs, streams, rects, kinds, what):
    """-> {(shift, quota index, frame): (rc, stream, K, foreground units)} of icerx_encode_device_roi, checked against roi_model"""
    quotas = scc.roi_quotas(g, streams)
    plain = {q: tl.separate(enc, t, q) for q in sorted(set(quotas))}
    rois = tgr.rois_tensor(rects, t.device)
    out = {}
    for shift in scc.SHIFTS:
        got, fg = tgr.roi_call(enc, t, rois, shift, quotas)
        for f, spec in enumerate(specs):
            tag = f"{what} ROI encode: shift {shift} frame {f} {spec} rectangle {rects[f]} ({kinds[f]})"
            want, n_fg = rm.roi_streams(m, streams[f], rects[f], shift, quotas)
            assert fg[f] == n_fg, (tag, fg[f], n_fg)
            for q, quota in enumerate(quotas):
                code, stream, K = got[q][f]
                w_stream, w_code, w_K = want[q]
                assert (code, K, len(stream)) == (w_code, w_K, len(w_stream)), (tag, quota, code, K, len(stream), w_code, w_K, len(w_stream))
                assert stream == w_stream, f"{tag} quota {quota}: first difference at byte {ebc.first_difference(stream, w_stream)}"
                if scc.identity(g, kinds[f], shift, n_fg, m.n_units):
                    assert (code, stream) == plain[quota][f], f"{tag} quota {quota}: not the separate call's stream"
                out[shift, q, f] = (code, stream, K, n_fg)
    return out, quotas


def check_recuts(torch, r_, g, specs, masters, sizes, streams, rects, kinds, roi_enc, roi_quotas, what):              # noqa: F811
    """the cuts call and the ROI re-cut of the case's cut list against the host model -> the cut list"""
    n = len(streams)
    cut_list = scc.cuts(g, streams)
    want, derived = scc.model_of_cuts(g, streams, rects, cut_list)
    flat, _ = scc.model_of_cuts(g, streams, [(0, 0, 0, 0)] * n, [(c[0], c[1], 0) for c in cut_list])
    plain = tgc.recut_cuts(torch, r_, masters, sizes, [(c[0], c[1]) for c in cut_list])
    roi = tgo.recut_roi(torch, r_, masters, sizes, rects, cut_list)
    gen = scc.generous(cut_list)
    for c, (r, quota, shift) in enumerate(cut_list):
        m = scc.models(g)[r]
        for f in range(n):
            tag = f"{what}: cut {cut_list[c]} frame {f} {specs[f]} rectangle {rects[f]} ({kinds[f]})"
            w, got = want[c][f], roi[c][f]
            assert got[0] == w[0] and got[2:] == w[2:], (tag, got[0], got[2:], w[0], w[2:])
            assert got[1] == w[1], f"{tag}: first difference at byte {ebc.first_difference(got[1], w[1])}"
            assert plain[c][f] == flat[c][f][:2], f"{tag}: the cuts call, first difference at byte {ebc.first_difference(plain[c][f][1], flat[c][f][1])}"
            check_packets(got[1], tag)
            if scc.identity(g, kinds[f], shift, w[3], m.n_units):
                assert got[:2] == plain[c][f], f"{tag}: not the cuts call's output"
            if gen[r] == c:
                assert got[:3] == (0, derived[r][f], m.n_units), f"{tag}: a generous cut is derive(M, r)"
            if r == 0:
                q = 0 if gen[0] == c else 1                       # (the generous cut keeps every unit, as the lossless quota does)
                assert gen[0] == c or quota == roi_quotas[1]
                assert got == roi_enc[shift, q, f], f"{tag}: not the ROI encode's stream"
    return cut_list


def check_chain(torch, oracle, r_, g, masters, sizes, streams, cut_list, what):                                      # noqa: F811
    """the generous cut of every r, left on the device, through the decoder made for stages - r"""
    n = len(streams)
    gen = scc.generous(cut_list)
    cuts = [(r, cut_list[gen[r]][1]) for r in range(g.stages)]
    stride = (max(q for _, q in cuts) + 5) | 1
    out = torch.zeros((len(cuts), n, stride), dtype=torch.uint8, device="cuda")
    cut_sizes = torch.zeros((len(cuts), n), dtype=torch.int64, device="cuda")
    cut_rcs = torch.full((len(cuts), n), 77, dtype=torch.int32, device="cuda")
    r_.recut_cuts_torch(masters, sizes, cuts, out, cut_sizes, cut_rcs)
    res, decs = [], []
    try:
        for r in range(g.stages):
            rw, rh = red.reduced_size(g.w, g.h, r)
            d = decoder.Decoder(g.channels, g.stages - r, g.filt, g.segments, bits=g.bits)
            decs.append(d)
            planes = torch.full((n, g.channels, rw * rh), 0x5A, dtype=torch.int16 if g.bits == 16 else torch.uint8, device="cuda")
            rcs = torch.full((n,), 77, dtype=torch.int32, device="cuda")
            ws, hs = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
            d.decode_torch(out[r], cut_sizes[r], planes, rcs, ws, hs)
            res.append((planes, rcs, ws, hs))
        torch.cuda.synchronize()
    finally:
        for d in decs:
            d.close()
    assert cut_rcs.cpu().tolist() == [[0] * n] * len(cuts), what
    for r, (planes, rcs, ws, hs) in enumerate(res):
        b = scc.SweepBatch(oracle, g, streams, r, from_masters=False)
        flat = planes.cpu().numpy()
        flat = flat.view(np.uint16) if g.bits == 16 else flat
        b.check(rcs.cpu().tolist(), ws.cpu().tolist(), hs.cpu().tolist(), lambda k, c: flat[k, c], f"{what}: the generous cut at r {r} decoded")


def check_reduced_and_display(torch, oracle, g, streams, what):                                                      # noqa: F811
    """Decoder(reduce=r) on the masters at r in {1, stages - 1}; the display decode at r = stages - 1"""
    for r in sorted({min(1, g.stages - 1), g.stages - 1}):
        b = scc.SweepBatch(oracle, g, streams, r)
        d = decoder.Decoder(g.channels, g.stages, g.filt, g.segments, bits=g.bits, reduce=r)
        try:
            assert d.reduce == r
            if r > 0:
                rcs, ws, hs, frame = tgx.async_call(torch, d, b, b.stride)
                b.check(rcs, ws, hs, frame, f"{what}: the masters at reduce {r}")
            if r == g.stages - 1:
                scc.check_display(b, tgd.display_call(torch, "async", d, b, b.stride), tgd.plain_call(torch, d, b, b.stride), JUNK,
                                  f"{what}: display at reduce {r}")
        finally:
            d.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", list(enumerate(CASES)), ids=[gsc.case_id(g) for g, _ in CASES])
def test_roi_encode_recuts_and_decodes(torch, oracle, expected, case):            # noqa: F811
    i, (g, specs) = case
    what = gsc.case_id(g)
    m = scc.models(g)[0]
    rects, kinds = scc.rectangles(i, g), scc.rect_kinds(i)
    enc, r_ = tg.encoder(g, len(specs)), tgc.recutter(g)
    try:
        assert m.n_units == enc.info()["units_per_frame"] == gsc.n_units(g) and r_.max_reduce == g.stages - 1
        t = tl.device_frames(ebc.batch(g, specs))
        big = ebc.quota(g, "lossless")
        masters, sizes, enc_rcs = tg.encode_masters(torch, enc, t, big)
        streams = tgc.host_streams(masters, sizes)
        for f, spec in enumerate(specs):
            ebc.check_frame(int(enc_rcs[f]), streams[f], expected(g, spec, big), f"{what}: master {f} {spec}")
            assert int(enc_rcs[f]) == 0
        roi_enc, roi_quotas = check_roi_encode(enc, t, g, m, specs, streams, rects, kinds, what)
        assert enc.stats()["unit_timeouts"] == 0
        cut_list = check_recuts(torch, r_, g, specs, masters, sizes, streams, rects, kinds, roi_enc, roi_quotas, what)
        check_chain(torch, oracle, r_, g, masters, sizes, streams, cut_list, what)
        check_reduced_and_display(torch, oracle, g, streams, what)
    finally:
        enc.close()
        r_.close()
