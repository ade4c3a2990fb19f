"""The geometry sweep of the ROI encode, the re-cuts by resolution and by region and the reduced and display decodes, on the CPU
(tests/sweep_cut_cases.py over the sample of tests/geometry_sweep_cases.py).  For every swept geometry:

  conditions   the non-vacuity conditions of sweep_cut_cases hold on the models alone;
  rank, scan   roi_rank_kernel's phases and scan_roi_wave (tests/emu/roi_emu.cpp, the binding of tests/test_emu_roi.py) on the
               bit counts of the oracle's lossless streams give roi_model's rank, order, foreground count, K, size, rc and
               final offsets at the three shifts and the four quotas;
  re-cuts      icerx_recut_device_cuts_async and icerx_recut_device_roi_async through the mock runtime (the build of
               tests/test_recut_mock.py) on the oracle's lossless masters at odd offsets: every (rc, stream, K, foreground)
               equals model_cuts on derive(M, r) with the model of the geometry at 1/2^r size and the scaled rectangle; a
               generous cut is derive(M, r); a shift-0 ROI cut is the cuts call's; a reduce-0 ROI cut is
               roi_model.roi_streams -- the stream icerx_encode_device_roi makes;
  decodes      Decoder(reduce=r) through the same build at r in {0, 1, stages - 1} (host, synchronous and asynchronous calls:
               check_planes of tests/test_reduced_mock.py) gives reduced_model.expected -- the decoder oracle on derive(M, r);
               rc -3 and the words decoded so far under quirk P1 -- and the display decode at r = stages - 1 gives
               tests/display_model.py of those planes.  (A frame of 12-bit content whose chains read on behind their packets
               is owed rc and size alone at r >= 1, the exception include/icer_hip_dec.h makes: sweep_cut_cases.SweepBatch.
               On the committed seed that is 13 of the 111 (geometry, r, frame) decodes at r >= 1.)
  reference    the unmodified reference decoder, told stages - r, decodes one ROI cut per r to what the decoder oracle gives
               (the geometries without a kept grid).
The same cases run on the GPU in tests/test_gpu_geometry_sweep_cuts.py."""
import ctypes as C

import numpy as np
import pytest

from tests import encoder_batch_cases as ebc
from tests import geometry_sweep_cases as gsc
from tests import reduced_model as red
from tests import roi_model as rm
from tests import sweep_cut_cases as scc
from tests import test_recut_cuts_mock as tcm
from tests import test_recut_mock as trm
from tests.decoder_batch_cases import oracle_decode
from tests.test_display_mock import JUNK, display_call, plain_call
from tests.test_emu_roi import lib                                  # noqa: F401  (fixture: the build of tests/emu/roi_emu.cpp)
from tests.test_recut_mock import mock_lib                          # noqa: F401  (fixture: decoder.hip against the mock runtime)
from tests.test_recut_roi_mock import roi_call
from tests.test_reduced_mock import check_planes

CASES = gsc.cases()
INDEXED = list(enumerate(CASES))
sweep = pytest.mark.parametrize("case", INDEXED, ids=[gsc.case_id(g) for g, _ in CASES])
no_kept_grid = pytest.mark.parametrize("case", [c for c in INDEXED if not gsc.is_p1(c[1][0])],
                                       ids=[gsc.case_id(g) for g, _ in CASES if not gsc.is_p1(g)])
QUOTA_EXCEEDED = trm.QUOTA_EXCEEDED


@pytest.fixture(scope="module")
def expected(oracle):
    return ebc.Expected(oracle)


def masters_of(expected, g, specs):
    """the oracle's lossless streams of the batch: the masters"""
    res = [expected(g, s, ebc.quota(g, "lossless")) for s in specs]
    assert all(m[0] == 0 for m in res)
    return [m[1] for m in res]


# ---- 1. the conditions ------------------------------------------------------------------------------------------------------------
def test_cases_and_conditions(expected):
    """every case and every r has its models (none is refused), the six rectangle kinds occur, a call never takes more than 16
    cuts, and the cuts depend on the rectangle where sweep_cut_cases says they must"""
    assert len(CASES) == 28 and sum(g.stages - 1 for g, _ in CASES) == 56
    assert sum(gsc.is_p1(g) for g, _ in CASES) == 3
    kinds = set()
    for i, (g, specs) in INDEXED:
        assert len(scc.models(g)) == g.stages and all(m.n_units > 0 for m in scc.models(g))
        kinds |= set(scc.rect_kinds(i))
        assert scc.decode_reduces(g) == sorted({0, min(1, g.stages - 1), g.stages - 1})
    assert kinds == {"empty", "full", "segment", "border", "last", "outside"}
    at0, reduced, pairs = scc.check_conditions(lambda g, spec: expected(g, spec, ebc.quota(g, "lossless"))[1])
    print(f"cuts that depend on the rectangle: {at0} geometries at r = 0, {reduced} of {pairs} (geometry, r >= 1) pairs")
    assert pairs == 56


# ---- 2. ROI rank and scan ---------------------------------------------------------------------------------------------------------
@sweep
def test_roi_rank_and_scan_equal_the_model(lib, expected, case):                 # noqa: F811
    i, (g, specs) = case
    m = scc.models(g)[0]
    n = lib.emu_roi_plan(g.w, g.h, g.channels, g.stages, g.segments, g.bits)
    assert n == m.n_units == gsc.n_units(g)
    forder = rm.final_order(m)
    streams = masters_of(expected, g, specs)
    rects, kinds = scc.rectangles(i, g), scc.rect_kinds(i)
    quotas = np.array(scc.roi_quotas(g, streams), np.uint64)
    Q = len(quotas)
    unbound = np.zeros(n, np.uint8)
    for f, stream in enumerate(streams):
        packets = rm.split_stream(m, stream)
        assert len(packets) == n
        bits = np.array([int.from_bytes(packets[k][16:20], "little") for k in range(n)], np.uint32)
        want, n_fg = {}, {}
        for shift in scc.SHIFTS:
            want[shift], n_fg[shift] = rm.roi_streams(m, stream, rects[f], shift, quotas.tolist())
            what = (gsc.case_id(g), f, kinds[f], rects[f], shift)
            rank, order, fgc = np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), C.c_uint32(7)
            lib.emu_roi_rank(np.array([v & 0xFFFFFFFF for v in rects[f]], np.uint32), shift, 77 * f + shift, rank, order, C.byref(fgc))
            w_rank, w_order, w_fg = rm.roi_order(m, rects[f], shift)
            assert fgc.value == w_fg == n_fg[shift], what
            assert order.tolist() == w_order and rank.tolist() == w_rank, what
            foff = np.full(Q * n, 7, np.uint64)
            sizes, rcs, kept = np.full(Q, 7, np.uint64), np.full(Q, 7, np.int32), np.full(Q, 7, np.uint32)
            assert lib.emu_scan_roi(bits, quotas, Q, 0, unbound, rank, order, foff, sizes, rcs, kept) == 0, what
            for q, quota in enumerate(quotas.tolist()):
                w_foff, w_size, w_rc, w_K, _ = rm.scan(bits, forder, w_rank, w_order, quota)
                assert (int(sizes[q]), int(rcs[q]), int(kept[q])) == (w_size, w_rc, w_K), (what, quota)
                assert foff[q * n: (q + 1) * n].tolist() == w_foff, (what, quota)
                assert (len(want[shift][q][0]), want[shift][q][1], want[shift][q][2]) == (w_size, w_rc, w_K), (what, quota)
            assert want[shift][0] == (stream, 0, n), (what, "the lossless quota keeps every unit")
            if scc.identity(g, kinds[f], shift, w_fg, n):
                assert w_order == list(range(n)) and want[shift] == want[0], what


# ---- 3. the cuts call and the ROI re-cut through the mock runtime -------------------------------------------------------------------
def mock_cuts(lib_, g, streams, rects, cut_list, rng):
    """(the cuts call's res[c][f] = (rc, stream), the ROI re-cut's res[c][f] = (rc, stream, K, foreground)) of one recutter
    made with max_reduce = stages - 1, the masters at odd offsets with junk between them"""
    r_ = tcm.recutter(lib_, g)
    assert r_.max_reduce == g.stages - 1
    blob, offsets = trm.pack_odd(rng, streams)
    lens = [len(s) for s in streams]
    code, plain = tcm.cuts_call(r_, blob, offsets, lens, [(c[0], c[1]) for c in cut_list])
    assert code == 0
    code, roi = roi_call(r_, blob, offsets, lens, rects, cut_list)
    assert code == 0
    r_.close()
    return plain, roi


@sweep
def test_recuts_mock_equal_the_model(mock_lib, expected, case):                  # noqa: F811
    i, (g, specs) = case
    what = gsc.case_id(g)
    rng = np.random.default_rng(g.w * 1000 + g.h)
    streams = masters_of(expected, g, specs)
    rects, kinds = scc.rectangles(i, g), scc.rect_kinds(i)
    if g.segments > 1:                                             # (the case's own share of the non-vacuity conditions)
        assert scc.depends_on_rectangle(g, 0, streams[0]), f"{what}: no cut at r = 0 depends on the rectangle"
    cut_list = scc.cuts(g, streams)
    want, derived = scc.model_of_cuts(g, streams, rects, cut_list)
    flat, _ = scc.model_of_cuts(g, streams, [(0, 0, 0, 0)] * len(streams), [(c[0], c[1], 0) for c in cut_list])
    plain, roi = mock_cuts(mock_lib, g, streams, rects, cut_list, rng)
    gen = scc.generous(cut_list)
    assert sorted(gen) == list(range(g.stages))
    for c, (r, quota, shift) in enumerate(cut_list):
        m = scc.models(g)[r]
        for f in range(len(streams)):
            tag = f"{what}: cut {cut_list[c]} frame {f} {specs[f]} rectangle {rects[f]} ({kinds[f]})"
            w, got = want[c][f], roi[c][f]
            assert got[0] == w[0] and got[2:] == w[2:], (tag, got[0], got[2:], w[0], w[2:])
            assert got[1] == w[1], f"{tag}: first difference at byte {ebc.first_difference(got[1], w[1])}"
            assert plain[c][f] == flat[c][f][:2], f"{tag}: the cuts call, first difference at byte {ebc.first_difference(plain[c][f][1], flat[c][f][1])}"
            if scc.identity(g, kinds[f], shift, w[3], m.n_units):
                assert got[:2] == plain[c][f], f"{tag}: not the cuts call's output"
            if gen[r] == c:
                assert got[:3] == (0, derived[r][f], m.n_units) == plain[c][f] + (m.n_units,), f"{tag}: a generous cut is derive(M, r)"
            if r == 0:
                ((s, code, K),), n_fg = rm.roi_streams(m, streams[f], rects[f], shift, [quota])
                assert got == (code, s, K, n_fg), f"{tag}: not the ROI encode's stream"
            tcm.check_packets(got[1], tag)


# ---- 4. reduced and display decodes through the mock runtime ------------------------------------------------------------------------
@sweep
def test_reduced_and_display_decodes_mock(mock_lib, oracle, expected, case):      # noqa: F811
    from icer_compression_amd import decoder
    i, (g, specs) = case
    streams = masters_of(expected, g, specs)
    for r in scc.decode_reduces(g):
        label = f"{gsc.case_id(g)} r {r}"
        b = scc.SweepBatch(oracle, g, streams, r)
        for f, exact in enumerate(b.exact):                        # (only 12-bit content reads on behind its packets)
            assert exact or "wide" in ebc.channel_kinds(g, specs[f][0]), (label, f, specs[f])
        d = decoder.Decoder(g.channels, g.stages, g.filt, g.segments, bits=g.bits, lib=mock_lib, reduce=r)
        assert d.reduce == r
        check_planes(d, b, label)
        if r == g.stages - 1:
            scc.check_display(b, display_call("async", d, b, b.stride), plain_call(d, b, b.stride), JUNK, label)
        d.close()


# ---- 5. the reference decoder on ROI cuts --------------------------------------------------------------------------------------------
@no_kept_grid
def test_reference_decoder_decodes_one_roi_cut_per_r(mock_lib, oracle, reference, expected, case):      # noqa: F811
    """the cut at half the generous quota, shift 3, of every r: the reference decoder told stages - r against the decoder oracle
    (a colour stream that lacks a channel altogether is not the reference's to decode: tests/decoder_batch_cases.py)"""
    i, (g, specs) = case
    streams = masters_of(expected, g, specs)
    rects = scc.rectangles(i, g)
    cut_list = [c for c in scc.cuts(g, streams) if c[2] == 3]
    assert [c[0] for c in cut_list] == list(range(g.stages))
    _, roi = mock_cuts(mock_lib, g, streams, rects, cut_list, np.random.default_rng(3))
    for c, (r, quota, shift) in enumerate(cut_list):
        rw, rh = red.reduced_size(g.w, g.h, r)
        seen = 0
        for f in range(len(streams)):
            code, s = roi[c][f][:2]
            assert code in (0, QUOTA_EXCEEDED), (gsc.case_id(g), cut_list[c], f)
            if len(s) <= 28 or (g.channels == 3 and len({s[o + 7] >> 4 for o, _ in red.walk(s)}) < 3):
                continue
            seen += 1
            ref = reference.decompress_raw(s, g.channels, g.stages - r, g.filt, g.segments, rw * rh, g.bits)
            orc = oracle_decode(oracle, s, g.channels, g.stages - r, g.filt, g.segments, rw * rh, g.bits)
            assert ref[:3] == orc[:3] and ref[1:3] == (rw, rh), (gsc.case_id(g), cut_list[c], f, ref[:3], orc[:3])
            assert all(np.array_equal(a, b) for a, b in zip(ref[3], orc[3])), (gsc.case_id(g), cut_list[c], f)
        assert seen >= 1, (gsc.case_id(g), cut_list[c])
