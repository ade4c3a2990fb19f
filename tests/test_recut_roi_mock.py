"""icerx_recut_device_roi_async end to end on the CPU (the mock build of tests/test_recut_mock.py): stored masters cut by
(resolution, byte quota, ROI shift) with a rectangle per frame.  The masters are the oracle's streams.

  reduce 0    against tests/roi_model.py run on the master's packet table -- for a lossless master that is roi_model.roi_streams,
              the stream icerx_encode_device_roi makes of the frame, and the digests of tests/golden/roi_golden.json recorded for
              that encode -- on the geometries, frames, rectangles, shifts and quotas of tests/roi_cases.py;
  reduce r    against the same model run on derive(M, r) with the geometry at 1/2^r size and the scaled rectangle, and against
              the DEFINITION: a reduce-0 ROI call of a plain recutter for that geometry on derive(M, r) (odd image sizes, so that
              every ceil matters);
  shift 0, no region of interest, a foreground of every unit, one segment: icerx_recut_device_cuts_async's output;
  cut, truncated, damaged, alien and out-of-blob masters; the buffer promises; the refusals.
CPU only."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import encoder_batch_cases as ebc
from tests import reduced_model as red
from tests import roi_cases as rc
from tests import roi_model as rm
from tests import target_model as tm
from tests import test_recut_cuts_mock as tcm
from tests import test_recut_mock as trm
from tests.decoder_batch_cases import oracle_decode
from tests.test_recut_mock import expected, mock_lib        # noqa: F401  (fixtures: the oracle's streams, the mock build)

SENT, SENT_SIZE, SENT_RC, SENT_U32 = trm.SENT, trm.SENT_SIZE, trm.SENT_RC, 0x5A5A5A5A
QUOTA_EXCEEDED, OUT_OF_DATA, INVALID_INPUT, FATAL = trm.QUOTA_EXCEEDED, trm.OUT_OF_DATA, trm.INVALID_INPUT, trm.FATAL
GUARD = trm.GUARD
HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "roi_golden.json")) as _fh:
    GOLDEN = json.load(_fh)


def model_of(g):
    return tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments, g.bits)


def roi_call(r, blob, offsets, lens, rects, cuts, stream_stride=0, stride=None, ws_bytes=None, null_reduces=False, **override):
    """icerx_recut_device_roi_async on host arrays (the mock's device memory), cuts = [(reduce, quota, shift)], into
    len(cuts) * n + 1 sentinel rows of an odd stride and a workspace of exactly roi_workspace_bytes with a guard tail
    -> (rc of the call, res[c][f] = (rc, stream, K, foreground units)) after checking the buffer promises"""
    n, Q = len(lens), len(cuts)
    reduces, quotas, shifts = [c[0] for c in cuts], [c[1] for c in cuts], [c[2] for c in cuts]
    stride = stride or (max(quotas) + 5) | 1
    out = np.full((Q * n + 1, stride), SENT, np.uint8)
    sizes = np.full(Q * n + 1, SENT_SIZE, np.uint64)
    rcs = np.full(Q * n + 1, SENT_RC, np.int32)
    kept = np.full(Q * n + 1, SENT_U32, np.uint32)
    fg = np.full(Q * n + 1, SENT_U32, np.uint32)
    offs = np.asarray(offsets, np.uint64) if offsets is not None else None
    ln = np.asarray(lens, np.uint64)
    rois = np.array([[int(v) & 0xFFFFFFFF for v in rect] for rect in rects], np.uint32).reshape(-1, 4)
    keep, keep_rois = blob.copy(), rois.copy()
    need = r.roi_workspace_bytes(n, len(blob), Q)
    work = np.full(need + GUARD, 0xCD, np.uint8)
    args = dict(n=n, d_data=blob.ctypes.data, data_bytes=len(blob), d_offsets=offs.ctypes.data if offs is not None else None,
                stream_stride=stream_stride, d_lens=ln.ctypes.data, d_rois=rois.ctypes.data, reduces=None if null_reduces else reduces,
                shifts=shifts, quotas=quotas, d_out=out.ctypes.data, out_stride=stride, d_sizes=sizes.ctypes.data, d_rcs=rcs.ctypes.data,
                d_kept=kept.ctypes.data, d_foreground=fg.ctypes.data, d_workspace=work.ctypes.data,
                workspace_bytes=need if ws_bytes is None else ws_bytes, stream=None)
    args.update(override)
    rc = r.recut_roi_device_async_ptrs(**args)
    assert (work[need:] == 0xCD).all(), "written behind the workspace"
    assert np.array_equal(blob, keep), "the masters were modified"
    assert np.array_equal(rois, keep_rois), "the rectangles were modified"
    if rc != 0:
        assert (out == SENT).all() and (sizes == SENT_SIZE).all() and (rcs == SENT_RC).all(), "a refused call wrote"
        assert (kept == SENT_U32).all() and (fg == SENT_U32).all(), "a refused call wrote"
        return rc, None
    assert (out[Q * n] == SENT).all() and sizes[Q * n] == SENT_SIZE and rcs[Q * n] == SENT_RC, "written past the n_cuts * n rows"
    assert kept[Q * n] == SENT_U32 and fg[Q * n] == SENT_U32, "entries written past n_cuts * n"
    res = []
    for c, quota in enumerate(quotas):
        row = []
        for f in range(n):
            k = c * n + f
            s = int(sizes[k])
            assert 0 <= s <= quota, (c, f, s, quota)
            assert (out[k, s:] == SENT).all(), f"cut {c} frame {f}: bytes written behind its stream of {s} bytes"
            row.append((int(rcs[k]), out[k, :s].tobytes(), int(kept[k]), int(fg[k])))
        res.append(row)
    return rc, res


def model_cuts(m, master, rect, shift, quotas):
    """the definition at reduce 0 in plain integers: roi_model's order and scan on the packet table of `master` (its CRC-valid
    packets; a unit without one is TOO_BIG) -> ([(rc, stream, K, foreground units)] per quota); a master without a valid
    packet: ICER_DECODER_OUT_OF_DATA and zeros"""
    index, packets = m.unit_index(), {}
    for off, n in red.walk(master):
        key = (master[off + 7] >> 4, master[off + 4], master[off + 5], master[off + 7] & 15, master[off + 6])
        if key in index:
            packets[index[key]] = master[off: off + n]
    if not packets:
        return [(OUT_OF_DATA, b"", 0, 0) for _ in quotas]
    bits = [int.from_bytes(packets[k][16:20], "little") if k in packets else rm.TOO_BIG for k in range(m.n_units)]
    forder = rm.final_order(m)
    rank, order, n_fg = rm.roi_order(m, rect, shift)
    out = []
    for quota in quotas:
        _, size, code, K, _ = rm.scan(bits, forder, rank, order, int(quota))
        stream = b"".join(packets[u] for u in forder if rank[u] < K)
        assert len(stream) == size
        out.append((code, stream, K, n_fg))
    return out


def scaled_rect(rect, w, h, r):
    """the rectangle of a cut at reduce r as (x, y, w, h) of the image at 1/2^r size; (0, 0, 0, 0) for none"""
    x0, y0, x1, y1 = rm.clip(rect, w, h)
    if x1 <= x0 or y1 <= y0:
        return (0, 0, 0, 0)
    sx0, sy0, sx1, sy1 = x0 >> r, y0 >> r, -(-x1 >> r), -(-y1 >> r)
    rw, rh = red.reduced_size(w, h, r)
    assert sx0 < sx1 <= rw and sy0 < sy1 <= rh
    return (sx0, sy0, sx1 - sx0, sy1 - sy0)


def check_valid(m, stream, master_r, what):
    """consequence 6 without a decoder: packets with both CRCs valid and nothing else, each of them a packet of M_r, no hole
    above a kept plane"""
    tcm.check_packets(stream, what)
    have = {master_r[o: o + n] for o, n in red.walk(master_r)}
    assert all(stream[o: o + n] in have for o, n in red.walk(stream)), f"{what}: a packet that M_r does not hold"
    assert rm.kept_planes_are_top_runs(m, stream), f"{what}: a hole above a kept plane"


def two_calls(rng, combos):
    """the (quota, shift) combinations of a case, shuffled, in calls of at most 16 cuts, one cut of each call twice"""
    combos = list(combos)
    rng.shuffle(combos)
    calls = []
    for at in range(0, len(combos), 15):
        part = [tuple(int(v) for v in c) for c in combos[at: at + 15]]
        part.insert(int(rng.integers(0, len(part) + 1)), part[int(rng.integers(0, len(part)))])
        calls.append(part)
    return calls


# ------------------------------------------------------------------------------------------------ reduce 0: the encoder's streams
@pytest.mark.parametrize("name", list(rc.GEOMETRIES))
def test_reduce_0_equals_the_roi_encode(mock_lib, expected, oracle, name):
    g, m, quotas = rc.GEOMETRIES[name], rc.model(name), rc.quotas(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    n_ll = sum(u[2] == tm.LL for u in m.units)
    plain_r, reduced_r = trm.recutter(mock_lib, g), tcm.recutter(mock_lib, g)
    decoded = {}
    for b, specs in enumerate(rc.BATCHES[name]):
        rects = rc.rectangles(name, b)
        masters = [expected(g, s, quotas[0]) for s in specs]
        assert all(mm[0] == (0 if rc.has_stream(s) else -1) and (rc.has_stream(s) or mm[1] == b"") for mm, s in zip(masters, specs))
        assert sum(not rc.has_stream(s) for s in specs) <= 1
        streams = [mm[1] for mm in masters]
        n = len(specs)
        # the expected value of every (shift, quota, frame), from the model alone
        want = {}
        for shift in rc.SHIFTS:
            gold = GOLDEN[rc.golden_key(name, b, shift)]
            for f, spec in enumerate(specs):
                if not rc.has_stream(spec):
                    for q in range(len(quotas)):
                        want[shift, q, f] = (OUT_OF_DATA, b"", 0, 0)
                    continue
                res, n_fg = rm.roi_streams(m, streams[f], rects[f], shift, quotas)
                assert n_fg == gold["foreground"][f]
                for q, (s, code, K) in enumerate(res):
                    assert (len(s), code, K, hashlib.sha256(s).hexdigest()[:16]) == \
                        (gold["size"][q][f], gold["rc"][q][f], gold["kept"][q][f], gold["sha256_16"][q][f]), (name, b, shift, q, f)
                    want[shift, q, f] = (code, s, K, n_fg)
        if b == 0 and name != "G5":
            # non-vacuity: the `segment` rectangle (frame 2) at shift 3 changes a stream, its foreground is a proper part
            assert rc.RECT_KINDS[2] == "segment" and rc.has_stream(specs[2])
            assert any(want[3, q, 2][1] != want[0, q, 2][1] for q in range(len(quotas))), "shift 3 changes no stream of this case"
            assert n_ll < want[3, 0, 2][3] < m.n_units, (n_ll, want[3, 0, 2][3], m.n_units)
        combos = [(q, shift) for shift in rc.SHIFTS for q in range(len(quotas))]
        for k, part in enumerate(two_calls(rng, combos)):
            cuts = [(0, quotas[q], shift) for q, shift in part]
            r, null_reduces = ((plain_r, True), (reduced_r, False))[k % 2]
            plain = tcm.cuts_call(reduced_r, *trm.pack_odd(rng, streams), [len(s) for s in streams], [(0, c[1]) for c in cuts])
            assert plain[0] == 0
            for what, (code, got) in tcm.both_layouts(rng, streams, lambda bl, o, ln, st: roi_call(r, bl, o, ln, rects, cuts, stream_stride=st,
                                                                                                   null_reduces=null_reduces)):
                assert code == 0, what
                for c, (q, shift) in enumerate(part):
                    for f, spec in enumerate(specs):
                        tag = f"{name} batch {b} {what}: cut {cuts[c]} frame {f} {spec} rectangle {rects[f]}"
                        w = want[shift, q, f]
                        assert got[c][f][0] == w[0] and got[c][f][2:] == w[2:], (tag, got[c][f][0], got[c][f][2:], w[0], w[2:])
                        assert got[c][f][1] == w[1], f"{tag}: first difference at byte {ebc.first_difference(got[c][f][1], w[1])}"
                        kind = rc.RECT_KINDS[((0, 3)[b] + f) % 6]
                        if shift == 0 or kind in ("empty", "outside") or w[3] == m.n_units or g.segments == 1 or not rc.has_stream(spec):
                            assert got[c][f][:2] == plain[1][c][f], f"{tag}: not the plain cut"
                        if w[1] and w[1] not in decoded:
                            check_valid(m, w[1], streams[f], tag)
                            decoded[w[1]] = tag
    plain_r.close()
    reduced_r.close()
    for s, tag in list(decoded.items())[:: max(1, len(decoded) // 24)]:
        rcd, wd, hd, _ = oracle_decode(oracle, s, g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits)
        assert (rcd, wd, hd) == (0, g.w, g.h), tag


# ------------------------------------------------------------------------------------------------ reduce r: the definition
def reduced_case(name):
    g, specs = tcm.GEOMETRIES[name]
    m = model_of(g)
    kinds = [rc.RECT_KINDS[(2 + f) % 6] for f in range(len(specs))]         # segment, border, last, outside, empty, ...
    return g, specs, m, [rc.rectangle(m, k) for k in kinds], kinds


def mixed_cuts(g, streams, rng):
    """every r in 0 .. S - 1 with three quotas (above, at half and at a fifth of the longest derived master) at shifts 3, 0 and
    another of roi_cases.SHIFTS, 60 / 28 bytes at some (r, shift), one cut twice; shuffled.  12 cuts for 3 stages, 15 for 4."""
    cuts = []
    for r in range(g.stages):
        top = max(len(red.derive(s, r)) for s in streams)
        cuts += [(r, top + 9, 3), (r, top // 2, 0), (r, top // 5, rc.SHIFTS[1 + (r + 2) % 4]), (r, top // 2, 3)][: 3 if g.stages == 4 else 4]
    cuts += [(int(rng.integers(0, g.stages)), q, rc.SHIFTS[int(rng.integers(0, 5))]) for q in (60, 28)]
    cuts.append(cuts[int(rng.integers(0, len(cuts)))])
    rng.shuffle(cuts)
    cuts = [tuple(int(v) for v in c) for c in cuts]
    assert len(cuts) <= 16
    return cuts


def by_definition(lib, g, streams, rects, cuts, rng):
    """want[c][f] = (rc, stream, K, foreground): a reduce-0 ROI call of a plain recutter for the geometry at 1/2^r size on
    derive(M, r) with the scaled rectangles, one call per reduce"""
    want = [None] * len(cuts)
    for r in sorted({c[0] for c in cuts}):
        idx = [i for i, c in enumerate(cuts) if c[0] == r]
        derived = [red.derive(s, r) for s in streams]
        plain = trm.recutter(lib, tcm.reduced_geometry(g, r))
        blob, offsets = trm.pack_odd(rng, derived)
        code, got = roi_call(plain, blob, offsets, [len(s) for s in derived], [scaled_rect(x, g.w, g.h, r) for x in rects],
                             [(0, cuts[i][1], cuts[i][2]) for i in idx], null_reduces=True)
        plain.close()
        assert code == 0
        for j, i in enumerate(idx):
            want[i] = got[j]
    return want


@pytest.mark.parametrize("master_cls", ["lossless", "cut"])
@pytest.mark.parametrize("name", ["yuv16", "gray16"])
def test_reduced_cuts_equal_the_definition_and_the_model(mock_lib, expected, oracle, name, master_cls):
    g, specs, m, rects, kinds = reduced_case(name)
    rng = np.random.default_rng(sum(map(ord, name + master_cls)))
    streams, mrcs = tcm.masters_of(expected, g, specs, master_cls)
    assert master_cls == "lossless" or any(code == QUOTA_EXCEEDED for code in mrcs), "no master of this batch is cut"
    cuts = mixed_cuts(g, streams, rng)
    assert len({c[0] for c in cuts}) == g.stages and len({c[2] for c in cuts}) >= 3
    models = [model_of(tcm.reduced_geometry(g, r)) for r in range(g.stages)]
    derived = [[red.derive(s, r) for s in streams] for r in range(g.stages)]
    want = by_definition(mock_lib, g, streams, rects, cuts, rng)
    # the model, independent of any recutter
    for c, (r, quota, shift) in enumerate(cuts):
        for f in range(len(specs)):
            (w,) = model_cuts(models[r], derived[r][f], scaled_rect(rects[f], g.w, g.h, r), shift, [quota])
            assert want[c][f] == w, (name, master_cls, cuts[c], f, want[c][f][0], want[c][f][2:], w[0], w[2:])
    if master_cls == "lossless":
        # non-vacuity: at some r > 0 the `segment` rectangle (frame 0) changes a stream and its foreground is a proper part
        assert kinds[0] == "segment"
        changed = False
        for r in range(1, g.stages):
            q = len(derived[r][0]) // 2
            a, b = (model_cuts(models[r], derived[r][0], scaled_rect(rects[0], g.w, g.h, r), s, [q])[0] for s in (0, 3))
            changed |= a[1] != b[1] and sum(u[2] == tm.LL for u in models[r].units) < b[3] < models[r].n_units
        assert changed, "no reduced cut of this case depends on the rectangle"
    r_ = tcm.recutter(mock_lib, g)
    plain = tcm.cuts_call(r_, *trm.pack_odd(rng, streams), [len(s) for s in streams], [(c[0], c[1]) for c in cuts])
    assert plain[0] == 0
    decoded = {}
    for what, (code, got) in tcm.both_layouts(rng, streams, lambda bl, o, ln, st: roi_call(r_, bl, o, ln, rects, cuts, stream_stride=st)):
        assert code == 0, what
        for c, cut in enumerate(cuts):
            for f, spec in enumerate(specs):
                tag = f"{name} {master_cls} master, {what}: cut {cut} frame {f} {spec} rectangle {rects[f]} ({kinds[f]})"
                w = want[c][f]
                assert got[c][f][0] == w[0] and got[c][f][2:] == w[2:], (tag, got[c][f][0], got[c][f][2:], w[0], w[2:])
                assert got[c][f][1] == w[1], f"{tag}: first difference at byte {ebc.first_difference(got[c][f][1], w[1])}"
                if cut[2] == 0 or kinds[f] in ("empty", "outside") or w[3] in (0, models[cut[0]].n_units):
                    assert got[c][f][:2] == plain[1][c][f], f"{tag}: not the plain cut"
                if w[0] in (0, QUOTA_EXCEEDED):
                    assert w[0] == 0 or w[2] < models[cut[0]].n_units
                    if w[1] and (cut[0], w[1]) not in decoded:
                        check_valid(models[cut[0]], w[1], derived[cut[0]][f], tag)
                        decoded[cut[0], w[1]] = tag
                else:
                    assert w == (OUT_OF_DATA, b"", 0, 0), tag
    r_.close()
    assert any(r for r, _ in decoded)
    for (r, s), tag in list(decoded.items())[:: max(1, len(decoded) // 16)]:
        rw, rh = red.reduced_size(g.w, g.h, r)
        rcd, wd, hd, _ = oracle_decode(oracle, s, g.channels, g.stages - r, g.filt, g.segments, rw * rh, g.bits)
        assert (rcd, wd, hd) == (0, rw, rh), tag


@pytest.mark.parametrize("name", ["yuv16", "gray16"])
def test_reference_decoder_decodes_the_roi_cuts(mock_lib, expected, oracle, reference, name):
    """the unmodified reference decoder, told stages - r, decodes ROI cuts to the oracle's image"""
    g, specs, m, rects, kinds = reduced_case(name)
    streams, mrcs = tcm.masters_of(expected, g, specs[:3], "lossless")
    keep = [f for f, code in enumerate(mrcs) if code == 0][:2]
    streams, rects = [streams[f] for f in keep], [rects[f] for f in keep]
    cuts = []
    for r in range(g.stages):
        top = max(len(red.derive(s, r)) for s in streams)
        cuts += [(r, top // 3, 3), (r, top // 6, 16)]
    r_ = tcm.recutter(mock_lib, g)
    blob, offsets = trm.pack_odd(np.random.default_rng(3), streams)
    code, got = roi_call(r_, blob, offsets, [len(s) for s in streams], rects, cuts)
    assert code == 0
    for c, (r, quota, shift) in enumerate(cuts):
        rw, rh = red.reduced_size(g.w, g.h, r)
        for f in range(len(streams)):
            code_f, s = got[c][f][:2]
            assert code_f in (0, QUOTA_EXCEEDED) and len(s) > 28, (name, cuts[c], f)
            ref = reference.decompress_raw(s, g.channels, g.stages - r, g.filt, g.segments, rw * rh, g.bits)
            orc = oracle_decode(oracle, s, g.channels, g.stages - r, g.filt, g.segments, rw * rh, g.bits)
            assert ref[:3] == orc[:3] and ref[1:3] == (rw, rh), (name, cuts[c], f, ref[:3], orc[:3])
            assert all(np.array_equal(a, b) for a, b in zip(ref[3], orc[3])), (name, cuts[c], f)
    r_.close()


# ------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_stored_roi_streams_compose(mock_lib, expected, name):
    """a stored ROI stream made with (rectangle, shift) at Q1, re-cut with the same rectangle and shift at Q2 <= Q1, is the ROI
    stream at Q2 -- where the byte-quota call, which walks in priority order, loses what the ROI order had kept"""
    g, m, quotas = rc.GEOMETRIES[name], rc.model(name), rc.quotas(name)
    specs, rects = rc.BATCHES[name][0], [rc.rectangle(rc.model(name), "segment")] * 3
    rng = np.random.default_rng(31)
    streams = [expected(g, s, quotas[0])[1] for s in specs]
    S = g.samples
    q1s, q2s = [S // 2 + S // 8, S // 4], [S // 4, S // 6, S // 16, 60]
    r = trm.recutter(mock_lib, g)
    blob, offsets = trm.pack_odd(rng, streams)
    code, got = roi_call(r, blob, offsets, [len(s) for s in streams], rects, [(0, q, 3) for q in q1s + q2s], null_reduces=True)
    assert code == 0
    lost = False
    for i in range(len(q1s)):
        stored = [x[1] for x in got[i]]
        blob1, offsets1 = trm.pack_odd(rng, stored)
        q2 = [q for q in q2s if q <= q1s[i]]
        code, again = roi_call(r, blob1, offsets1, [len(s) for s in stored], rects, [(0, q, 3) for q in q2], null_reduces=True)
        assert code == 0
        for j, q in enumerate(q2):
            for f in range(len(specs)):
                assert again[j][f][:2] == got[len(q1s) + q2s.index(q)][f][:2], (name, q1s[i], q, f)
                assert again[j][f][3] == got[0][f][3]
        code, flat = trm.recut_call(r, blob1, offsets1, [len(s) for s in stored], q2)
        assert code == 0
        lost |= any(len(flat[j][f][1]) < len(again[j][f][1]) for j in range(len(q2)) for f in range(len(specs)))
    assert lost, "the byte-quota call lost nothing on these stored ROI streams: the case shows nothing"
    r.close()


@pytest.mark.parametrize("name", ["yuv16", "gray16"])
def test_reduced_roi_cuts_compose(mock_lib, expected, name):
    """a stored output of cut (r, Q1, shift), re-cut by a plain recutter of the geometry at 1/2^r size with the scaled rectangle
    at Q2 <= Q1, is cut (r, Q2, shift)"""
    g, specs, m, rects, kinds = reduced_case(name)
    rng = np.random.default_rng(29)
    streams, _ = tcm.masters_of(expected, g, specs, "lossless")
    r_ = tcm.recutter(mock_lib, g)
    for r in range(1, g.stages):
        top = max(len(red.derive(s, r)) for s in streams)
        q1s, q2s = [top + 1, top // 2], [top // 3, top // 7, 60]
        blob, offsets = trm.pack_odd(rng, streams)
        code, got = roi_call(r_, blob, offsets, [len(s) for s in streams], rects, [(r, q, 3) for q in q1s + q2s])
        assert code == 0
        plain = trm.recutter(mock_lib, tcm.reduced_geometry(g, r))
        for i in range(len(q1s)):
            stored = [x[1] for x in got[i]]
            blob1, offsets1 = trm.pack_odd(rng, stored)
            code, again = roi_call(plain, blob1, offsets1, [len(s) for s in stored], [scaled_rect(x, g.w, g.h, r) for x in rects],
                                   [(0, q, 3) for q in q2s], null_reduces=True)
            assert code == 0
            for j in range(len(q2s)):
                for f in range(len(specs)):
                    assert again[j][f][:2] == got[len(q1s) + j][f][:2], (name, r, q1s[i], q2s[j], f)
        plain.close()
    r_.close()


# ------------------------------------------------------------------------------------------------ missing units, statuses
@pytest.mark.parametrize("name", ["yuv16", "gray16"])
def test_damaged_masters(mock_lib, expected, name):
    """a master cut at a fifth of its length, truncated in the middle of a packet, with one payload byte flipped at level 1 and at
    the top level: every cut equals the model on the packets that are left, ends with ICER_BYTE_QUOTA_EXCEEDED at the first unit
    in ROI order without a packet, and damage at a level <= r does not show at r"""
    g, specs, m, rects, kinds = reduced_case(name)
    S = g.stages
    rng = np.random.default_rng(23)
    master = tcm.masters_of(expected, g, specs[:1], "lossless")[0][0]
    fifth = expected(g, specs[0], len(master) // 5)
    assert fifth[0] == QUOTA_EXCEEDED and 0 < len(fifth[1]) <= len(master) // 5
    ends = [o + n for o, n in red.walk(master)]
    mid = master[: ends[len(ends) // 2] - 9]                                  # (ends 9 bytes before the end of a packet)
    low = red.flip_in_packet(master, 1, False, which=2)
    high = red.flip_in_packet(master, S, False, which=3, subband=0)
    streams = [master, fifth[1], mid, low, high]
    rect = rects[0]
    assert kinds[0] == "segment"
    top = len(master) + 3
    cuts = [(r, q, s) for r in range(S) for q, s in ((top, 3), (len(red.derive(master, r)) // 2, 9))] + [(0, top, 0), (1, top, 0)]
    models = [model_of(tcm.reduced_geometry(g, r)) for r in range(S)]
    r_ = tcm.recutter(mock_lib, g)
    blob, offsets = trm.pack_odd(rng, streams)
    code, got = roi_call(r_, blob, offsets, [len(s) for s in streams], [rect] * len(streams), cuts)
    assert code == 0
    for c, (r, quota, shift) in enumerate(cuts):
        for f, s in enumerate(streams):
            (w,) = model_cuts(models[r], red.derive(s, r), scaled_rect(rect, g.w, g.h, r), shift, [quota])
            assert got[c][f] == w, (name, cuts[c], f, got[c][f][0], got[c][f][2:], w[0], w[2:])
        full = got[c][0]
        if quota == top:
            assert full[0] == 0 and full[2] == models[r].n_units
            for f in (1, 2, 4):                                               # units are missing above level r: the walk ends there
                assert got[c][f][0] == QUOTA_EXCEEDED and got[c][f][2] < full[2] and len(got[c][f][1]) < len(full[1]), (cuts[c], f)
        assert (got[c][3] == full) == (r >= 1 or got[c][3][2] == full[2]), (cuts[c], "damage at level 1")
        if r == 0 and quota == top:
            assert got[c][3][0] == QUOTA_EXCEEDED and got[c][3][2] < full[2]
    r_.close()


def test_bad_frames_and_refused_calls(mock_lib, expected):
    g, specs = tcm.GEOMETRIES["gray16"]
    m = model_of(g)
    other = ebc.Geometry(510, 384, 1, 4, 3, 2)
    mq = ebc.quota(g, "lossless")
    good = [expected(g, s, mq)[1] for s in specs[:2]]
    alien = expected(other, ("smooth", 0), ebc.quota(other, "lossless"))[1]
    rng = np.random.default_rng(5)
    junk = rng.integers(0, 256, 3000).astype(np.uint8).tobytes()
    only1 = b"".join(good[0][o: o + n] for o, n in red.walk(good[0]) if good[0][o + 4] == 1)
    streams = [good[0], junk, alien, good[1], b"", only1]
    blob, offsets = trm.pack_odd(rng, streams)
    lens = [len(s) for s in streams]
    offsets += [len(blob) - 10, len(blob) + 1]                          # two frames that leave the blob
    lens += [11, 0]
    rects = [rc.rectangle(m, "segment"), (-5, -5, 40, 40), rc.rectangle(m, "full"), rc.rectangle(m, "border"), (1, 1, 9, 9),
             rc.rectangle(m, "segment"), (0, 0, 1, 1), (3, 3, 3, 3)]
    cuts = [(0, ebc.quota(g, "cut"), 3), (1, mq, 9), (3, 60, 1), (2, 5000, 16), (3, mq, 0), (1, 2000, 3)]
    want = by_definition(mock_lib, g, good, [rects[0], rects[3]], cuts, rng)
    r = tcm.recutter(mock_lib, g)
    code, got = roi_call(r, blob, offsets, lens, rects, cuts)
    assert code == 0
    for c, cut in enumerate(cuts):
        for j, f in enumerate((0, 3)):
            assert got[c][f] == want[c][j], f"a neighbour of bad frames: cut {cut} frame {f}"
            assert got[c][f][3] > 0
        bad = lambda code: (code, b"", 0, 0)
        assert [got[c][f] for f in (1, 2, 4, 6, 7)] == [bad(OUT_OF_DATA), bad(INVALID_INPUT), bad(OUT_OF_DATA), bad(INVALID_INPUT),
                                                         bad(INVALID_INPUT)], cut
        # level-1 packets only: no stream from r = 1 on, a cut stream at r = 0
        assert (got[c][5] == bad(OUT_OF_DATA)) == (cut[0] >= 1), cut
        assert cut[0] >= 1 or (got[c][5][0] == QUOTA_EXCEEDED and got[c][5][3] > 0), cut
    # a rectangle given as int32 values below 0 reads as far outside: the plain cut
    code, neg = roi_call(r, blob, offsets[:1], lens[:1], [(-5, -5, 40, 40)], cuts)
    code2, plain = tcm.cuts_call(r, blob, offsets[:1], lens[:1], [(c[0], c[1]) for c in cuts])
    assert code == 0 == code2 and [x[0][:2] for x in neg] == [x[0] for x in plain]
    # refused calls write nothing (roi_call checks that)
    n = len(lens)
    need = r.roi_workspace_bytes(n, len(blob), len(cuts))
    assert need > r.cuts_workspace_bytes(n, len(blob), len(cuts))
    reduces, quotas, shifts = [c[0] for c in cuts], [c[1] for c in cuts], [c[2] for c in cuts]
    cases = {
        "null rectangles": dict(d_rois=None), "null shifts": dict(shifts=None), "null kept": dict(d_kept=None),
        "null foreground": dict(d_foreground=None), "shift -1": dict(shifts=shifts[:-1] + [-1]), "shift 17": dict(shifts=[17] + shifts[1:]),
        "reduce above max_reduce": dict(reduces=[r.max_reduce + 1] + reduces[1:]), "negative reduce": dict(reduces=reduces[:-1] + [-1]),
        "no cuts": dict(n_cuts=0), "17 cuts": dict(reduces=[1] * 17, quotas=[60] * 17, shifts=[3] * 17), "negative cut count": dict(n_cuts=-1),
        "no frames": dict(n=0), "negative frames": dict(n=-1), "too many frames": dict(n=65536),
        "null quotas": dict(quotas=None, n_cuts=2), "null data": dict(d_data=None), "null lens": dict(d_lens=None),
        "null out": dict(d_out=None), "null sizes": dict(d_sizes=None), "null rcs": dict(d_rcs=None), "null workspace": dict(d_workspace=None),
        "stride below the largest quota": dict(out_stride=mq - 1), "workspace one byte short": dict(workspace_bytes=need - 1),
    }
    for what, kw in cases.items():
        assert roi_call(r, blob, offsets, lens, rects, cuts, **kw)[0] == INVALID_INPUT, what
    assert roi_call(r, blob, offsets, lens, rects, cuts, data_bytes=0xFFFFFFFF - 64)[0] == FATAL
    assert r.lib.icerx_recut_device_roi_async(None, n, blob.ctypes.data, len(blob), None, 0, None, None, None, None, None, 1, None, 0, None,
                                              None, None, None, None, 0, None) == INVALID_INPUT
    assert r.roi_workspace_bytes(n, len(blob), 0) == 0 == r.roi_workspace_bytes(n, len(blob), 17)
    # a plain recutter: reduces NULL or all 0 serve, a reduce above 0 is refused
    plain = trm.recutter(mock_lib, g)
    zero = [(0, q, s) for _, q, s in cuts]
    a = roi_call(plain, blob, offsets, lens, rects, zero, null_reduces=True)
    assert a[0] == 0 and a == roi_call(plain, blob, offsets, lens, rects, zero) == roi_call(r, blob, offsets, lens, rects, zero)
    assert roi_call(plain, blob, offsets, lens, rects, zero[:-1] + [(1, 60, 0)])[0] == INVALID_INPUT, "a plain recutter refuses reduce 1"
    # the existing calls of the same recutters are what they were
    assert tcm.cuts_call(r, blob, offsets, lens, [(c[0], c[1]) for c in cuts])[0] == 0
    plain.close()
    r.close()
