"""Region-of-interest encode on the GPU (icerx_encode_device_roi, include/icer_hip.h) on the cases of tests/roi_cases.py.  Every
stream, size, return code, K and foreground count equals what tests/roi_model.py cuts from the units of the lossless
icerx_encode_device stream of the same frames by the same encoder, and the golden digests made from the reference encoder's
lossless streams (tests/golden/roi_golden.json); nothing is written behind a stream in its row; shift 0, an empty rectangle, one
outside the frame, a foreground of every unit and an encoder of one segment give icerx_encode_device's streams byte for byte;
the project's GPU decoder decodes every stream to the image the decoder oracle gives; rectangles written by a torch kernel
on the same stream need no synchronisation; a refused call writes nothing."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from icer_compression_amd import api
from tests import encoder_batch_cases as ebc
from tests import roi_cases as rc
from tests import roi_model as rm
from tests import test_gpu_encoder_batch as tb
from tests import test_gpu_ladder as tl

pytestmark = pytest.mark.gpu

SENT, SENT_SIZE, SENT_RC = tb.SENT, tb.SENT_SIZE, tb.SENT_RC
SENT_U32 = 0x5A5A5A5A
HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "roi_golden.json")) as _fh:
    GOLDEN = json.load(_fh)


def roi_call(enc, t, rois_dev, shift, quotas):
    """icerx_encode_device_roi on the cuda tensors `t` and `rois_dev` into Q * n + 1 rows / entries filled with a sentinel (odd
    stride: rows start at every byte alignment).  Returns (res[q][f] = (rc, stream, K), foreground[f]) after checking the
    buffer promises."""
    import torch
    n, Q = t.shape[0], len(quotas)
    stride = max(quotas) + 5
    keep = t.clone()
    dev = t.device
    out = torch.full((Q * n + 1, stride), SENT, dtype=torch.uint8, device=dev)
    sizes = torch.full((Q * n + 1,), SENT_SIZE, dtype=torch.int64, device=dev)
    rcs = torch.full((Q * n + 1,), SENT_RC, dtype=torch.int32, device=dev)
    kept = torch.full((Q * n + 1,), SENT_U32, dtype=torch.int32, device=dev)
    fg = torch.full((n + 1,), SENT_U32, dtype=torch.int32, device=dev)
    enc.encode_roi_ptrs(t.data_ptr(), n, rois_dev.data_ptr(), shift, quotas, out.data_ptr(), stride, sizes.data_ptr(), rcs.data_ptr(),
                        kept.data_ptr(), fg.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(t, keep), "the input frames were modified on the device"
    out, sizes, rcs, kept, fg = out.cpu().numpy(), sizes.cpu().numpy(), rcs.cpu().numpy(), kept.cpu().numpy(), fg.cpu().numpy()
    assert (out[Q * n] == SENT).all(), "bytes written past the Q * n rows of the output"
    assert int(sizes[Q * n]) == SENT_SIZE and int(rcs[Q * n]) == SENT_RC and int(kept[Q * n]) == SENT_U32, "entries written past Q * n"
    assert int(fg[n]) == SENT_U32, "foreground counts written past n entries"
    res = []
    for q, quota in enumerate(quotas):
        row = []
        for f in range(n):
            k = q * n + f
            s = int(sizes[k])
            assert 0 <= s <= quota, (q, f, s, quota)
            assert (out[k, s:] == SENT).all(), f"quota {q} frame {f}: bytes written behind its stream of {s} bytes"
            row.append((int(rcs[k]), out[k, :s].tobytes(), int(kept[k])))
        res.append(row)
    return res, [int(x) for x in fg[:n]]


def rois_tensor(rects, dev):
    import torch
    return torch.tensor(rects, dtype=torch.int64, device=dev).to(torch.int32)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", list(rc.GEOMETRIES))
def test_roi_streams_equal_the_model(name, oracle):
    import torch
    from icer_compression_amd import decoder
    decoder.load_library()
    g, m, quotas = rc.GEOMETRIES[name], rc.model(name), rc.quotas(name)
    dev = torch.device("cuda", 0)
    decoded = {}                                                            # stream -> checked against the decoder oracle
    for b, specs in enumerate(rc.BATCHES[name]):
        enc = api.Encoder(g.w, g.h, g.channels, g.stages, g.filt, g.segments, max_frames=rc.MAX_FRAMES[b], sample_bits=g.bits)
        t = tl.device_frames(ebc.batch(g, specs))
        rects = rc.rectangles(name, b)
        rois = rois_tensor(rects, dev)
        n = len(specs)
        # the encoder's own lossless streams and its streams at every quota
        plain = {q: tl.separate(enc, t, q) for q in sorted(set(quotas))}
        lossless = plain[quotas[0]]
        for f, spec in enumerate(specs):
            assert lossless[f][0] == (0 if rc.has_stream(spec) else -1), (name, b, f, lossless[f][0])
        for shift in rc.SHIFTS:
            got, fg = roi_call(enc, t, rois, shift, quotas)
            if b == 1:
                assert enc.parts() == 2, enc.parts()                       # (the five frames went in two parts on two streams)
            gold = GOLDEN[rc.golden_key(name, b, shift)]
            for f, spec in enumerate(specs):
                what = f"{name} batch {b} shift {shift} frame {f} {spec} rectangle {rects[f]}"
                if not rc.has_stream(spec):
                    assert fg[f] == rm.roi_order(m, rects[f], shift)[2] == gold["foreground"][f], what
                    for q in range(len(quotas)):
                        assert got[q][f] == (-1, b"", 0), (what, q)
                    continue
                want, n_fg = rm.roi_streams(m, lossless[f][1], rects[f], shift, quotas)
                assert fg[f] == n_fg == gold["foreground"][f], (what, fg[f], n_fg)
                identity = shift == 0 or rc.RECT_KINDS[((0, 3)[b] + f) % 6] in ("empty", "outside") or n_fg == m.n_units or g.segments == 1
                for q, quota in enumerate(quotas):
                    code, stream, K = got[q][f]
                    w_stream, w_code, w_K = want[q]
                    assert (code, K, len(stream)) == (w_code, w_K, len(w_stream)), (what, quota, code, K, len(stream), w_code, w_K, len(w_stream))
                    assert stream == w_stream, f"{what} quota {quota}: first difference at byte {ebc.first_difference(stream, w_stream)}"
                    assert (len(stream), code, K, hashlib.sha256(stream).hexdigest()[:16]) == \
                        (gold["size"][q][f], gold["rc"][q][f], gold["kept"][q][f], gold["sha256_16"][q][f]), (what, quota)
                    if identity:
                        assert (code, stream) == plain[quota][f], (what, quota)
                    if quota == quotas[0]:
                        assert (code, stream) == lossless[f], (what, "a quota that keeps every unit gives the lossless stream")
                    decoded.setdefault(stream, what)
        assert enc.stats()["unit_timeouts"] == 0
        enc.close()
    # every distinct stream through the project's decoder and the decoder oracle
    streams = [s for s in decoded if s]
    d = decoder.Decoder(g.channels, g.stages, g.filt, g.segments, bits=g.bits)
    code, res = d.decode_host(streams, g.w * g.h)
    assert code == 0
    for s, (rk, wk, hk, planes) in zip(streams, res):
        want = oracle.decompress(s, g.channels, g.stages, g.filt, g.segments, bufsize=g.w * g.h, bits=g.bits)
        assert (rk, wk, hk) == want[:3] and rk == 0, (decoded[s], rk, want[0])
        for c in range(g.channels):
            assert np.array_equal(planes[c][: wk * hk], want[3][c][: wk * hk]), (decoded[s], c)
    d.close()


@pytest.mark.timeout(300)
def test_rectangles_written_on_the_stream_and_torch_entry():
    """the rectangles come out of a torch kernel enqueued just before the call, with no synchronisation in between; and
    Encoder.encode_roi_torch gives the same streams as the pointer entry"""
    import torch
    name, b, shift = "G1", 1, 3
    g, quotas = rc.GEOMETRIES[name], rc.quotas(name)
    dev = torch.device("cuda", 0)
    enc = api.Encoder(g.w, g.h, g.channels, g.stages, g.filt, g.segments, max_frames=8)
    t = tl.device_frames(ebc.batch(g, rc.BATCHES[name][b]))
    rects = rc.rectangles(name, b)
    want, want_fg = roi_call(enc, t, rois_tensor(rects, dev), shift, quotas)
    base = torch.tensor(rects, dtype=torch.int64, device=dev)
    big = torch.ones((2048, 2048), device=dev)
    torch.cuda.synchronize()
    for _ in range(4):
        big = big @ big * 1e-4                                              # (work in front of the kernel that writes the rectangles)
    rois = ((base * 3 + 7 - 7) // 3).to(torch.int32)
    out, sizes, rcs, kept, fg = enc.encode_roi_torch(t, rois, shift, quotas)
    torch.cuda.synchronize()
    assert [int(x) for x in fg.cpu()] == want_fg
    for q in range(len(quotas)):
        for f in range(t.shape[0]):
            s = int(sizes[q, f])
            assert (int(rcs[q, f]), out[q, f, :s].cpu().numpy().tobytes(), int(kept[q, f])) == want[q][f], (q, f)
    enc.close()


@pytest.mark.timeout(300)
def test_roi_slot_retry(monkeypatch):
    """slots of 1 bit per sample: the noise frame outgrows them, the ranked walk stops at such a unit, the batch is redone with
    larger slots and every quota's streams are cut again"""
    import torch
    from tests import target_model as tm
    monkeypatch.setenv("ICER_HIP_SLOT_BPP", "1")
    g = ebc.Geometry(256, 256, 1, 2, 0, 2)
    m = tm.Model(g.w, g.h, 1, g.stages, g.filt, g.segments, 16)
    enc = api.Encoder(g.w, g.h, 1, g.stages, g.filt, g.segments, max_frames=4)
    assert enc.info()["slot_bits_per_pixel"] == 1
    specs = [("blank", 0), ("flat", 0), ("noise8", 0), ("dot", 0)]
    quotas = [ebc.quota(g, c) for c in ("cut", "lossless", "tiny60", "progressive")]
    rects = [(0, 0, 40, 40), (200, 190, 56, 66), (30, 20, 50, 20), (128, 200, 1, 56)]
    t = tl.device_frames(ebc.batch(g, specs))
    got, fg = roi_call(enc, t, rois_tensor(rects, torch.device("cuda", 0)), 3, quotas)
    assert enc.stats()["slot_retries"] >= 1 and enc.info()["slot_bits_per_pixel"] > 1, (enc.stats(), enc.info())
    lossless = tl.separate(enc, t, quotas[1])
    for f in range(len(specs)):
        assert lossless[f][0] == 0
        want, n_fg = rm.roi_streams(m, lossless[f][1], rects[f], 3, quotas)
        assert fg[f] == n_fg
        for q in range(len(quotas)):
            assert got[q][f] == (want[q][1], want[q][0], want[q][2]), (f, q)
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()


@pytest.mark.timeout(300)
def test_invalid_roi_calls_write_nothing():
    import torch
    name = "G1"
    g, quotas = rc.GEOMETRIES[name], rc.quotas(name)[:3]
    dev = torch.device("cuda", 0)
    enc = api.Encoder(g.w, g.h, 1, g.stages, g.filt, g.segments, max_frames=3)
    t = tl.device_frames(ebc.batch(g, rc.BATCHES[name][0]))
    rois = rois_tensor(rc.rectangles(name, 0), dev)
    Q, n, stride = len(quotas), 3, max(quotas) + 5
    out = torch.full((Q * n, stride), SENT, dtype=torch.uint8, device=dev)
    sizes = torch.full((Q * n,), SENT_SIZE, dtype=torch.int64, device=dev)
    rcs = torch.full((Q * n,), SENT_RC, dtype=torch.int32, device=dev)
    kept = torch.full((Q * n,), SENT_U32, dtype=torch.int32, device=dev)
    fg = torch.full((n,), SENT_U32, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    L = enc.lib

    def call(handle=enc.handle, frames=t.data_ptr(), nf=n, r=rois.data_ptr(), shift=3, qs=quotas, nq=None, o=out.data_ptr(), s=stride,
             sz=sizes.data_ptr(), code=rcs.data_ptr(), k=kept.data_ptr(), f=fg.data_ptr()):
        arr = None if qs is None else (C.c_size_t * max(len(qs), 1))(*qs)
        return L.icerx_encode_device_roi(handle, frames, nf, r, shift, arr, len(qs) if nq is None else nq, o, s, sz, code, k, f, st)

    cases = {
        "no quotas": dict(nq=0), "17 quotas": dict(qs=[quotas[0]] * 17), "null encoder": dict(handle=None), "null frames": dict(frames=None),
        "null rectangles": dict(r=None), "null quotas": dict(qs=None, nq=2), "null out": dict(o=None), "null sizes": dict(sz=None),
        "null rcs": dict(code=None), "null kept": dict(k=None), "null foreground": dict(f=None), "no frames": dict(nf=0),
        "too many frames": dict(nf=4), "shift 17": dict(shift=17), "negative shift": dict(shift=-1),
        "stride below the largest quota": dict(s=min(quotas) + 5),
    }
    for what, kw in cases.items():
        assert call(**kw) == api.ICER_INVALID_INPUT, what
    torch.cuda.synchronize()
    assert (out == SENT).all().item() and (sizes == SENT_SIZE).all().item() and (rcs == SENT_RC).all().item(), "a refused call wrote"
    assert (kept == SENT_U32).all().item() and (fg == SENT_U32).all().item(), "a refused call wrote"
    assert call() == 0 and call(shift=0) == 0 and call(shift=16) == 0
    torch.cuda.synchronize()
    assert not (sizes == SENT_SIZE).any().item()
    enc.close()
