"""The window decode on the GPU (include/icer_hip_dec_window.h; Decoder.decode_window_host / _device / decode_window_torch,
decoder.decompress(window=...)): the cases of tests/test_window_mock.py at the same small shapes through the real library,
against tests/window_model.py -- the crop of what the plain call delivers, and the model's chain counts -- then one 512 x 384
(and 511 x 383) case per filter class, whose windows cross the blocks of the new inverse kernels, two asynchronous calls in
flight on two streams, and the asynchronous call captured in a graph on a non-null stream and replayed beside a second call."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import Oracle
from tests import recon_model as rcm
from tests import reduced_cases as rc_
from tests import window_model as wm
from tests.decoder_batch_cases import oracle_decode
from tests.test_decoder_async_emu import _batch
from tests.test_display_mock import JUNK
from tests.test_gpu_display import junk_rows, rows_back
from tests.test_window_mock import check_window, pick_windows

pytestmark = pytest.mark.gpu

_sz = C.c_size_t


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def dec():
    from icer_compression_amd import decoder
    decoder.load_library()
    return decoder


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _decoder(dec, b, reconstruct=0):
    return dec.Decoder(b.channels, b.stages, b.filt, b.segments, bits=b.bits, reduce=getattr(b, "r", 0), reconstruct=reconstruct)


def gpu_call(torch):
    """window_call of tests/test_window_mock.py for device memory: "host" icerx_decode_host_window, "sync" the device call on
    raw pointers, "async" Decoder.decode_window_torch on a stream of its own"""
    def call(kind, d, b, wins, frame_stride, full_stride, display=False):
        blob, offs, lens = d._pack(b.streams)
        n, ch = len(b.streams), b.channels
        dt = np.uint8 if display or b.bits == 8 else np.uint16
        size = dt().itemsize
        if kind == "host":
            rc, res = d.decode_window_host(b.streams, wins, frame_stride, full_stride)
            assert rc == 0, rc
            # (the wrapper's planes start out zero: junk behind the windows is the mock test's business)
            junk = JUNK if dt == np.uint8 else JUNK * 0x0101
            rows = {}
            for k, (rck, w, h, planes, info) in enumerate(res):
                for c in range(ch):
                    nwin = 0 if rck == wm.QUOTA else info[2] * info[3]
                    assert not planes[c][nwin:].any(), (k, c, "written behind the window")
                    rows[(k, c)] = np.concatenate([planes[c][:nwin], np.full(frame_stride - nwin, junk, dt)])
            return [r[0] for r in res], [r[1] for r in res], [r[2] for r in res], [r[4] for r in res], lambda k, c: rows[(k, c)]
        out, raw = junk_rows(torch, n * ch * frame_stride * size)
        if kind == "sync":
            d_blob = torch.from_numpy(blob).cuda()
            torch.cuda.synchronize()
            rc, rcs, ws, hs, info = d.decode_window_device(n, d_blob.data_ptr(), offs, lens, wins, out.data_ptr(), frame_stride, full_stride, display)
            assert rc == 0, rc
            assert np.array_equal(d_blob.cpu().numpy(), blob), "the input was written"
        else:
            st = torch.cuda.Stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                d_blob = torch.from_numpy(blob).cuda()
                ln = torch.tensor([int(x) for x in lens], dtype=torch.int64, device="cuda")
                of = torch.tensor([int(x) for x in offs], dtype=torch.int64, device="cuda")
                t_rcs = torch.full((n,), 77, dtype=torch.int32, device="cuda")
                t_ws, t_hs = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
                t_win = torch.tensor(np.asarray(wins, np.int64).reshape(n, 4), device="cuda").to(torch.int32)       # (written on the stream)
                t_info = torch.full((n, 6), -1, dtype=torch.int32, device="cuda")
                d.decode_window_torch(d_blob, ln, out if dt == np.uint8 else out.view(torch.int16), t_rcs, t_ws, t_hs, t_win, t_info,
                                      full_stride, offsets=of, display=display)
            st.synchronize()
            rcs, ws, hs, info = t_rcs.cpu().tolist(), t_ws.cpu().tolist(), t_hs.cpu().tolist(), t_info.cpu().tolist()
        flat = np.concatenate(rows_back(out, raw, n, ch * frame_stride * size)).view(dt)
        if display:
            return rcs, ws, hs, info, lambda k, c: flat[k * ch * frame_stride: (k + 1) * ch * frame_stride]
        return rcs, ws, hs, info, lambda k, c: flat[(k * ch + c) * frame_stride: (k * ch + c + 1) * frame_stride]
    return call


# ---------------------------------------------------------------------------------------------- the mock test's cases
@pytest.mark.parametrize("filt", [0, 2, 6])
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (1, 8), (3, 8)])
def test_window_mixed_batches(dec, orc, torch, ch, bits, filt):
    b = _batch(orc, ch, bits, filt)
    d = _decoder(dec, b)
    wins = pick_windows(b)
    seen, run, full = check_window(orc, d, b, wins, ("host", "sync", "async"), label=f"ch {ch} bits {bits} filt {filt}", call=gpu_call(torch))
    assert seen >= 5 and run < full
    check_window(orc, d, b, pick_windows(b, 5), ("sync", "async"), display=True, label=f"ch {ch} bits {bits} filt {filt}", call=gpu_call(torch))
    d.close()


def test_window_reduced_and_reconstructed(dec, orc, torch):
    for r, (ch, bits, filt) in ((1, (1, 16, 0)), (2, (3, 16, 4)), (1, (1, 8, 0))):
        b = rc_.of_batch(orc, _batch(orc, ch, bits, filt), r)
        d = _decoder(dec, b)
        check_window(orc, d, b, pick_windows(b, r), ("sync", "async"), label=f"r {r} filt {filt}", call=gpu_call(torch))
        check_window(orc, d, b, pick_windows(b, r + 3), ("async",), display=True, label=f"r {r} filt {filt}", call=gpu_call(torch))
        d.close()
    b = _batch(orc, 3, 16, 1)
    want = [rcm.expected(orc, s, 3, 3, b.stages, 1, b.segments, b.stride, 16) for s in b.streams]
    d = _decoder(dec, b, reconstruct=3)
    check_window(orc, d, b, pick_windows(b, 1), ("sync", "async"), label="recon 3", want=want, call=gpu_call(torch))
    d.close()


def test_window_tight_stride_and_early_stops(dec, orc, torch):
    b = _batch(orc, 3, 16, 0)
    wins = pick_windows(b)
    areas = sorted({wm.clip(wins[k], w, h)[2] * wm.clip(wins[k], w, h)[3] for k, (rc, w, h, _) in enumerate(b.want) if wm.delivered(rc, w, h, b.stride)})
    d = _decoder(dec, b)
    for display in (False, True):
        seen, _, _ = check_window(orc, d, b, wins, ("sync", "async"), frame_stride=areas[len(areas) // 2], display=display, label="tight stride",
                                  call=gpu_call(torch))
        assert seen >= 2
    d.close()
    for b in (rc_.too_many_segments_batch(orc), rc_.thin_ll_batch(orc)):
        d = _decoder(dec, b)
        check_window(orc, d, b, pick_windows(b, 3), ("host", "sync", "async"), label="early stop", call=gpu_call(torch))
        d.close()


# ---------------------------------------------------------------------------------------------- chains are skipped
class OneBatch:
    """a batch of lossless streams of one w x h image, shaped like decoder_batch_cases.Batch for check_window"""

    def __init__(self, orc, w, h, ch, stages, filt, segments, n=1, bits=16):
        self.channels, self.bits, self.filt, self.stages, self.segments = ch, bits, filt, stages, segments
        self.streams = [rc_.encode(orc, rc_.planes(w, h, ch, 10 + k, bits), stages, filt, segments, None, bits) for k in range(n)]
        self.entries = [(w, h, "lossless")] * n
        self.stride = w * h
        self.want = [oracle_decode(orc, s, ch, stages, filt, segments, self.stride, bits) for s in self.streams]
        assert all(x[:3] == (0, w, h) for x in self.want)


def test_interior_window_runs_fewer_chains(dec, orc, torch):
    """filter A, 128 x 96, 3 stages, 8 segments, a 16 x 16 interior window: chains run strictly below chains in full"""
    b = OneBatch(orc, 128, 96, 1, 3, 0, 8)
    d = _decoder(dec, b)
    for kind in ("sync", "async"):
        rcs, ws, hs, info, row = gpu_call(torch)(kind, d, b, [(56, 40, 16, 16)], 256, b.stride)
        assert rcs == [0] and tuple(info[0][:4]) == (56, 40, 16, 16) and 0 < info[0][4] < info[0][5], info
    check_window(orc, d, b, [(56, 40, 16, 16)], ("host", "sync", "async"), frame_stride=256, label="interior", call=gpu_call(torch))
    d.close()


_LARGE = {}


@pytest.mark.parametrize("filt", [0, 1, 2, 6], ids=["A", "B", "C", "Q"])
def test_window_large_frames(dec, orc, torch, filt):
    """512 x 384 and 511 x 383 at 4 stages and 6 segments, YUV: windows that start at odd coordinates, end on the last sample of
    an odd line, cross the 64-wide and 256-item blocks of the inverse kernels, and the whole frame"""
    for w, h in ((512, 384), (511, 383)):
        if (w, h, filt) not in _LARGE:
            _LARGE[(w, h, filt)] = OneBatch(orc, w, h, 3, 4, filt, 6, n=4)
        b = _LARGE[(w, h, filt)]
        d = _decoder(dec, b)
        wins = [(129, 67, 200, 131), (w - 77, h - 93, 77, 93), (1, h - 2, w - 1, 2), (0, 0, w, h)]
        seen, run, full = check_window(orc, d, b, wins, ("sync", "async"), label=f"{w}x{h} filt {filt}", call=gpu_call(torch))
        assert seen == 4 and run < full
        check_window(orc, d, b, wins[1:] + wins[:1], ("async",), display=True, label=f"{w}x{h} filt {filt}", call=gpu_call(torch))
        d.close()


def test_decompress_window_one_shot(dec, orc, torch):
    b = _batch(orc, 3, 16, 0)
    k = next(k for k, (rc, w, h, _) in enumerate(b.want) if rc == 0 and wm.delivered(rc, w, h, b.stride))
    rc, w, h, planes = b.want[k]
    win = (w // 3, h // 4, w // 2, h // 2)
    e_rc, clip, crop, run, full = wm.expected(orc, b.want[k], win, win[2] * win[3], w * h, 3, b.stages, b.filt, b.segments, 16, b.streams[k])
    got = dec.decompress(b.streams[k], 3, b.stages, b.filt, b.segments, window=win)
    assert got[:3] == (e_rc, w, h) and got[4] == list(clip) + [run, full] and run < full
    assert all(np.array_equal(g, c.reshape(-1)) for g, c in zip(got[3], crop))


# ---------------------------------------------------------------------------------------------- two calls in flight
def test_two_window_calls_in_flight_on_two_streams(dec, orc, torch):
    """two decoders, a non-null stream each, the second call enqueued while the first is held back by a sleep on its stream;
    the windows are written by a torch kernel on the same stream just before, and nothing waits in between"""
    b = _batch(orc, 1, 16, 0)
    n, stride = len(b.streams), b.stride
    decs = [_decoder(dec, b), _decoder(dec, b)]
    runs = []
    torch.cuda.synchronize()
    for k, st in enumerate((torch.cuda.Stream(), torch.cuda.Stream())):
        wins = pick_windows(b, 3 * k)
        blob, offs, lens = decs[k]._pack(b.streams)
        with torch.cuda.stream(st):
            d_blob = torch.from_numpy(blob).cuda()
            ln = torch.tensor([int(x) for x in lens], dtype=torch.int64, device="cuda")
            of = torch.tensor([int(x) for x in offs], dtype=torch.int64, device="cuda")
            out = torch.full((n, 2 * stride), JUNK, dtype=torch.uint8, device="cuda").view(torch.int16)
            t_rcs = torch.full((n,), 77, dtype=torch.int32, device="cuda")
            t_ws, t_hs = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
            t_info = torch.full((n, 6), -1, dtype=torch.int32, device="cuda")
            torch.cuda._sleep(int(5e-3 * 2.1e9))
            t_win = (torch.tensor(np.asarray(wins, np.int64), device="cuda") + 0).to(torch.int32)
            decs[k].decode_window_torch(d_blob, ln, out, t_rcs, t_ws, t_hs, t_win, t_info, stride, offsets=of)
        runs.append((wins, out, t_rcs, t_info, d_blob))
    torch.cuda.synchronize()
    for wins, out, t_rcs, t_info, _ in runs:
        flat = out.cpu().numpy().view(np.uint16)
        for k in range(n):
            rc, clip, crop, run, full = wm.expected(orc, b.want[k], wins[k], stride, stride, 1, b.stages, b.filt, b.segments, 16, b.streams[k])
            assert int(t_rcs[k]) == rc and tuple(t_info[k, :4].tolist()) == clip, (k, int(t_rcs[k]), rc)
            nwin = 0 if crop is None else crop[0].size
            assert (flat[k][nwin:] == JUNK * 0x0101).all() and (crop is None or np.array_equal(flat[k][:nwin], crop[0].reshape(-1))), k
    for d in decs:
        d.close()


def test_window_call_captured_in_a_graph_and_replayed_beside_a_call_in_flight(dec, orc, torch):
    """The stream-ordered promise, held to its word: after one warm-up call (which makes the decoder's side streams and events and
    the stream's cached workspace) decode_window_torch is CAPTURED on a non-null stream -- a blocking copy, a synchronisation, an
    allocation or a lazily made stream inside icerx_decode_device_window_async would end the capture with an error -- and nothing
    runs while it is captured.  The graph is then replayed with other windows in the same device tensor, while a second decoder's
    call is in flight on another stream; both results are the model's."""
    b = _batch(orc, 1, 16, 0)
    n, stride = len(b.streams), b.stride
    junk = JUNK * 0x0101
    d1, d2 = _decoder(dec, b), _decoder(dec, b)
    wins = [pick_windows(b, 0), pick_windows(b, 4), pick_windows(b, 9)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def tensors(st, d):
        blob, offs, lens = d._pack(b.streams)
        with torch.cuda.stream(st):
            t = {"blob": torch.from_numpy(blob).cuda(), "lens": torch.tensor([int(x) for x in lens], dtype=torch.int64, device="cuda"),
                 "offs": torch.tensor([int(x) for x in offs], dtype=torch.int64, device="cuda"),
                 "out": torch.full((n, 2 * stride), JUNK, dtype=torch.uint8, device="cuda").view(torch.int16),
                 "rcs": torch.full((n,), 77, dtype=torch.int32, device="cuda"), "ws": torch.zeros(n, dtype=torch.int64, device="cuda"),
                 "hs": torch.zeros(n, dtype=torch.int64, device="cuda"), "win": torch.zeros((n, 4), dtype=torch.int32, device="cuda"),
                 "info": torch.full((n, 6), -1, dtype=torch.int32, device="cuda")}
        st.synchronize()
        return t

    def call(d, t):
        d.decode_window_torch(t["blob"], t["lens"], t["out"], t["rcs"], t["ws"], t["hs"], t["win"], t["info"], stride, offsets=t["offs"])

    def set_windows(t, w):
        t["win"].copy_(torch.tensor(np.asarray(w, np.int64), device="cuda").to(torch.int32))
        t["out"].view(torch.uint8).fill_(JUNK)
        t["info"].fill_(-1)
        torch.cuda.synchronize()

    def check(t, w, label):
        flat, rcs, info = t["out"].cpu().numpy().view(np.uint16), t["rcs"].cpu().tolist(), t["info"].cpu().tolist()
        for k in range(n):
            rc, clip, crop, run, full = wm.expected(orc, b.want[k], w[k], stride, stride, 1, b.stages, b.filt, b.segments, 16, b.streams[k])
            assert rcs[k] == rc and tuple(info[k][:4]) == clip, (label, k, rcs[k], rc, info[k], clip)
            if full is not None:
                assert (info[k][4], info[k][5]) == (run, full), (label, k, info[k], run, full)
            nwin = 0 if crop is None else crop[0].size
            assert (flat[k][nwin:] == junk).all() and (crop is None or np.array_equal(flat[k][:nwin], crop[0].reshape(-1))), (label, k)

    t1, t2 = tensors(s1, d1), tensors(s2, d2)
    set_windows(t1, wins[0])
    with torch.cuda.stream(s1):                            # the warm-up, on the stream of the capture
        call(d1, t1)
    s1.synchronize()
    check(t1, wins[0], "warm-up")
    set_windows(t1, wins[1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s1):
        call(d1, t1)
    torch.cuda.synchronize()
    assert (t1["out"].cpu().numpy().view(np.uint16) == junk).all() and (t1["info"].cpu().numpy() == -1).all(), "the captured call ran"
    for rnd, w in enumerate(wins[1:]):                     # two replays, the windows changed in place in between
        set_windows(t1, w)
        set_windows(t2, wins[0])
        with torch.cuda.stream(s2):
            torch.cuda._sleep(int(2e-3 * 2.1e9))
            call(d2, t2)
        with torch.cuda.stream(s1):
            graph.replay()
        torch.cuda.synchronize()
        check(t1, w, f"replay {rnd}")
        check(t2, wins[0], f"beside replay {rnd}")
    del graph
    d1.close()
    d2.close()
