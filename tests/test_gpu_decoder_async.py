"""icerx_decode_device_async / Decoder.decode_torch on the GPU (icer_compression_amd/csrc/decoder_async.hpp): the batches of
tests/test_gpu_decoder_batch.py through the stream-ordered call on a non-default torch stream, into outputs filled with junk,
frame by frame against the decoder oracle and with rcs / ws / hs equal to icerx_decode_device's; the encoder's device output
decoded without the host; asynchrony; two calls in flight; call- and frame-level errors.  (The same planner and pipeline run
on the CPU in tests/test_decoder_plan_device.py and tests/test_decoder_async_emu.py.)
"""
import os

import numpy as np
import pytest

from oracle.binding import Oracle
from tests import decoder_batch_cases as dbc

pytestmark = pytest.mark.gpu


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


@pytest.fixture(params=[None, "0", "1", "2"], ids=["by-load", "thread-per-chain", "wave-per-chain", "wave-per-plane"])
def kernel(request):
    old = os.environ.get("ICER_DEC_WAVE")
    if request.param is None:
        os.environ.pop("ICER_DEC_WAVE", None)
    else:
        os.environ["ICER_DEC_WAVE"] = request.param
    yield request.param
    if old is None:
        os.environ.pop("ICER_DEC_WAVE", None)
    else:
        os.environ["ICER_DEC_WAVE"] = old


def tensors(torch, n, channels, stride, bits, w_in=None, h_in=None, junk=0x5A):
    dt = torch.int16 if bits == 16 else torch.uint8
    out = torch.full((n, channels, stride), junk, dtype=dt, device="cuda")
    rcs = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    ws = torch.tensor(w_in if w_in is not None else [0] * n, dtype=torch.int64, device="cuda")
    hs = torch.tensor(h_in if h_in is not None else [0] * n, dtype=torch.int64, device="cuda")
    return out, rcs, ws, hs


def out_np(out, bits):
    a = out.cpu().numpy()
    return (a.view(np.uint16) if bits == 16 else a).reshape(-1)


def decode_async(torch, d, blob, offsets, lens, stride, w_in=None, h_in=None, stream=None):
    """decode_torch on `stream` (a new non-default stream when None); -> (rcs, ws, hs, flat output) after a synchronise"""
    n = len(lens)
    st = stream or torch.cuda.Stream()
    with torch.cuda.stream(st):
        data = torch.from_numpy(np.asarray(blob, np.uint8)).to("cuda", non_blocking=False)
        ln = torch.tensor([int(x) for x in lens], dtype=torch.int64, device="cuda")
        offs = torch.tensor([int(x) for x in offsets], dtype=torch.int64, device="cuda")
        out, rcs, ws, hs = tensors(torch, n, d.channels, stride, d.bits, w_in, h_in)
        d.decode_torch(data, ln, out, rcs, ws, hs, offsets=offs)
    st.synchronize()
    return rcs.cpu().tolist(), ws.cpu().tolist(), hs.cpu().tolist(), out_np(out, d.bits)


def check_batch(torch, dec, b, label):
    d = dec.Decoder(b.channels, b.stages, b.filt, b.segments, bits=b.bits)
    try:
        blob, offs, lens = d._pack(b.streams)
        n, ch, stride = len(b.streams), b.channels, b.stride
        rcs, ws, hs, out = decode_async(torch, d, blob, list(offs), list(lens), stride)
        b.check(rcs, ws, hs, lambda k, c: out[(k * ch + c) * stride:], label + " async")
        d_blob = torch.from_numpy(blob).cuda()
        sync_out = torch.zeros(n * ch * stride * (2 if b.bits == 16 else 1), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc, rcs2, ws2, hs2 = d.decode_device(n, d_blob.data_ptr(), offs, lens, sync_out.data_ptr(), stride)
        assert rc == 0 and (rcs, ws, hs) == (rcs2, ws2, hs2), label
    finally:
        d.close()


_BATCHES = {}


def cached(key, make):
    if key not in _BATCHES:
        _BATCHES[key] = make()
    return _BATCHES[key]


@pytest.mark.timeout(240)
@pytest.mark.parametrize("filt", range(7))
def test_async_batch_filters_channels_bits(dec, orc, torch, kernel, filt):
    for ch in (1, 3):
        for bits in (16, 8):
            b = cached(("mixed", filt, ch, bits), lambda: dbc.mixed_batch(orc, ch, bits, filt))
            check_batch(torch, dec, b, f"filt {filt} ch {ch} bits {bits} mode {kernel}")


@pytest.mark.timeout(420)
def test_async_batch_past_the_load_threshold(dec, orc, torch, kernel):
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count

    def make():
        specs = [((1024, 1024, "noise", 1), dbc.LOSSLESS), ((1024, 1024, "smooth", 2), dbc.LOSSLESS),
                 ((1024, 1024, "noise", 3), dbc.CUT)]
        probe = dbc.Batch(orc, 1, 16, 1, 4, 32, [(s, q, None) for s, q in specs], check_reference=False)
        per = min(dbc.chains_in(s, 1) for s in probe.streams)
        reps = (2 * 12 * n_cus + per - 1) // per // len(specs) + 1
        return dbc.Batch(orc, 1, 16, 1, 4, 32, [(s, q, None) for _ in range(reps) for s, q in specs])
    check_batch(torch, dec, cached(("load", n_cus), make), f"load mode {kernel}")


@pytest.mark.timeout(300)
def test_async_wide_and_narrow_chains_in_one_call(dec, orc, torch, kernel):
    narrow = [(6, 180), (9, 150), (7, 96), (12, 200), (5, 64), (40, 130)]

    def make():
        entries = [((4096, 256, "noise", 9), dbc.LOSSLESS, None)]
        for i, (w, h) in enumerate(narrow):
            entries.append(((w, h, "noise", 20 + i), dbc.LOSSLESS if i % 2 == 0 else dbc.CUT, None))
        entries.insert(4, ((4096, 256, "smooth", 10), dbc.CUT, None))
        return dbc.Batch(orc, 1, 16, 0, 1, 1, entries)
    check_batch(torch, dec, cached("wide", make), f"wide mode {kernel}")


@pytest.mark.timeout(120)
def test_async_second_header_pass(dec, orc, torch, kernel):
    check_batch(torch, dec, cached("headers", lambda: dbc.header_pass_batch(orc, frames=6)), f"headers mode {kernel}")


@pytest.mark.timeout(180)
@pytest.mark.parametrize("bits", [16, 8])
def test_async_decoder_reused_across_calls(dec, orc, torch, bits):
    large, small = cached(("reuse", bits), lambda: dbc.reuse_batches(orc, bits))
    for k, b in enumerate((large, small, large)):
        check_batch(torch, dec, b, f"call {k}")


@pytest.mark.timeout(180)
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 8), (3, 16)])
def test_async_blob_layout(dec, orc, torch, ch, bits):
    layout = cached(("layout", ch, bits), lambda: dbc.Layout(orc, dbc.mixed_batch(orc, ch, bits, 4, seed=5)))
    b = layout.batch
    d = dec.Decoder(ch, b.stages, b.filt, b.segments, bits=bits)
    try:
        rcs, ws, hs, out = decode_async(torch, d, layout.blob, layout.offsets, layout.lens, b.stride, layout.w_in, layout.h_in)
        layout.check(rcs, ws, hs, lambda k, c: out[(k * ch + c) * b.stride:], "async")
    finally:
        d.close()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (1, 8), (3, 8)])
def test_encode_then_decode_without_the_host(dec, torch, ch, bits):
    """encode_torch (icerx_encode_device / _s8) a lossless batch, then decode_torch of its d_out / d_sizes on the same
    stream (offsets = k * out_stride); one synchronise at the end; the output is the input (filter A, even sides)"""
    from icer_compression_amd import api
    n, w, h, stages, segments = 5, 96, 64, 3, 6
    rng = np.random.default_rng(ch * 100 + bits)
    top = 60 if bits == 16 else 24
    frames = rng.integers(0, top, (n, ch, h, w)).astype(np.uint16 if bits == 16 else np.uint8)
    quota = 4 * w * h * ch + 32 * 9 * (3 * stages + 1) * segments * ch
    enc = api.Encoder(w, h, channels=ch, stages=stages, filt=0, segments=segments, max_frames=n, sample_bits=bits)
    d = dec.Decoder(ch, stages, 0, segments, bits=bits)
    st = torch.cuda.Stream()
    try:
        with torch.cuda.stream(st):
            src = torch.from_numpy(frames.view(np.int16) if bits == 16 else frames).to("cuda")
            out_stride = quota + 64
            streams = torch.zeros((n, out_stride), dtype=torch.uint8, device="cuda")
            sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
            enc_rcs = torch.full((n,), 99, dtype=torch.int32, device="cuda")
            if bits == 16:
                enc.encode_torch(src, quota, streams, sizes, enc_rcs)
            else:
                rc = enc.lib.icerx_encode_device_s8(enc.handle, src.data_ptr(), n, quota, streams.data_ptr(), out_stride,
                                                    sizes.data_ptr(), enc_rcs.data_ptr(), st.cuda_stream)
                assert rc == 0
            planes, rcs, ws, hs = tensors(torch, n, ch, w * h, bits)
            d.decode_torch(streams, sizes, planes, rcs, ws, hs)
        st.synchronize()
        assert enc_rcs.cpu().tolist() == [0] * n
        assert rcs.cpu().tolist() == [0] * n and ws.cpu().tolist() == [w] * n and hs.cpu().tolist() == [h] * n
        got = out_np(planes, bits).reshape(n, ch, h, w)
        assert np.array_equal(got, frames)
    finally:
        d.close()
        enc.close()


@pytest.mark.timeout(120)
def test_call_returns_before_the_work_is_done(dec, orc, torch):
    """a ~50 ms sleep on the stream ahead of the call: the call returns while an event recorded after it is pending"""
    b = cached(("mixed", 0, 1, 16), lambda: dbc.mixed_batch(orc, 1, 16, 0))
    d = dec.Decoder(1, b.stages, b.filt, b.segments, bits=16)
    try:
        blob, offs, lens = d._pack(b.streams)
        n = len(b.streams)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            data = torch.from_numpy(blob).cuda()
            ln = torch.tensor(list(lens), dtype=torch.int64, device="cuda")
            of = torch.tensor(list(offs), dtype=torch.int64, device="cuda")
            out, rcs, ws, hs = tensors(torch, n, 1, b.stride, 16)
            d.decode_torch(data, ln, out, rcs, ws, hs, offsets=of)          # (first call: workspace and side streams made)
        st.synchronize()
        with torch.cuda.stream(st):
            out.fill_(0x5A)
            rcs.fill_(77)
            torch.cuda._sleep(int(50e-3 * 2.1e9))
            d.decode_torch(data, ln, out, rcs, ws, hs, offsets=of)
            ev = torch.cuda.Event()
            ev.record(st)
            assert not ev.query()
        st.synchronize()
        flat = out_np(out, 16)
        b.check(rcs.cpu().tolist(), ws.cpu().tolist(), hs.cpu().tolist(), lambda k, c: flat[k * b.stride:], "after the sleep")
    finally:
        d.close()


@pytest.mark.timeout(180)
def test_two_calls_in_flight_on_two_streams(dec, orc, torch):
    """one decoder, two streams, a workspace each (decode_torch keeps one per stream)"""
    b1 = cached(("mixed", 3, 1, 16), lambda: dbc.mixed_batch(orc, 1, 16, 3))
    b2 = cached(("mixed2", 3, 1, 16), lambda: dbc.mixed_batch(orc, 1, 16, 3, seed=11))
    d = dec.Decoder(1, b1.stages, b1.filt, b1.segments, bits=16)
    try:
        runs = []
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for b, st in zip((b1, b2), streams):
            blob, offs, lens = d._pack(b.streams)
            with torch.cuda.stream(st):
                data = torch.from_numpy(blob).cuda()
                ln = torch.tensor(list(lens), dtype=torch.int64, device="cuda")
                of = torch.tensor(list(offs), dtype=torch.int64, device="cuda")
                out, rcs, ws, hs = tensors(torch, len(b.streams), 1, b.stride, 16)
                torch.cuda._sleep(int(10e-3 * 2.1e9))
                d.decode_torch(data, ln, out, rcs, ws, hs, offsets=of)
            runs.append((b, out, rcs, ws, hs, data))
        assert len(d._workspaces) >= 2
        torch.cuda.synchronize()
        for b, out, rcs, ws, hs, _ in runs:
            flat = out_np(out, 16)
            b.check(rcs.cpu().tolist(), ws.cpu().tolist(), hs.cpu().tolist(), lambda k, c: flat[k * b.stride:], "two streams")
    finally:
        d.close()


@pytest.mark.timeout(120)
def test_errors(dec, orc, torch):
    """a workspace one byte short, n = 0, frames out of range (per-frame ICER_INVALID_INPUT, ws / hs kept)"""
    b = cached(("mixed", 0, 1, 16), lambda: dbc.mixed_batch(orc, 1, 16, 0))
    d = dec.Decoder(1, b.stages, b.filt, b.segments, bits=16)
    try:
        blob, offs, lens = d._pack(b.streams)
        n = len(b.streams)
        data = torch.from_numpy(blob).cuda()
        ln = torch.tensor(list(lens), dtype=torch.int64, device="cuda")
        of = torch.tensor(list(offs), dtype=torch.int64, device="cuda")
        out, rcs, ws, hs = tensors(torch, n, 1, b.stride, 16)
        need = d.workspace_bytes(n, len(blob), b.stride)
        assert need >= 4 * (len(blob) // 2)
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        args = (data.data_ptr(), len(blob), of.data_ptr(), 0, ln.data_ptr(), out.data_ptr(), b.stride, rcs.data_ptr(), ws.data_ptr(),
                hs.data_ptr(), work.data_ptr())
        assert d.decode_device_async_ptrs(n, *args, need - 1, st) == -11
        assert d.decode_device_async_ptrs(0, *args, 0, st) == 0
        torch.cuda.synchronize()
        assert rcs.cpu().tolist() == [77] * n                            # (nothing was enqueued)
        bad_off = torch.tensor([0, len(blob) - 5, len(blob) + 1, len(blob)], dtype=torch.int64, device="cuda")
        bad_len = torch.tensor([lens[0], 6, 0, 0], dtype=torch.int64, device="cuda")
        out4, rcs4, ws4, hs4 = tensors(torch, 4, 1, b.stride, 16, [1, 2, 3, 4], [5, 6, 7, 8])
        d.decode_torch(data, bad_len, out4, rcs4, ws4, hs4, offsets=bad_off)
        torch.cuda.synchronize()
        r = rcs4.cpu().tolist()
        assert r[1:3] == [-11, -11] and r[0] == b.rcs()[0] and r[3] != -11
        assert ws4.cpu().tolist()[1:3] == [2, 3] and hs4.cpu().tolist()[1:3] == [6, 7]
    finally:
        d.close()
