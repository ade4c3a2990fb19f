"""icerx_decode_device_async -- decoder.hip's asynchronous path with its device planner and list-driven kernels
(icer_compression_amd/csrc/decoder_async.hpp) -- compiled by g++ against tests/emu/hip_mock_async.h (device memory = host
memory, a launch = a loop over the grid, streams and events = names) and run on the CPU-scale batches of
tests/decoder_batch_cases.py against the decoder oracle, and against icerx_decode_device of the same build.  CPU only.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle.binding import Oracle
from tests import decoder_batch_cases as dbc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def mock_lib(tmp_path_factory):
    from icer_compression_amd import decoder
    lib_path = str(tmp_path_factory.mktemp("mock_async") / "libdecoder_mock_async.so")
    subprocess.check_call(["g++", "-x", "c++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas",
                           "-DICER_HOST_MOCK", "-DICER_WAVE_EMU", "-include", os.path.join(HERE, "emu", "hip_mock_async.h"),
                           "-o", lib_path, os.path.join(ROOT, "icer_compression_amd", "csrc", "decoder.hip")])
    return decoder.bind(lib_path)


@pytest.fixture(params=[None, "0", "1", "2"], ids=["by-load", "thread-per-chain", "wave-per-chain", "wave-per-plane"])
def dec_wave(request):
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


def _decoder(lib, b):
    from icer_compression_amd import decoder
    return decoder.Decoder(b.channels, b.stages, b.filt, b.segments, bits=b.bits, lib=lib)


def async_call(d, n, blob, offsets, lens, stride, w_in=None, h_in=None, stream_stride=0, junk=0xA5, ws_bytes=None):
    """icerx_decode_device_async on host arrays (the mock's device memory) -> (rc, rcs, ws, hs, out)"""
    dt = np.uint16 if d.bits == 16 else np.uint8
    out = np.full(max(n * d.channels * stride, 1), junk, dt)
    offs = np.asarray(offsets, np.uint64) if offsets is not None else None
    ln = np.asarray(lens, np.uint64)
    rcs = np.full(max(n, 1), 77, np.int32)
    ws = np.asarray(w_in if w_in is not None else [0] * n, np.uint64)
    hs = np.asarray(h_in if h_in is not None else [0] * n, np.uint64)
    need = d.workspace_bytes(n, len(blob), stride)
    work = np.full(max(need if ws_bytes is None else ws_bytes, 1), 0xCD, np.uint8)
    rc = d.decode_device_async_ptrs(n, blob.ctypes.data, len(blob), offs.ctypes.data if offs is not None else None, stream_stride,
                                    ln.ctypes.data, out.ctypes.data, stride, rcs.ctypes.data, ws.ctypes.data, hs.ctypes.data,
                                    work.ctypes.data, need if ws_bytes is None else ws_bytes, None)
    return rc, list(rcs[:n]), [int(x) for x in ws[:n]], [int(x) for x in hs[:n]], out


def check_batch(d, b, label):
    """the batch through the async call: the oracle's frames, and decode_device's rcs / ws / hs"""
    blob, offs, lens = d._pack(b.streams)
    n, ch, stride = len(b.streams), b.channels, b.stride
    rc, rcs, ws, hs, out = async_call(d, n, blob, list(offs), list(lens), stride)
    assert rc == 0, (label, rc)
    b.check(rcs, ws, hs, lambda k, c: out[(k * ch + c) * stride:], label + " async")
    sync_out = np.zeros(n * ch * stride, out.dtype)
    rc2, rcs2, ws2, hs2 = d.decode_device(n, blob.ctypes.data, offs, lens, sync_out.ctypes.data, stride)
    assert rc2 == 0 and (rcs, ws, hs) == (rcs2, ws2, hs2), label


_BATCHES = {}


def _batch(orc, ch, bits, filt):
    key = (ch, bits, filt)
    if key not in _BATCHES:
        _BATCHES[key] = dbc.mixed_batch(orc, ch, bits, filt, "mock")
    return _BATCHES[key]


@pytest.mark.parametrize("filt", range(7))
def test_async_mock_batch_filters_channels_bits(mock_lib, orc, dec_wave, filt):
    for ch in (1, 3):
        for bits in (16, 8):
            b = _batch(orc, ch, bits, filt)
            d = _decoder(mock_lib, b)
            check_batch(d, b, f"filt {filt} ch {ch} bits {bits} mode {dec_wave}")
            d.close()


def test_async_mock_second_header_pass(mock_lib, orc, dec_wave):
    b = dbc.header_pass_batch(orc)
    d = _decoder(mock_lib, b)
    check_batch(d, b, f"mode {dec_wave}")
    d.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_async_mock_decoder_reused_across_calls(mock_lib, orc, bits):
    large, small = dbc.reuse_batches(orc, bits, "mock")
    d = _decoder(mock_lib, large)
    for k, b in enumerate((large, small, large)):
        check_batch(d, b, f"call {k}")
    d.close()


@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 8)])
def test_async_mock_blob_layout(mock_lib, orc, ch, bits):
    """junk, out-of-order and shared offsets, a zero-length entry inside another stream, ws / hs in-values"""
    lay = dbc.Layout(orc, _batch(orc, ch, bits, 4))
    b = lay.batch
    d = _decoder(mock_lib, b)
    rc, rcs, ws, hs, out = async_call(d, lay.n, lay.blob, lay.offsets, lay.lens, b.stride, lay.w_in, lay.h_in)
    assert rc == 0
    lay.check(rcs, ws, hs, lambda k, c: out[(k * b.channels + c) * b.stride:], "async")
    d.close()


def test_async_mock_stream_stride_and_invalid_frames(mock_lib, orc):
    """d_offsets = NULL: stream k at k * stream_stride (the encoder's layout); frames leaving the blob get ICER_INVALID_INPUT
    and keep their ws / hs; call-level errors"""
    b = _batch(orc, 1, 16, 0)
    d = _decoder(mock_lib, b)
    stride_bytes = max(len(s) for s in b.streams) + 5
    n = len(b.streams)
    blob = np.zeros(n * stride_bytes, np.uint8)
    for k, s in enumerate(b.streams):
        blob[k * stride_bytes: k * stride_bytes + len(s)] = np.frombuffer(s, np.uint8)
    lens = [len(s) for s in b.streams]
    rc, rcs, ws, hs, out = async_call(d, n, blob, None, lens, b.stride, stream_stride=stride_bytes)
    assert rc == 0
    b.check(rcs, ws, hs, lambda k, c: out[k * b.stride:], "stream_stride")
    # out of range: one past the end, an offset beyond it, a length that runs over
    offs = [0, len(blob) - 10, len(blob) + 1, len(blob)]
    lens2 = [lens[0], 11, 0, 0]
    rc, rcs, ws, hs, out = async_call(d, 4, blob, offs, lens2, b.stride, w_in=[1, 2, 3, 4], h_in=[5, 6, 7, 8])
    assert rc == 0 and rcs[1:3] == [-11, -11] and (ws[1:3], hs[1:3]) == ([2, 3], [6, 7])
    assert rcs[0] == b.rcs()[0] and rcs[3] != -11
    # call level
    assert async_call(d, 0, blob, [], [], b.stride)[0] == 0
    need = d.workspace_bytes(n, len(blob), b.stride)
    assert need >= 4 * (len(blob) // 2)
    assert async_call(d, n, blob, None, lens, b.stride, stream_stride=stride_bytes, ws_bytes=need - 1)[0] == -11
    d.close()
