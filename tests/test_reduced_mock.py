"""Reduced-resolution decoders (icerx_decoder_create_reduced, include/icer_hip_dec.h) through every entry point that takes a
decoder -- icerx_decode_host / _device / _device_async / _device_display / _device_display_async -- and the one-shot
icerx_decompress_reduced, with decoder.hip compiled by g++ against tests/emu/hip_mock_async.h as tests/test_display_mock.py
builds it.  Expected: the decoder oracle's plain decode, at stages - r, of each stream's derived stream
(tests/reduced_model.py, tests/reduced_cases.py), and tests/display_model.py of it for the display calls.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.binding import Oracle
from tests import decoder_batch_cases as dbc
from tests import reduced_cases as rc_
from tests import reduced_model as rm
from tests.test_decoder_async_emu import _batch
from tests.test_display_mock import DECODER_HIP, JUNK, MOCK_FLAGS, aligned, check_display, untouched_around

INVALID, QUOTA = -11, -5
_sz = C.c_size_t


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def mock_lib(tmp_path_factory):
    from icer_compression_amd import decoder
    lib_path = str(tmp_path_factory.mktemp("mock_reduced") / "libdecoder_mock_reduced.so")
    subprocess.check_call(["g++"] + MOCK_FLAGS + ["-O2", "-fPIC", "-shared", "-o", lib_path, DECODER_HIP])
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


def _decoder(lib, b, r=None):
    from icer_compression_amd import decoder
    d = decoder.Decoder(b.channels, b.stages, b.filt, b.segments, bits=b.bits, lib=lib, reduce=b.r if r is None else r)
    assert d.reduce == (b.r if r is None else r)
    return d


def plane_call(kind, d, b, stride, w_in=None, h_in=None):
    """the batch through icerx_decode_device ("sync") or icerx_decode_device_async ("async") into n junk-filled rows inside a
    junk-filled buffer -> (rcs, ws, hs, out); everything around the n rows must stay junk, and the input unwritten"""
    blob, offs, lens = d._pack(b.streams)
    before = blob.copy()
    n, ch = len(b.streams), b.channels
    dt = np.uint16 if b.bits == 16 else np.uint8
    view, raw = aligned(n * ch * stride * dt().itemsize)
    if kind == "sync":
        rcs, ws, hs = (C.c_int * n)(), (_sz * n)(*(w_in or [0] * n)), (_sz * n)(*(h_in or [0] * n))
        rc = d.lib.icerx_decode_device(d.handle, n, blob.ctypes.data, offs, lens, view.ctypes.data, stride, rcs, ws, hs)
        res = list(rcs), list(ws), list(hs)
    else:
        o64, l64 = np.asarray(list(offs), np.uint64), np.asarray(list(lens), np.uint64)
        rcs, ws, hs = np.full(n, 77, np.int32), np.asarray(w_in or [0] * n, np.uint64), np.asarray(h_in or [0] * n, np.uint64)
        need = d.workspace_bytes(n, len(blob), stride)
        work, work_raw = aligned(need, 0, 0xCD)
        rc = d.decode_device_async_ptrs(n, blob.ctypes.data, len(blob), o64.ctypes.data, 0, l64.ctypes.data, view.ctypes.data, stride,
                                        rcs.ctypes.data, ws.ctypes.data, hs.ctypes.data, work.ctypes.data, need, None)
        assert untouched_around(work, work_raw, 0xCD), "written outside the workspace"
        res = [int(x) for x in rcs], [int(x) for x in ws], [int(x) for x in hs]
    assert rc == 0, (kind, rc)
    assert untouched_around(view, raw), (kind, "written outside the n rows")
    assert np.array_equal(blob, before), (kind, "the input was written")
    return res[0], res[1], res[2], view.view(dt)


def check_planes(d, b, label, stride=None):
    """host, device and async calls against the batch; the async call's rcs / ws / hs equal the synchronous call's"""
    stride = b.stride if stride is None else stride
    ch = b.channels
    rc, res = d.decode_host(b.streams, stride)
    assert rc == 0, (label, rc)
    b.check([x[0] for x in res], [x[1] for x in res], [x[2] for x in res], lambda k, c: res[k][3][c], label + " host")
    got = {}
    for kind in ("sync", "async"):
        rcs, ws, hs, out = plane_call(kind, d, b, stride)
        b.check(rcs, ws, hs, lambda k, c: out[(k * ch + c) * stride:], f"{label} {kind}")
        got[kind] = (rcs, ws, hs)
    assert got["sync"] == got["async"], label


def check_all(d, b, label):
    check_planes(d, b, label)
    for kind in ("sync", "async", "host"):
        check_display(d, b, kind, label=label)


# ---------------------------------------------------------------------------------------------- the shared batches
@pytest.mark.parametrize("filt", [0, 2, 5])
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (1, 8), (3, 8)])
def test_reduced_mixed_batches_every_entry_point(mock_lib, orc, ch, bits, filt):
    """the mixed batches (3 stages; whole, quota-cut, damaged, truncated, empty, too-large and too-small frames) at r 1 and 2"""
    full = _batch(orc, ch, bits, filt)
    for r in (1, 2):
        b = rc_.of_batch(orc, full, r)
        assert {0, -3, -5} <= set(b.rcs()) and sum(b.written(k) for k in range(len(b.streams))) >= 6
        d = _decoder(mock_lib, b)
        check_all(d, b, f"ch {ch} bits {bits} filt {filt} r {r}")
        d.close()


def test_reduced_mixed_batch_with_each_chain_kernel(mock_lib, orc, dec_wave):
    for ch, bits in ((1, 16), (3, 8)):
        b = rc_.of_batch(orc, _batch(orc, ch, bits, 3), 1)
        d = _decoder(mock_lib, b)
        check_planes(d, b, f"mode {dec_wave} ch {ch} bits {bits}")
        d.close()


def test_reduced_header_pass_and_reuse_batches(mock_lib, orc):
    """more packets than the synchronous header kernel's first capacity (the dropped ones are candidates too); one decoder
    over a large batch, a smaller one, the large one again"""
    b = rc_.of_batch(orc, dbc.header_pass_batch(orc), 2)
    d = _decoder(mock_lib, b)
    check_planes(d, b, "header pass")
    d.close()
    large, small = (rc_.of_batch(orc, x, 1) for x in dbc.reuse_batches(orc, 16, "mock"))
    d = _decoder(mock_lib, large)
    for k, b in enumerate((large, small, large)):
        check_planes(d, b, f"call {k}")
    d.close()


# ---------------------------------------------------------------------------------------------- new small batches
_DEEP = {}


def deep_batch(orc, ch, bits, r):
    """5 stages, three sizes with odd sides at several levels, whole and cut inside level 2, one frame truncated in the middle
    of a packet, one with a damaged level-1 packet, one with a damaged LL packet, one whose packets are all of level <= r, one
    empty"""
    if (ch, bits) not in _DEEP:
        st, filt, sg = 5, 4, 3
        specs = [(97, 99, 1), (130, 97, 2), (97, 99, 3), (112, 96, 4)]
        streams, entries = [], []
        for w, h, seed in specs:
            pl = rc_.planes(w, h, ch, seed, bits)
            streams.append(rc_.encode(orc, pl, st, filt, sg, None if seed % 2 else rc_.level_quota(orc, pl, st, filt, sg, 2, bits), bits))
            entries.append((w, h, "whole" if seed % 2 else "cut in level 2"))
        x = streams[0]
        pk = [x[o: o + n] for o, n in rm.walk(x)]
        extra = [(x[: len(x) // 2 + 3], "truncated"), (rm.flip_in_packet(x, 1, False, 3), "level-1 payload"),
                 (rm.flip_in_packet(x, st, False, 0, subband=0), "LL payload"), (rm.flip_in_packet(x, st, True, 1), "level-5 header"), (b"", "empty")]
        for s, what in extra:
            streams.insert(len(streams) - 1, s)
            entries.insert(len(entries) - 1, (97, 99, what))
        _DEEP[(ch, bits)] = (st, filt, sg, streams, entries, pk)
    st, filt, sg, streams, entries, pk = _DEEP[(ch, bits)]
    low = b"".join(p for p in pk if p[4] <= r)
    rw, rh = rm.reduced_size(130, 97, r)
    return rc_.ReducedBatch(orc, ch, bits, filt, st, sg, streams + [low], r, rw * rh + 7, entries + [(97, 99, "levels <= r only")])


@pytest.mark.parametrize("r", [1, 2, 3, 4])
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (1, 8)])       # (YUV 8-bit at 5 stages exceeds the reference's packet count)
def test_reduced_deep_batch_every_r(mock_lib, orc, ch, bits, r):
    b = deep_batch(orc, ch, bits, r)
    assert b.want[-1][1:3] == (0, 0) == b.want[-3][1:3], "a frame without a kept packet keeps the size in-values"
    assert [w[1:3] for w in b.want[:2]] == [rm.reduced_size(97, 99, r), rm.reduced_size(130, 97, r)]
    d = _decoder(mock_lib, b)
    check_all(d, b, f"deep ch {ch} bits {bits} r {r}")
    # size in-values: kept by the frames without a kept packet, replaced in all others -- in both planners
    n = len(b.streams)
    for kind in ("sync", "async"):
        rcs, ws, hs, _ = plane_call(kind, d, b, b.stride, [3] * n, [4] * n)
        kept = [k for k in range(n) if (ws[k], hs[k]) == (3, 4)]
        assert kept == [n - 3, n - 1] and rcs == [rm.expected(orc, s, r, ch, b.stages, b.filt, b.segments, b.stride, bits, 3, 4)[0] for s in b.streams], kind
    d.close()


def test_reduced_thin_ll_skips_the_transform(mock_lib, orc):
    b = rc_.thin_ll_batch(orc)
    d = _decoder(mock_lib, b)
    check_all(d, b, "thin LL")
    d.close()


def test_reduced_too_many_segments_keeps_the_words(mock_lib, orc):
    b = rc_.too_many_segments_batch(orc)
    d = _decoder(mock_lib, b)
    check_all(d, b, "too many segments")
    d.close()


# ---------------------------------------------------------------------------------------------- strides and arguments
def test_reduced_frame_stride_counts_reduced_samples(mock_lib, orc):
    """a stride that fits the reduced image but not the full one succeeds; one sample less gives the largest frame
    ICER_BYTE_QUOTA_EXCEEDED and leaves the others as they were"""
    full = _batch(orc, 3, 16, 1)
    loose = rc_.of_batch(orc, full, 1)
    area = max(w * h for rc, w, h, _ in loose.want if rc == 0)
    assert area < min(w * h for rc, w, h, _ in full.want if rc == 0)
    d = _decoder(mock_lib, loose)
    exact = rc_.of_batch(orc, full, 1, stride=area)
    assert sum(rc == 0 and w * h == area for rc, w, h, _ in exact.want) >= 2
    check_all(d, exact, "stride = the reduced area")
    tight = rc_.of_batch(orc, full, 1, stride=area - 1)
    assert [rc for rc, w, h, _ in tight.want] == [QUOTA if (rc == 0 and w * h == area) else rc for rc, w, h, _ in exact.want]
    check_all(d, tight, "stride one sample short")
    d.close()


def test_reduce_zero_is_the_plain_decoder_byte_for_byte(mock_lib, orc):
    from icer_compression_amd import decoder
    b = _batch(orc, 3, 16, 6)
    plain = decoder.Decoder(b.channels, b.stages, b.filt, b.segments, bits=b.bits, lib=mock_lib)
    zero = decoder.Decoder.__new__(decoder.Decoder)
    zero.__dict__.update(plain.__dict__)
    zero.handle, zero._workspaces, zero._display_workspaces = C.c_void_p(), {}, {}
    assert mock_lib.icerx_decoder_create_reduced(C.byref(zero.handle), -1, b.channels, b.stages, b.filt, b.segments, b.bits, 0) == 0
    assert mock_lib.icerx_decoder_reduce(zero.handle) == 0 == mock_lib.icerx_decoder_reduce(plain.handle) == mock_lib.icerx_decoder_reduce(None)
    n = len(b.streams)
    assert zero.workspace_bytes(n, 12345, b.stride) == plain.workspace_bytes(n, 12345, b.stride)
    assert zero.display_workspace_bytes(n, 12345, b.stride) == plain.display_workspace_bytes(n, 12345, b.stride)
    for kind in ("sync", "async"):
        a, z = plane_call(kind, plain, b, b.stride), plane_call(kind, zero, b, b.stride)
        assert a[:3] == z[:3] and a[3].tobytes() == z[3].tobytes(), kind
    b.check(*z[:3], lambda k, c: z[3][(k * b.channels + c) * b.stride:], "reduce 0")
    plain.close()
    zero.close()


def test_reduced_argument_errors(mock_lib):
    h = C.c_void_p(0x1234)
    for stages, reduce in ((3, -1), (3, 3), (3, 4), (1, 1), (6, 6), (6, -7)):
        h.value = 0x1234
        assert mock_lib.icerx_decoder_create_reduced(C.byref(h), -1, 1, stages, 0, 1, 16, reduce) == INVALID, (stages, reduce)
        assert not h.value
    assert mock_lib.icerx_decoder_create_reduced(None, -1, 1, 3, 0, 1, 16, 1) == INVALID
    assert mock_lib.icerx_decoder_create_reduced(C.byref(h), -1, 1, 7, 0, 1, 16, 1) == -4          # ICER_TOO_MANY_STAGES first
    assert mock_lib.icerx_decoder_create_reduced(C.byref(h), -1, 2, 3, 0, 1, 16, 1) == INVALID
    for stages in range(1, 7):
        for reduce in range(stages):
            assert mock_lib.icerx_decoder_create_reduced(C.byref(h), -1, 3, stages, 0, 4, 8, reduce) == 0
            assert mock_lib.icerx_decoder_reduce(h) == reduce
            mock_lib.icerx_decoder_destroy(h)
    from icer_compression_amd import decoder
    with pytest.raises(RuntimeError):
        decoder.Decoder(1, 3, 0, 1, lib=mock_lib, reduce=3)
    # the host helper
    rw, rh = _sz(), _sz()
    for w, h_, r in ((61, 47, 1), (61, 47, 2), (64, 48, 3), (1, 1, 5), (0, 9, 2), (4096, 4096, 0), (2 ** 64 - 1, 2 ** 63 + 1, 1)):
        mock_lib.icerx_reduced_size(w, h_, r, C.byref(rw), C.byref(rh))
        assert (rw.value, rh.value) == rm.reduced_size(w, h_, r) == decoder.reduced_size(w, h_, r)
    mock_lib.icerx_reduced_size(5, 5, 1, None, None)


# ---------------------------------------------------------------------------------------------- the one-shot call
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (1, 8), (3, 8)])
def test_decompress_reduced_one_shot(mock_lib, orc, ch, bits):
    from icer_compression_amd import decoder
    b = deep_batch(orc, ch, bits, 2) if (ch, bits) != (3, 8) else rc_.of_batch(orc, _batch(orc, 3, 8, 1), 2)
    seen = set()
    for k, s in enumerate(b.streams):
        if s in seen:
            continue
        seen.add(s)
        rc, w, h, planes = b.want[k]
        got = decoder.decompress(s, ch, b.stages, b.filt, b.segments, bufsize=b.stride, bits=bits, lib=mock_lib, reduce=b.r)
        assert got[:3] == (rc, w, h), (k, b.entries[k], got[:3])
        assert all(np.array_equal(g[: w * h], p[: w * h]) for g, p in zip(got[3], planes)), (k, b.entries[k])
    # the default buffer: exactly the reduced image; one sample less: ICER_BYTE_QUOTA_EXCEEDED and nothing written
    s, (rc, w, h, planes) = b.streams[0], b.want[0]
    got = decoder.decompress(s, ch, b.stages, b.filt, b.segments, bits=bits, lib=mock_lib, reduce=b.r)
    assert got[:3] == (0, w, h) and all(g.size == w * h and np.array_equal(g, p[: w * h]) for g, p in zip(got[3], planes))
    short = decoder.decompress(s, ch, b.stages, b.filt, b.segments, bufsize=w * h - 1, bits=bits, lib=mock_lib, reduce=b.r)
    assert short[0] == QUOTA and not any(p.any() for p in short[3])
    # arguments
    buf = np.frombuffer(s, np.uint8).copy()
    out = [np.full(b.stride, JUNK, np.uint16 if bits == 16 else np.uint8) for _ in range(ch)]
    ptrs = (C.c_void_p * ch)(*[p.ctypes.data for p in out])
    w_, h_ = _sz(0), _sz(0)

    def call(planes_p=ptrs, channels=ch, wp=C.byref(w_), reduce=b.r, stages=b.stages):
        return mock_lib.icerx_decompress_reduced(planes_p, channels, wp, C.byref(h_), b.stride, buf, len(s), stages, b.filt, b.segments, bits, reduce)
    nulled = (C.c_void_p * ch)(*([p.ctypes.data for p in out[:-1]] + [None]))
    for kw in (dict(planes_p=None), dict(planes_p=nulled), dict(channels=2), dict(wp=None), dict(reduce=-1), dict(reduce=b.stages), dict(stages=2, reduce=2)):
        assert call(**kw) == INVALID, kw
    assert all((p == JUNK).all() for p in out)
    assert call() == 0 and (w_.value, h_.value) == (w, h)
