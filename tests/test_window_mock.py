"""The window decode (include/icer_hip_dec_window.h; csrc/decoder_window.hpp) through every entry point --
icerx_decode_host_window / _device_window / _device_window_display, their asynchronous twins and the one-shot
icerx_decompress_window -- with decoder.hip compiled by g++ against tests/emu/hip_mock_async.h as tests/test_display_mock.py
builds it.  Expected: tests/window_model.py -- the crop of what the plain call delivers (the decoder oracle's frames, and
reduced_model / recon_model / display_model of them) and the model's chain counts.  CPU only."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from oracle.binding import Oracle
from tests import recon_model as rcm
from tests import reduced_cases as rc_
from tests import reduced_model as rm
from tests import window_model as wm
from tests.test_decoder_async_emu import _batch
from tests.test_display_mock import DECODER_HIP, JUNK, MOCK_FLAGS, aligned, untouched_around
from tests.test_reduced_mock import dec_wave                        # noqa: F401  (the ICER_DEC_WAVE fixture)

INVALID = -11
_sz = C.c_size_t


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def mock_lib(tmp_path_factory):
    from icer_compression_amd import decoder
    lib_path = str(tmp_path_factory.mktemp("mock_window") / "libdecoder_mock_window.so")
    subprocess.check_call(["g++"] + MOCK_FLAGS + ["-O2", "-fPIC", "-shared", "-o", lib_path, DECODER_HIP])
    return decoder.bind(lib_path)


def _decoder(lib, b, reconstruct=0):
    from icer_compression_amd import decoder
    return decoder.Decoder(b.channels, b.stages, b.filt, b.segments, bits=b.bits, lib=lib, reduce=getattr(b, "r", 0), reconstruct=reconstruct)


def pick_windows(b, shift=0):
    """a window per frame, walking through window_model.windows_for of the frame's size (frames without a size: of 40 x 30)"""
    out = []
    for k, (rc, w, h, _) in enumerate(b.want):
        ws = wm.windows_for(w or 40, h or 30)
        out.append(ws[(k + shift) % len(ws)])
    return out


def window_call(kind, d, b, wins, frame_stride, full_stride, display=False):
    """the batch through one window call into junk-filled rows inside a junk-filled buffer -> (rcs, ws, hs, info, row(k, c));
    everything around the rows must stay junk, the workspace's surroundings and the input unwritten"""
    blob, offs, lens = d._pack(b.streams)
    before = blob.copy()
    n, ch = len(b.streams), b.channels
    dt = np.uint8 if display or b.bits == 8 else np.uint16
    if kind == "host":
        assert not display
        rows = [np.full(frame_stride, JUNK * 0x0101 if dt == np.uint16 else JUNK, dt) for _ in range(n * ch)]
        ptrs = (C.c_void_p * (n * ch))(*[r.ctypes.data for r in rows])
        rc, rcs, ws, hs, info = d._sync_window(d.lib.icerx_decode_host_window, n, blob.ctypes.data, offs, lens, wins, ptrs, frame_stride, full_stride)
        row = lambda k, c: rows[k * ch + c]
    else:
        view, raw = aligned(n * ch * frame_stride * dt().itemsize)
        if kind == "sync":
            rc, rcs, ws, hs, info = d.decode_window_device(n, blob.ctypes.data, offs, lens, wins, view.ctypes.data, frame_stride, full_stride, display)
        else:
            o64, l64 = np.asarray(list(offs), np.uint64), np.asarray(list(lens), np.uint64)
            rcs, ws, hs = np.full(n, 77, np.int32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
            w32, info = np.asarray(wins, np.uint32).reshape(n, 4).copy(), np.full((n, 6), 0xEEEEEEEE, np.uint32)
            need = d.window_workspace_bytes(n, len(blob), full_stride, display)
            work, work_raw = aligned(need, 0, 0xCD)
            rc = d.decode_window_async_ptrs(n, blob.ctypes.data, len(blob), o64.ctypes.data, 0, l64.ctypes.data, w32.ctypes.data,
                                            view.ctypes.data, frame_stride, full_stride, rcs.ctypes.data, ws.ctypes.data, hs.ctypes.data,
                                            info.ctypes.data, work.ctypes.data, need, None, display)
            assert untouched_around(work, work_raw, 0xCD), "written outside the workspace"
            assert np.array_equal(w32, np.asarray(wins, np.uint32).reshape(n, 4)), "the windows were written"
            rcs, ws, hs, info = [int(x) for x in rcs], [int(x) for x in ws], [int(x) for x in hs], [[int(x) for x in r] for r in info]
        assert untouched_around(view, raw), (kind, "written outside the n rows")
        out = view.view(dt)
        row = (lambda k, c: out[k * ch * frame_stride: (k + 1) * ch * frame_stride]) if display else \
              (lambda k, c: out[(k * ch + c) * frame_stride: (k * ch + c + 1) * frame_stride])
    assert rc == 0, (kind, rc)
    assert np.array_equal(blob, before), (kind, "the input was written")
    return rcs, ws, hs, info, row


def check_window(orc, d, b, wins, kinds, frame_stride=None, full_stride=None, display=False, label="", want=None, model_stream=None, call=None):
    """every call of `kinds` (through `call`; default window_call, the mock's host memory) against the model
    -> (frames with a window written, chains run, chains of the plain call)"""
    full_stride = b.stride if full_stride is None else full_stride
    frame_stride = full_stride if frame_stride is None else frame_stride
    want = b.want if want is None else want
    r = getattr(b, "r", 0)
    ch = b.channels
    exp = [wm.expected(orc, want[k], wins[k], frame_stride, full_stride, ch, b.stages - r, b.filt, b.segments, b.bits,
                       (model_stream or (lambda s: rm.derive(s, r) if r else s))(b.streams[k]), display) for k in range(len(b.streams))]
    seen = run_total = full_total = 0
    for kind in kinds:
        rcs, ws, hs, info, row = (call or window_call)(kind, d, b, wins, frame_stride, full_stride, display)
        tag = f"{label} {kind}{' display' if display else ''}"
        junk = JUNK if (display or b.bits == 8) else JUNK * 0x0101
        for k, (rc, clip, win, run, full) in enumerate(exp):
            assert rcs[k] == rc and (ws[k], hs[k]) == want[k][1:3], (tag, k, rcs[k], rc, ws[k], hs[k], want[k][1:3])
            assert tuple(info[k][:4]) == clip, (tag, k, info[k], clip)
            if full is not None:
                assert (info[k][4], info[k][5]) == (run, full), (tag, k, info[k], run, full)
            else:
                assert info[k][4] == info[k][5] > 0 or rc == wm.QUOTA, (tag, k, info[k])
            for c in range(1 if display else ch):
                got = row(k, c)
                nwin = 0 if win is None else (win.size if display else win[c].size)
                assert (got[nwin:] == junk).all(), (tag, k, c, "written behind the window")
                if win is None:
                    continue
                ref = (win if display else win[c]).reshape(-1)
                if not np.array_equal(got[:nwin], ref):
                    bad = np.flatnonzero(got[:nwin] != ref)
                    raise AssertionError(f"{tag}: frame {k} {b.entries[k]} window {wins[k]} channel {c}: {bad.size} of {nwin} differ, first at {bad[0]}")
            if kind == kinds[0] and win is not None:
                seen += 1
                run_total += info[k][4]
                full_total += info[k][5]
    return seen, run_total, full_total


# ---------------------------------------------------------------------------------------------- the mixed batches
@pytest.mark.parametrize("filt", [0, 1, 2, 6])
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (1, 8), (3, 8)])
def test_window_mixed_batches_every_entry_point(mock_lib, orc, ch, bits, filt):
    """the mixed batches (3 stages, several sizes; whole, quota-cut, damaged, truncated, empty, too-large and too-small frames),
    a different window per frame: planes through the host, device and async calls, display through the device and async ones"""
    b = _batch(orc, ch, bits, filt)
    assert {0, -3, -5} <= set(b.rcs())
    d = _decoder(mock_lib, b)
    for shift in (0, 5):
        wins = pick_windows(b, shift)
        seen, run, full = check_window(orc, d, b, wins, ("host", "sync", "async"), label=f"ch {ch} bits {bits} filt {filt}")
        assert seen >= 5 and run < full
        check_window(orc, d, b, wins, ("sync", "async"), display=True, label=f"ch {ch} bits {bits} filt {filt}")
    d.close()


def test_window_with_each_chain_kernel(mock_lib, orc, dec_wave):
    for ch, bits in ((1, 16), (3, 8)):
        b = _batch(orc, ch, bits, 3)
        d = _decoder(mock_lib, b)
        check_window(orc, d, b, pick_windows(b, 2), ("sync", "async"), label=f"mode {dec_wave}")
        d.close()


@pytest.mark.parametrize("r", [1, 2])
def test_window_of_a_reduced_decoder(mock_lib, orc, r):
    """the rectangle is in pixels of the reduced image; strides count its samples"""
    for ch, bits, filt in ((1, 16, 0), (3, 16, 4), (1, 8, 0)):
        b = rc_.of_batch(orc, _batch(orc, ch, bits, filt), r)
        d = _decoder(mock_lib, b)
        check_window(orc, d, b, pick_windows(b, r), ("host", "sync", "async"), label=f"r {r} filt {filt}")
        check_window(orc, d, b, pick_windows(b, r + 3), ("async",), display=True, label=f"r {r} filt {filt}")
        d.close()


def test_window_with_reconstruction(mock_lib, orc):
    """reconstruction 3: the crop of recon_model's frames (the kept chains are rebuilt, which is all the window reads)"""
    for ch, bits, filt in ((1, 16, 0), (3, 16, 1)):
        b = _batch(orc, ch, bits, filt)
        want = [rcm.expected(orc, s, 3, ch, b.stages, filt, b.segments, b.stride, bits) for s in b.streams]
        assert any(not np.array_equal(a[3][0], w[3][0]) for a, w in zip(want, b.want)), "no frame of the batch is lossy"
        d = _decoder(mock_lib, b, reconstruct=3)
        check_window(orc, d, b, pick_windows(b, 1), ("host", "sync", "async"), label="recon 3", want=want)
        check_window(orc, d, b, pick_windows(b, 1), ("sync",), display=True, label="recon 3", want=want)
        d.close()


def test_window_larger_than_the_stride(mock_lib, orc):
    """a clipped window of more than frame_stride samples: ICER_BYTE_QUOTA_EXCEEDED for that frame alone, nothing written"""
    b = _batch(orc, 3, 16, 0)
    wins = pick_windows(b)
    areas = sorted({wm.clip(wins[k], w, h)[2] * wm.clip(wins[k], w, h)[3] for k, (rc, w, h, _) in enumerate(b.want) if wm.delivered(rc, w, h, b.stride)})
    stride = areas[len(areas) // 2]
    d = _decoder(mock_lib, b)
    for display in (False, True):
        kinds = ("sync", "async") if display else ("host", "sync", "async")
        seen, _, _ = check_window(orc, d, b, wins, kinds, frame_stride=stride, display=display, label="tight stride")
        assert seen >= 2
    rcs = window_call("sync", d, b, wins, stride, b.stride)[0]
    assert sum(a == wm.QUOTA and w[0] != wm.QUOTA for a, w in zip(rcs, b.want)) >= 2
    d.close()


def test_window_of_frames_that_stop_before_the_transform(mock_lib, orc):
    """ICER_TOO_MANY_SEGMENTS and a deepest LL thinner than 3: all chains stay, the window is the crop of what the plain call leaves"""
    for b in (rc_.too_many_segments_batch(orc), rc_.thin_ll_batch(orc)):
        d = _decoder(mock_lib, b)
        for shift in (0, 3, 11):
            check_window(orc, d, b, pick_windows(b, shift), ("host", "sync", "async"), label="early stop")
        check_window(orc, d, b, pick_windows(b, 1), ("sync", "async"), display=True, label="early stop")
        d.close()


def test_full_frame_window_is_the_plain_call(mock_lib, orc):
    b = _batch(orc, 3, 16, 5)
    d = _decoder(mock_lib, b)
    wins = [(0, 0, 1 << 20, 1 << 20)] * len(b.streams)
    rcs, ws, hs, info, row = window_call("sync", d, b, wins, b.stride, b.stride)
    b.check(rcs, ws, hs, row, "full-frame window")
    assert all(i[4] == i[5] for i in info)
    d.close()


# ---------------------------------------------------------------------------------------------- the one-shot call, arguments
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (1, 8), (3, 8)])
def test_decompress_window_one_shot(mock_lib, orc, ch, bits):
    from icer_compression_amd import decoder
    b = _batch(orc, ch, bits, 0)
    seen = set()
    for k, s in enumerate(b.streams):
        rc, w, h, planes = b.want[k]
        if s in seen or rc != 0 or not wm.delivered(rc, w, h, b.stride):
            continue
        seen.add(s)
        win = wm.windows_for(w, h)[k % 13]
        e_rc, clip, crop, run, full = wm.expected(orc, b.want[k], win, win[2] * win[3], w * h, ch, b.stages, b.filt, b.segments, bits, s)
        got = decoder.decompress(s, ch, b.stages, b.filt, b.segments, bits=bits, lib=mock_lib, window=win)
        assert got[:3] == (e_rc, w, h) and got[4] == list(clip) + [run, full], (k, got[:3], got[4])
        if crop is not None:
            assert all(np.array_equal(g[: c.size], c.reshape(-1)) and not g[c.size:].any() for g, c in zip(got[3], crop)), k
    assert len(seen) >= 3


@pytest.mark.parametrize("ch,bits,filt", [(1, 16, 0), (3, 16, 2), (1, 8, 6)])
def test_decompress_window_one_shot_on_every_stream_of_the_batch(mock_lib, orc, ch, bits, filt):
    """damaged, truncated, quota-cut, too-small and empty streams too: rc, size and window of the one-shot call are those of the
    plain one-shot call (decoder.decompress with its default buffer) and its crop"""
    from icer_compression_amd import decoder
    b = _batch(orc, ch, bits, filt)
    kinds = set()
    for k, s in enumerate(dict.fromkeys(b.streams)):
        plain = decoder.decompress(s, ch, b.stages, b.filt, b.segments, bits=bits, lib=mock_lib)
        rc, w, h, planes = plain
        full = planes[0].size if w * h else 0
        for win in (wm.windows_for(w or 40, h or 30)[k % 15], (0, 0, 1 << 20, 1 << 20)):
            e_rc, clip, crop, run, full_n = wm.expected(orc, plain, win, 1 << 40, max(full, w * h if rc != wm.QUOTA else 0), ch, b.stages, b.filt,
                                                        b.segments, bits, s)
            got = decoder.decompress(s, ch, b.stages, b.filt, b.segments, bits=bits, lib=mock_lib, window=win)
            assert got[:3] == (e_rc, w, h) and got[4][:4] == list(clip), (k, win, got[:3], (e_rc, w, h), got[4], clip)
            if full_n is not None:
                assert got[4][4:] == [run, full_n], (k, win, got[4], run, full_n)
            if crop is None:
                assert not any(g.any() for g in got[3]), (k, win)
            else:
                assert all(g.size == c.size and np.array_equal(g, c.reshape(-1)) for g, c in zip(got[3], crop)), (k, win)
        kinds.add((rc, w * h > 0))
    assert len(kinds) >= 3, kinds


def test_window_argument_errors(mock_lib, orc):
    b = _batch(orc, 1, 16, 0)
    d = _decoder(mock_lib, b)
    blob, offs, lens = d._pack(b.streams)
    n = len(b.streams)
    out = np.full(n * b.stride, JUNK * 0x0101, np.uint16)
    win, info = np.zeros((n, 4), np.uint32), np.full((n, 6), 7, np.uint32)
    rcs, ws, hs = (C.c_int * n)(), (_sz * n)(), (_sz * n)()
    good = [d.handle, n, blob.ctypes.data, offs, lens, win.ctypes.data, out.ctypes.data, b.stride, b.stride, rcs, ws, hs, info.ctypes.data]
    for name in ("icerx_decode_host_window", "icerx_decode_device_window", "icerx_decode_device_window_display"):
        for at in (0, 3, 4, 5, 6, 9, 10, 11, 12):
            args = list(good)
            args[at] = None
            assert getattr(mock_lib, name)(*args) == INVALID, (name, at)
    need = d.window_workspace_bytes(n, len(blob), b.stride)
    work = np.zeros(need, np.uint8)
    a64 = np.zeros(n, np.uint64)
    r32 = np.zeros(n, np.int32)
    good = [d.handle, n, blob.ctypes.data, len(blob), None, 64, a64.ctypes.data, win.ctypes.data, out.ctypes.data, b.stride, b.stride,
            r32.ctypes.data, a64.ctypes.data, a64.ctypes.data, info.ctypes.data, work.ctypes.data, need, None]
    for name in ("icerx_decode_device_window_async", "icerx_decode_device_window_display_async"):
        for at in (0, 6, 7, 8, 11, 12, 13, 14, 15):
            args = list(good)
            args[at] = None
            assert getattr(mock_lib, name)(*args) == INVALID, (name, at)
        args = list(good)
        args[16] = need - 1
        assert getattr(mock_lib, name)(*args) == INVALID, name
    assert (out == JUNK * 0x0101).all() and (info == 7).all() and not work.any()
    assert d.window_workspace_bytes(n, len(blob), b.stride, True) == need and mock_lib.icerx_decode_window_workspace_bytes(None, n, 10, 10) == 0
    d.close()
