"""The decoder's display entry points (include/icer_hip_dec.h: icerx_decode_host_display / _device_display /
_device_display_async, icerx_planes_to_display_device, icerx_decompress_display; csrc/decoder_display.hpp) compiled by g++
against tests/emu/hip_mock_async.h, exactly as tests/test_decoder_async_emu.py builds decoder.hip, and run on the CPU-scale
batches of tests/decoder_batch_cases.py.  Expected images: tests/display_model.py of the frames the decoder oracle expects,
and of the plain call's output of the same build.  CPU only."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle.binding import Oracle
from tests import decoder_batch_cases as dbc
from tests.display_model import display_of
from tests.test_decoder_async_emu import _batch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DECODER_HIP = os.path.join(ROOT, "icer_compression_amd", "csrc", "decoder.hip")
MOCK_FLAGS = ["-x", "c++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-DICER_HOST_MOCK", "-DICER_WAVE_EMU",
              "-include", os.path.join(HERE, "emu", "hip_mock_async.h")]
INVALID = -11                                   # ICER_INVALID_INPUT
JUNK = 0xA5
_sz = C.c_size_t


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def mock_lib(tmp_path_factory):
    from icer_compression_amd import decoder
    lib_path = str(tmp_path_factory.mktemp("mock_display") / "libdecoder_mock_display.so")
    subprocess.check_call(["g++"] + MOCK_FLAGS + ["-O2", "-fPIC", "-shared", "-o", lib_path, DECODER_HIP])
    return decoder.bind(lib_path)


def _decoder(lib, b):
    from icer_compression_amd import decoder
    return decoder.Decoder(b.channels, b.stages, b.filt, b.segments, bits=b.bits, lib=lib)


def aligned(nbytes, shift=0, fill=JUNK, align=64):
    """a uint8 view of `nbytes` bytes that starts `shift` bytes past an `align`-byte boundary, inside a buffer filled with
    `fill`; -> (view, whole buffer)"""
    raw = np.full(nbytes + 2 * align + shift, fill, np.uint8)
    at = (-raw.ctypes.data) % align + shift
    return raw[at: at + nbytes], raw


def untouched_around(view, raw, fill=JUNK):
    at = view.ctypes.data - raw.ctypes.data
    return bool((raw[:at] == fill).all() and (raw[at + view.size:] == fill).all())


def written(rc, w, h, stride):
    """the plain call delivers samples for this frame (tests/decoder_batch_cases.py Batch.check)"""
    return not (rc == -5 or w * h == 0 or w * h > stride)


def plain_call(d, b, stride):
    """icerx_decode_device of the same build -> (rcs, ws, hs, frame(k, c))"""
    blob, offs, lens = d._pack(b.streams)
    n, ch = len(b.streams), b.channels
    out = np.zeros(max(n * ch * stride, 1), np.uint16 if b.bits == 16 else np.uint8)
    rc, rcs, ws, hs = d.decode_device(n, blob.ctypes.data, offs, lens, out.ctypes.data, stride)
    assert rc == 0
    return rcs, ws, hs, lambda k, c: out[(k * ch + c) * stride:]


def display_call(kind, d, b, stride, shift=0):
    """the batch through one display call into junk-filled rows of channels * stride bytes, the device ones `shift` bytes
    past a 64-byte boundary -> (rcs, ws, hs, [row of frame k]); everything around the rows must stay junk"""
    blob, offs, lens = d._pack(b.streams)
    n, ch = len(b.streams), b.channels
    before = blob.copy()
    if kind == "host":
        rows = [np.full(ch * stride, JUNK, np.uint8) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in rows])
        rcs, ws, hs = (C.c_int * n)(), (_sz * n)(), (_sz * n)()
        rc = d.lib.icerx_decode_host_display(d.handle, n, blob.ctypes.data, offs, lens, ptrs, stride, rcs, ws, hs)
        res = list(rcs), list(ws), list(hs)
    else:
        out, raw = aligned(n * ch * stride, shift)
        if kind == "sync":
            rc, *res = d.decode_display_device(n, blob.ctypes.data, offs, lens, out.ctypes.data, stride)
        else:
            o64, l64 = np.asarray(list(offs), np.uint64), np.asarray(list(lens), np.uint64)
            rcs, ws, hs = np.full(n, 77, np.int32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
            need = d.display_workspace_bytes(n, len(blob), stride)
            work, work_raw = aligned(need, 0, 0xCD)
            rc = d.decode_display_async_ptrs(n, blob.ctypes.data, len(blob), o64.ctypes.data, 0, l64.ctypes.data, out.ctypes.data, stride,
                                             rcs.ctypes.data, ws.ctypes.data, hs.ctypes.data, work.ctypes.data, need, None)
            assert untouched_around(work, work_raw, 0xCD), "written outside the workspace"
            res = [int(x) for x in rcs], [int(x) for x in ws], [int(x) for x in hs]
        assert untouched_around(out, raw), (kind, "written outside the n rows")
        rows = [out[k * ch * stride: (k + 1) * ch * stride] for k in range(n)]
    assert rc == 0, (kind, rc)
    assert np.array_equal(blob, before), (kind, "the input was written")
    return res[0], res[1], res[2], rows


def check_display(d, b, kind, stride=None, shift=0, label=""):
    """rcs / ws / hs: the batch's own check and the plain call's; every image: display_of the oracle's frame and of the plain
    call's frame; junk kept behind each image and in the rows of frames without samples"""
    stride = b.stride if stride is None else stride
    label = f"{label} {kind} stride {stride} shift {shift}"
    rcs, ws, hs, rows = display_call(kind, d, b, stride, shift)
    p_rcs, p_ws, p_hs, p_frame = plain_call(d, b, stride)
    assert (list(rcs), list(ws), list(hs)) == (list(p_rcs), list(p_ws), list(p_hs)), label
    ch = b.channels
    # (the batch's check wants planes: hand it the plain call's, whose rcs / ws / hs are the display call's)
    b.check(rcs, ws, hs, p_frame, label)
    seen = 0
    for k, (rc, w, h, planes) in enumerate(b.want):
        nbytes = ch * w * h if written(rc, w, h, stride) else 0
        assert (rows[k][nbytes:] == JUNK).all(), (label, k, "written behind the image")
        if not nbytes:
            continue
        seen += 1
        want = display_of([p[: w * h] for p in planes], ch).reshape(-1)
        got = rows[k][:nbytes]
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{label}: frame {k} {b.entries[k]}: {bad.size} bytes differ from the oracle's image, first at {bad[0]}")
        assert np.array_equal(got, display_of([p_frame(k, c)[: w * h] for c in range(ch)], ch).reshape(-1)), (label, k, "plain call")
    assert seen >= 3, label


# ---------------------------------------------------------------------------------------------- mixed batches
@pytest.mark.parametrize("filt", [0, 3], ids=["A", "D"])
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (1, 8), (3, 8)])
def test_display_mixed_batches(mock_lib, orc, ch, bits, filt):
    """damaged, truncated and early-stop frames among whole ones, through the sync, host and async display calls"""
    b = _batch(orc, ch, bits, filt)
    assert any(rc == -3 for rc, *_ in b.want) and any(not written(rc, w, h, b.stride) for rc, w, h, _ in b.want)
    d = _decoder(mock_lib, b)
    for kind in ("sync", "host", "async"):
        check_display(d, b, kind, label=f"ch {ch} bits {bits} filt {filt}")
    d.close()


# ---------------------------------------------------------------------------------------------- placement
_PLACED = {}


def placement_batch(orc, ch, bits):
    """mixed sizes, w * h no multiple of 4 (61 x 37 = 2257), a frame without a valid packet and a truncated one"""
    if (ch, bits) not in _PLACED:
        entries = [((61, 37, "noise", 1), dbc.LOSSLESS, None), ((22, 19, "smooth", 2), dbc.CUT, None),
                   ((61, 37, "noise", 1), dbc.LOSSLESS, "empty"), ((33, 21, "noise", 3), dbc.LOSSLESS, "truncated"),
                   ((61, 37, "smooth", 4), dbc.CUT, None), ((17, 18, "noise", 5), dbc.LOSSLESS, None)]
        b = dbc.Batch(orc, ch, bits, 0, 2, 2, entries, stride=2260, seed=5)
        assert [written(rc, w, h, b.stride) for rc, w, h, _ in b.want].count(False) == 1
        _PLACED[(ch, bits)] = b
    return _PLACED[(ch, bits)]


@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (3, 8)])
def test_display_placement_vector_and_scalar_paths(mock_lib, orc, ch, bits):
    """frame strides that are a multiple of 4 (every group of an aligned frame takes the 8-byte loads and dword stores), + 1
    and + 3 (frames off the alignment: pixel by pixel), and d_out one byte off: the same images, nothing outside them"""
    b = placement_batch(orc, ch, bits)
    d = _decoder(mock_lib, b)
    for stride in (b.stride, b.stride + 1, b.stride + 3):
        for shift in (0, 1):
            for kind in ("sync", "async"):
                check_display(d, b, kind, stride, shift)
        check_display(d, b, "host", stride)
    d.close()


# ---------------------------------------------------------------------------------------------- the conversion alone
CORNERS = [0, 255, 256, 18492, 18493, 23372, 23373, 32767, 65535]     # (32-bit products overflow from Cb 18493 / Cr 23373)


def corner_planes():
    """27 x 27: the 729 pixels are every (Y, Cb, Cr) of CORNERS^3"""
    i = np.arange(729)
    v = np.asarray(CORNERS, np.uint16)
    return np.stack([v[i // 81], v[(i // 9) % 9], v[i % 9]])


def planes_call(lib, planes, ch, w, h, plane_stride, bits, frame_stride, shift=0, in_shift=0):
    """planes: (n, ch, plane_stride) -> (rc, rows (n, ch * frame_stride)); junk behind every image and around the rows"""
    n = planes.shape[0]
    src, _ = aligned(planes.nbytes, in_shift, 0)
    src[:] = planes.reshape(-1).view(np.uint8)
    keep = src.copy()
    out, raw = aligned(n * ch * frame_stride, shift)
    rc = lib.icerx_planes_to_display_device(src.ctypes.data, n, ch, w, h, plane_stride, bits, out.ctypes.data, frame_stride, None)
    assert untouched_around(out, raw) and np.array_equal(src, keep)
    rows = out.reshape(n, ch * frame_stride)
    assert (rows[:, ch * w * h:] == JUNK).all()
    return rc, rows


def test_planes_to_display_corner_values(mock_lib):
    p = corner_planes()
    want = display_of(list(p), 3).reshape(-1)
    # the set straddles the range in which 32-bit arithmetic (wrapping, here) gives the exact value: equal inside, not outside
    y, cb, cr = (x.astype(np.int32) for x in p)
    ok = (cb < 18493) & (cr < 23373)
    with np.errstate(over="ignore"):
        rgb32 = np.clip(np.stack([y + ((np.int32(91881) * cr) >> 16) - 179, y - ((np.int32(22544) * cb + np.int32(46793) * cr) >> 16) + 135,
                                  y + ((np.int32(116129) * cb) >> 16) - 226], axis=-1), 0, 255).astype(np.uint8)
    assert ok.sum() == 9 * 4 * 6 and np.array_equal(want.reshape(-1, 3)[ok], rgb32[ok])
    assert not np.array_equal(want.reshape(-1, 3)[~ok], rgb32[~ok])
    for plane_stride, frame_stride, shift, in_shift in ((732, 732, 0, 0), (729, 729, 0, 0), (731, 730, 1, 0), (732, 732, 0, 2)):
        planes = np.zeros((2, 3, plane_stride), np.uint16)
        planes[0, :, :729] = p
        planes[1, :, :729] = p[:, ::-1]
        rc, rows = planes_call(mock_lib, planes, 3, 27, 27, plane_stride, 16, frame_stride, shift, in_shift)
        assert rc == 0
        assert np.array_equal(rows[0, : 3 * 729], want) and np.array_equal(rows[1, : 3 * 729], want.reshape(-1, 3)[::-1].reshape(-1))
        gray = np.ascontiguousarray(planes[:, :1])
        rc, rows = planes_call(mock_lib, gray, 1, 27, 27, plane_stride, 16, frame_stride, shift, in_shift)
        assert rc == 0 and np.array_equal(rows[0, :729], np.minimum(p[0], 255).astype(np.uint8))


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("ch", [1, 3])
def test_planes_to_display_random_full_range(mock_lib, ch, bits):
    rng = np.random.default_rng(1000 + 10 * ch + bits)
    w, h, n = 37, 23, 3
    for plane_stride, frame_stride, shift in ((w * h + 5, w * h + 1, 0), (w * h + 5, w * h + 3, 1), (w * h, w * h, 0)):
        planes = rng.integers(0, 1 << bits, (n, ch, plane_stride)).astype(np.uint16 if bits == 16 else np.uint8)
        rc, rows = planes_call(mock_lib, planes, ch, w, h, plane_stride, bits, frame_stride, shift)
        assert rc == 0
        for k in range(n):
            assert np.array_equal(rows[k, : ch * w * h], display_of([planes[k, c, : w * h] for c in range(ch)], ch).reshape(-1)), (k, plane_stride)


# ---------------------------------------------------------------------------------------------- argument errors
def test_display_argument_errors_leave_the_buffers_untouched(mock_lib, orc):
    b = _batch(orc, 3, 16, 0)
    d = _decoder(mock_lib, b)
    lib = mock_lib
    blob, offs, lens = d._pack(b.streams)
    n, ch, stride = len(b.streams), b.channels, b.stride
    out = np.full(n * ch * stride, JUNK, np.uint8)
    rcs, ws, hs = (C.c_int * n)(*[77] * n), (_sz * n)(), (_sz * n)()
    # synchronous and host calls: null output, null image, null per-frame arrays
    assert lib.icerx_decode_device_display(d.handle, n, blob.ctypes.data, offs, lens, None, stride, rcs, ws, hs) == INVALID
    assert lib.icerx_decode_device_display(None, n, blob.ctypes.data, offs, lens, out.ctypes.data, stride, rcs, ws, hs) == INVALID
    assert lib.icerx_decode_device_display(d.handle, n, blob.ctypes.data, offs, lens, out.ctypes.data, stride, None, ws, hs) == INVALID
    assert lib.icerx_decode_host_display(d.handle, n, blob.ctypes.data, offs, lens, None, stride, rcs, ws, hs) == INVALID
    ptrs = (C.c_void_p * n)(*[out.ctypes.data + k * ch * stride for k in range(n)])
    ptrs[2] = None
    assert lib.icerx_decode_host_display(d.handle, n, blob.ctypes.data, offs, lens, ptrs, stride, rcs, ws, hs) == INVALID
    assert (out == JUNK).all() and list(rcs) == [77] * n
    # asynchronous: null pointers, the workspace one byte too small
    o64, l64 = np.asarray(list(offs), np.uint64), np.asarray(list(lens), np.uint64)
    r32, w64, h64 = np.full(n, 77, np.int32), np.full(n, 5, np.uint64), np.full(n, 6, np.uint64)
    need = d.display_workspace_bytes(n, len(blob), stride)
    assert need >= d.workspace_bytes(n, len(blob), stride) + 2 * n * ch * stride         # (the working planes are accounted for)
    work = np.full(need, 0xCD, np.uint8)

    def call(out_p=out.ctypes.data, lens_p=l64.ctypes.data, rcs_p=r32.ctypes.data, work_p=work.ctypes.data, nbytes=need, handle=d.handle):
        return d.lib.icerx_decode_device_display_async(handle, n, blob.ctypes.data, len(blob), o64.ctypes.data, 0, lens_p, out_p, stride,
                                                       rcs_p, w64.ctypes.data, h64.ctypes.data, work_p, nbytes, None)
    for kw in (dict(out_p=None), dict(lens_p=None), dict(rcs_p=None), dict(work_p=None), dict(nbytes=need - 1), dict(handle=None)):
        assert call(**kw) == INVALID, kw
    assert (out == JUNK).all() and (work == 0xCD).all() and (r32 == 77).all() and (w64 == 5).all() and (h64 == 6).all()
    assert call() == 0 and not (out == JUNK).all()
    d.close()
    # the conversion alone
    planes = np.zeros(3 * 40, np.uint16)
    img = np.full(3 * 40, JUNK, np.uint8)

    def conv(p=planes.ctypes.data, n_=1, ch_=3, w=5, h=8, ps=40, bits=16, o=img.ctypes.data, fs=40):
        return lib.icerx_planes_to_display_device(p, n_, ch_, w, h, ps, bits, o, fs, None)
    for kw in (dict(p=None), dict(o=None), dict(ch_=2), dict(ch_=0), dict(bits=12), dict(bits=0), dict(n_=-1), dict(ps=39), dict(fs=39),
               dict(w=1 << 40, h=1 << 40)):
        assert conv(**kw) == INVALID, kw
    assert (img == JUNK).all()
    assert conv(n_=0) == 0 and conv(w=0) == 0 and (img == JUNK).all()
    assert conv() == 0 and not (img[:120] == JUNK).all()
    # the single-stream call
    from icer_compression_amd import decoder
    s = next(s for s, (rc, w, h, _) in zip(b.streams, b.want) if rc == 0)
    buf = np.frombuffer(s, np.uint8).copy()
    image = np.full(3 * b.stride, JUNK, np.uint8)
    w_, h_ = _sz(0), _sz(0)
    for args in ((None, C.byref(w_), C.byref(h_), 2), (image.ctypes.data, None, C.byref(h_), 3), (image.ctypes.data, C.byref(w_), C.byref(h_), 2),
                 (image.ctypes.data, C.byref(w_), C.byref(h_), 4)):
        assert lib.icerx_decompress_display(args[0], args[1], args[2], b.stride, buf, len(s), b.stages, b.filt, b.segments, args[3]) == INVALID
    assert (image == JUNK).all()
    rc, got = decoder.decompress_display(s, 3, b.stages, b.filt, b.segments, lib=lib)
    k = b.streams.index(s)
    _, w, h, planes_k = b.want[k]
    assert rc == 0 and got.shape == (h, w, 3) and np.array_equal(got.reshape(-1), display_of([p[: w * h] for p in planes_k], 3).reshape(-1))
    # too small a buffer: the plain call's code, nothing written
    assert lib.icerx_decompress_display(image.ctypes.data, C.byref(w_), C.byref(h_), w * h - 1, buf, len(s), b.stages, b.filt, b.segments, 3) == -5
    assert (image == JUNK).all()


def test_decompress_display_gray(mock_lib, orc):
    from icer_compression_amd import decoder
    b = _batch(orc, 1, 16, 0)
    for k, (s, (rc, w, h, planes)) in enumerate(zip(b.streams, b.want)):
        if rc != 0 or b.entries[k][2] is not None:
            continue
        rc2, got = decoder.decompress_display(s, 1, b.stages, b.filt, b.segments, lib=mock_lib)
        assert rc2 == 0 and got.shape == (h, w) and np.array_equal(got.reshape(-1), display_of([planes[0][: w * h]], 1))


# ---------------------------------------------------------------------------------------------- stand-alone, sanitized
def _case_file(path, b):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<7i", b.channels, b.bits, b.stages, b.filt, b.segments, len(b.streams), b.stride))
        for s in b.streams:
            fh.write(struct.pack("<I", len(s)) + s)
        for rc, w, h, planes in b.want:
            img = display_of([p[: w * h] for p in planes], b.channels).reshape(-1).tobytes() if written(rc, w, h, b.stride) else b""
            fh.write(struct.pack("<iIII", rc, w, h, len(img)) + img)


def test_display_standalone_program_under_sanitizers(orc, tmp_path):
    """tests/emu/display_main.cpp and decoder.hip as one g++ -fsanitize=address,undefined executable (its own main; nothing
    is loaded into python): a colour and a gray batch through the sync and async display calls and the conversion alone,
    every buffer at exactly its contractual size"""
    exe = str(tmp_path / "display_main")
    subprocess.check_call(["g++"] + MOCK_FLAGS + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, DECODER_HIP,
                           os.path.join(HERE, "emu", "display_main.cpp")])
    for ch, bits in ((3, 16), (1, 8)):
        b = placement_batch(orc, ch, bits)
        case = str(tmp_path / f"case_{ch}_{bits}.bin")
        _case_file(case, b)
        r = subprocess.run([exe, case], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "equal the expectation" in r.stdout, (ch, bits, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
