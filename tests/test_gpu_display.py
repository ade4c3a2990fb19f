"""The decoder's display entry points on the GPU (include/icer_hip_dec.h, csrc/decoder_display.hpp; Decoder.decode_display_*,
decompress_display, planes_to_display_torch): the mixed batches of tests/decoder_batch_cases.py at GPU scale through the sync,
host and async display calls against the decoder oracle's frames and the plain call; placement into junk-filled buffers on
both the 8-byte-load and the pixel-by-pixel path; the values at which 32-bit arithmetic breaks; and byte for byte against the
images the reference's own `icer_util decompress` writes (oracle/_ref/ref_icer_util, prebuilt: it travels with the tree).
(The same code runs on the CPU mock in tests/test_display_mock.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.binding import Oracle
from tests import decoder_batch_cases as dbc
from tests.display_model import display_of
from tests.test_display_mock import JUNK, corner_planes, placement_batch, written
from tests.test_gpu_decoder_async import cached

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_UTIL = os.path.join(ROOT, "oracle", "_ref", "ref_icer_util")
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


def junk_rows(torch, nbytes, shift=0, guard=64):
    """`nbytes` device bytes `shift` past a 64-byte boundary inside a junk-filled tensor -> (view, whole tensor)"""
    raw = torch.full((nbytes + 2 * guard + shift,), JUNK, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 64 == 0
    return raw[guard + shift: guard + shift + nbytes], raw


def rows_back(view, raw, n, row_bytes):
    whole = raw.cpu().numpy()
    at = view.data_ptr() - raw.data_ptr()
    assert (whole[:at] == JUNK).all() and (whole[at + n * row_bytes:] == JUNK).all(), "written outside the n rows"
    return [whole[at + k * row_bytes: at + (k + 1) * row_bytes] for k in range(n)]


def plain_call(torch, d, b, stride):
    blob, offs, lens = d._pack(b.streams)
    n, ch = len(b.streams), b.channels
    d_blob = torch.from_numpy(blob).cuda()
    out = torch.zeros(n * ch * stride * (2 if b.bits == 16 else 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, rcs, ws, hs = d.decode_device(n, d_blob.data_ptr(), offs, lens, out.data_ptr(), stride)
    assert rc == 0
    flat = out.cpu().numpy().view(np.uint16 if b.bits == 16 else np.uint8)
    return rcs, ws, hs, lambda k, c: flat[(k * ch + c) * stride:]


def display_call(torch, kind, d, b, stride, shift=0):
    blob, offs, lens = d._pack(b.streams)
    n, ch = len(b.streams), b.channels
    if kind == "host":
        rows = [np.full(ch * stride, JUNK, np.uint8) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in rows])
        rcs, ws, hs = (C.c_int * n)(), (_sz * n)(), (_sz * n)()
        rc = d.lib.icerx_decode_host_display(d.handle, n, blob.ctypes.data, offs, lens, ptrs, stride, rcs, ws, hs)
        assert rc == 0
        return list(rcs), list(ws), list(hs), rows
    out, raw = junk_rows(torch, n * ch * stride, shift)
    if kind == "sync":
        d_blob = torch.from_numpy(blob).cuda()
        torch.cuda.synchronize()
        rc, rcs, ws, hs = d.decode_display_device(n, d_blob.data_ptr(), offs, lens, out.data_ptr(), stride)
        assert rc == 0
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
            d.decode_display_torch(d_blob, ln, out, t_rcs, t_ws, t_hs, offsets=of)
        st.synchronize()
        rcs, ws, hs = t_rcs.cpu().tolist(), t_ws.cpu().tolist(), t_hs.cpu().tolist()
    return rcs, ws, hs, rows_back(out, raw, n, ch * stride)


def check_display(torch, d, b, kind, stride=None, shift=0, label=""):
    stride = b.stride if stride is None else stride
    label = f"{label} {kind} stride {stride} shift {shift}"
    rcs, ws, hs, rows = display_call(torch, kind, d, b, stride, shift)
    p_rcs, p_ws, p_hs, p_frame = plain_call(torch, d, b, stride)
    assert (list(rcs), list(ws), list(hs)) == (list(p_rcs), list(p_ws), list(p_hs)), label
    ch = b.channels
    b.check(rcs, ws, hs, p_frame, label)
    for k, (rc, w, h, planes) in enumerate(b.want):
        nbytes = ch * w * h if written(rc, w, h, stride) else 0
        assert (rows[k][nbytes:] == JUNK).all(), (label, k, "written behind the image")
        if not nbytes:
            continue
        want = display_of([p[: w * h] for p in planes], ch).reshape(-1)
        got = rows[k][:nbytes]
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{label}: frame {k} {b.entries[k]}: {bad.size} bytes differ from the oracle's image, first at {bad[0]}")
        assert np.array_equal(got, display_of([p_frame(k, c)[: w * h] for c in range(ch)], ch).reshape(-1)), (label, k, "plain call")


@pytest.mark.parametrize("filt", [0, 4], ids=["A", "E"])
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (1, 8), (3, 8)])
def test_display_mixed_batches(dec, orc, torch, ch, bits, filt):
    b = cached(("mixed", filt, ch, bits), lambda: dbc.mixed_batch(orc, ch, bits, filt))
    d = dec.Decoder(ch, b.stages, filt, b.segments, bits=bits)
    try:
        for kind in ("sync", "host", "async"):
            check_display(torch, d, b, kind, label=f"ch {ch} bits {bits} filt {filt}")
    finally:
        d.close()


@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (3, 8)])
def test_display_placement_vector_and_scalar_paths(dec, orc, torch, ch, bits):
    b = placement_batch(orc, ch, bits)
    d = dec.Decoder(ch, b.stages, b.filt, b.segments, bits=bits)
    try:
        for stride in (b.stride, b.stride + 1, b.stride + 3):
            for shift in (0, 1):
                for kind in ("sync", "async"):
                    check_display(torch, d, b, kind, stride, shift)
            check_display(torch, d, b, "host", stride)
    finally:
        d.close()


def test_planes_to_display_corner_values_and_random(dec, torch):
    p = corner_planes()
    want = display_of(list(p), 3)
    t = torch.from_numpy(p.view(np.int16).reshape(1, 3, 27, 27)).cuda()
    assert np.array_equal(dec.planes_to_display_torch(t).cpu().numpy().reshape(-1, 3), want)
    gray = dec.planes_to_display_torch(t[0, 0].contiguous()).cpu().numpy()
    assert gray.shape == (27, 27) and np.array_equal(gray.reshape(-1), np.minimum(p[0], 255).astype(np.uint8))
    # strides off the group and a destination one byte off, through the C call
    lib = dec.load_library()
    for plane_stride, frame_stride, shift in ((732, 732, 0), (731, 730, 1), (729, 729, 0)):
        planes = np.zeros((2, 3, plane_stride), np.uint16)
        planes[0, :, :729], planes[1, :, :729] = p, p[:, ::-1]
        src = torch.from_numpy(planes.view(np.int16)).cuda()
        out, raw = junk_rows(torch, 2 * 3 * frame_stride, shift)
        assert lib.icerx_planes_to_display_device(src.data_ptr(), 2, 3, 27, 27, plane_stride, 16, out.data_ptr(), frame_stride, None) == 0
        torch.cuda.synchronize()
        rows = rows_back(out, raw, 2, 3 * frame_stride)
        assert np.array_equal(rows[0][: 3 * 729], want.reshape(-1)) and np.array_equal(rows[1][: 3 * 729], want[::-1].reshape(-1))
        assert (rows[0][3 * 729:] == JUNK).all() and (rows[1][3 * 729:] == JUNK).all()
    rng = np.random.default_rng(77)
    for ch, dt in ((1, np.uint16), (3, np.uint16), (1, np.uint8), (3, np.uint8)):
        planes = rng.integers(0, np.iinfo(dt).max + 1, (3, ch, 37, 23)).astype(dt)
        t = torch.from_numpy(planes.view(np.int16) if dt == np.uint16 else planes).cuda()
        got = dec.planes_to_display_torch(t).cpu().numpy()
        for k in range(3):
            assert np.array_equal(got[k], display_of([planes[k, c] for c in range(ch)], ch)), (ch, dt, k)


# ---------------------------------------------------------------------------------------------- against the reference itself
W, H, STAGES, FILT, SEGMENTS = 96, 80, 2, 0, 3


def _content():
    """8-bit RGB of saturated 8 x 8 blocks with a little noise: a lossy cut overshoots both ends of 0..255"""
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = np.zeros((H, W, 3), np.uint8)
    for c in range(3):
        blocks = rng.integers(0, 2, (H // 8 + 1, W // 8 + 1)) * 255
        rgb[:, :, c] = np.clip(blocks[yy // 8, (xx + 3 * c) // 8].astype(np.int64) + rng.integers(-6, 7, (H, W)), 0, 255)
    return rgb


def _ycbcr(img):
    r, g, b = (img[:, :, c].astype(np.int64) for c in range(3))
    y = np.clip((19595 * r + 38470 * g + 7471 * b) >> 16, 0, 255)
    return [p.astype(np.uint16) for p in (y, np.clip(((36962 * (b - y)) >> 16) + 128, 0, 255), np.clip(((46727 * (r - y)) >> 16) + 128, 0, 255))]


def _reference_streams():
    """{"gray" / "color": (channels, stream)} made by the encoder API at a lossy quota"""
    from icer_compression_amd import api
    rgb = _content()
    out = {}
    for name, planes, quota in (("gray", [rgb[:, :, 0].astype(np.uint16)], 2500), ("color", _ycbcr(rgb), 6000)):
        rc, stream, _ = api.compress(planes, STAGES, FILT, SEGMENTS, quota)
        assert rc == -5 and 0 < len(stream) <= quota, (name, rc, len(stream))
        out[name] = (len(planes), stream)
    return out


def _read_bmp24(path):
    """a 24-bit bottom-up BMP -> (h, w, 3) RGB"""
    raw = np.fromfile(path, np.uint8)
    assert bytes(raw[:2]) == b"BM" and int.from_bytes(bytes(raw[28:30]), "little") == 24
    off, w, h = (int.from_bytes(bytes(raw[a: a + 4]), "little") for a in (10, 18, 22))
    stride = (3 * w + 3) // 4 * 4
    rows = raw[off: off + stride * h].reshape(h, stride)[:, : 3 * w].reshape(h, w, 3)
    return rows[::-1, :, ::-1]


def _util(exe, args, cwd):
    r = subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (exe, args, r.stdout[-1000:], r.stderr[-1000:])


UTIL_FLAGS = ["-s", str(STAGES), "-f", "A", "-g", str(SEGMENTS)]


def test_display_equals_the_reference_programs_images(dec, torch, tmp_path):
    """ref_icer_util decompress (the reference's own program and library) writes the image; decompress_display,
    decode_display_torch and tools/icer_util_hip give the same bytes"""
    assert os.path.exists(REF_UTIL), "oracle/_ref/ref_icer_util is missing: run `make -C oracle examples` in the authoring container"
    exe = str(tmp_path / "icer_util_hip")
    libdir = os.path.join(ROOT, "icer_compression_amd")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "icer_util_hip.c"),
                           "-L", libdir, "-licer_hip", "-licer_hip_dec", "-Wl,-rpath," + libdir, "-o", exe])
    for name, (ch, stream) in _reference_streams().items():
        mode = "--grayscale" if ch == 1 else "--color"
        (tmp_path / f"{name}.bin").write_bytes(stream)
        _util(REF_UTIL, ["decompress", f"{name}.bin", f"{name}_ref.bmp"] + UTIL_FLAGS + [mode], str(tmp_path))
        _util(exe, ["decompress", f"{name}.bin", f"{name}_hip.bmp"] + UTIL_FLAGS + [mode], str(tmp_path))
        ref_bytes = (tmp_path / f"{name}_ref.bmp").read_bytes()
        assert len(ref_bytes) > 54 and (tmp_path / f"{name}_hip.bmp").read_bytes() == ref_bytes, name
        ref = _read_bmp24(str(tmp_path / f"{name}_ref.bmp"))
        assert ref.shape == (H, W, 3)
        # the plain decode: inside the range in which the reference's 32-bit formulas are defined, and overshooting 255
        rc, w, h, planes = dec.decompress(stream, ch, STAGES, FILT, SEGMENTS)
        assert (rc, w, h) == (0, W, H)
        assert all(int(p.max()) < 18493 for p in planes[1:]) and int(planes[0].max()) > 255 and int((planes[0] == 0).sum()) > 0
        want = ref[:, :, 0] if ch == 1 else ref
        if ch == 1:
            assert np.array_equal(ref[:, :, 0], ref[:, :, 1]) and np.array_equal(ref[:, :, 0], ref[:, :, 2])
        rc, image = dec.decompress_display(stream, ch, STAGES, FILT, SEGMENTS)
        assert rc == 0 and image.shape == want.shape and np.array_equal(image, want), name
        d = dec.Decoder(ch, STAGES, FILT, SEGMENTS)
        try:
            data = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()[None]
            lens = torch.tensor([len(stream)], dtype=torch.int64, device="cuda")
            out = torch.full((1,) + want.shape, JUNK, dtype=torch.uint8, device="cuda")
            rcs = torch.full((1,), 77, dtype=torch.int32, device="cuda")
            ws, hs = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
            d.decode_display_torch(data, lens, out, rcs, ws, hs)
            torch.cuda.synchronize()
            assert (rcs.item(), ws.item(), hs.item()) == (0, W, H) and np.array_equal(out[0].cpu().numpy(), want), name
        finally:
            d.close()


def test_display_torch_from_encoder_output_on_two_streams(dec, torch):
    """RGB8 frames -> Encoder (front-end fusion) -> decode_display_torch on the same stream, nothing on the host; enqueued on
    two streams with separate workspaces: equal results, and lossless streams give back the RGB -> YCbCr -> RGB images"""
    from icer_compression_amd import api
    n, w, h, stages, segments = 3, 88, 52, 3, 4
    rng = np.random.default_rng(11)
    rgb = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
    rgb[1, 10:30, 20:60] = (255, 0, 0)
    quota = 4 * 3 * w * h
    enc = api.Encoder(w, h, 3, stages, 0, segments, max_frames=n)
    d = dec.Decoder(3, stages, 0, segments)
    try:
        results = []
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        raw = torch.from_numpy(rgb).cuda()
        torch.cuda.synchronize()
        for st in streams:
            with torch.cuda.stream(st):
                coded = torch.zeros((n, quota), dtype=torch.uint8, device="cuda")
                sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
                enc_rcs = torch.zeros(n, dtype=torch.int32, device="cuda")
                enc.encode_torch_frontend(raw, quota, coded, sizes, enc_rcs)
                out = torch.full((n, h, w, 3), JUNK, dtype=torch.uint8, device="cuda")
                rcs = torch.full((n,), 77, dtype=torch.int32, device="cuda")
                ws, hs = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
                d.decode_display_torch(coded, sizes, out, rcs, ws, hs)
                results.append((enc_rcs, out, rcs, ws, hs))
        for st in streams:
            st.synchronize()
        assert len(d._display_workspaces) == 2
        a, b = results
        assert a[0].cpu().tolist() == [0] * n and a[2].cpu().tolist() == [0] * n
        assert a[3].cpu().tolist() == [w] * n and a[4].cpu().tolist() == [h] * n
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        got = a[1].cpu().numpy()
        for k in range(n):
            planes = _ycbcr(rgb[k])
            assert np.array_equal(got[k], display_of(planes, 3)), k
    finally:
        d.close()
        enc.close()
