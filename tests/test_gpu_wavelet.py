"""The standalone wavelet transform on an MI355X against the reference's own functions (oracle/_ref/libicer_ref.so):
every lib_icer-shaped call of include/icer_hip.h / icer_hip_dec.h must leave the caller's buffer and return the code the
reference does, and the device-resident batch calls must give the same planes and per-plane codes."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from icer_compression_amd import api, decoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
_REF = {}


def _ref(reference, name):
    if "lib" not in _REF:
        _REF["lib"] = C.CDLL(reference.lib._name, mode=os.RTLD_LOCAL)
    fn = getattr(_REF["lib"], name)
    fn.restype = C.c_int
    return fn


def ref_transform(reference, inverse, data, filt, stages=1, kind="stages", image_w=None, image_h=None, rowstride=None, N=None, stride=1):
    """the reference's function, with the argument conventions of api.wavelet_transform"""
    bits = 16 if data.dtype == np.uint16 else 8
    fn = _ref(reference, ("icer_inverse_wavelet_transform_" if inverse else "icer_wavelet_transform_") + kind + ("_uint16" if bits == 16 else "_uint8"))
    p = C.c_void_p(data.ctypes.data)
    if kind == "1d":
        return fn(p, C.c_size_t(N), C.c_size_t(stride), C.c_int(filt))
    h, w = data.shape[-2:]
    image_w = w if image_w is None else image_w
    image_h = h if image_h is None else image_h
    if kind == "stages":
        return fn(p, C.c_size_t(image_w), C.c_size_t(image_h), C.c_uint8(stages), C.c_int(filt))
    return fn(p, C.c_size_t(image_w), C.c_size_t(image_h), C.c_size_t(w if rowstride is None else rowstride), C.c_int(filt))


def ours(inverse, data, filt, **kw):
    return (decoder.inverse_wavelet_transform if inverse else api.wavelet_transform)(data, filt, **kw)


def _img(rng, h, w, bits, full):
    dt = np.uint16 if bits == 16 else np.uint8
    top = (1 << bits) if full else (1 << (bits - 4))
    return rng.integers(0, top, size=(h, w), dtype=np.int64).astype(dt)


def _same(reference, inverse, data, filt, **kw):
    a, b = data.copy(), data.copy()
    rr = ref_transform(reference, inverse, a, filt, **kw)
    rc = ours(inverse, b, filt, **kw)
    return rr, rc, a, b


SIZES = [(5, 5), (6, 7), (9, 16), (17, 33), (64, 64), (37, 100), (65, 129), (37, 1000)]     # (h, w)


@pytest.mark.parametrize("bits", [16, 8])
def test_stages_every_filter_size_and_depth(reference, bits):
    rng = np.random.default_rng(100 + bits)
    seen = set()
    for (h, w) in SIZES:
        for filt in range(7):
            for stages in range(1, 8):
                for inverse in (False, True):
                    for full in (False, True):
                        img = _img(rng, h, w, bits, full)
                        rr, rc, a, b = _same(reference, inverse, img, filt, stages=stages)
                        assert rc == rr and np.array_equal(a, b), (h, w, filt, stages, inverse, full)
                        seen.add(rc)
    assert {0, -1, -4} <= seen                       # OK, ICER_INTEGER_OVERFLOW and ICER_TOO_MANY_STAGES all met


@pytest.mark.parametrize("bits", [16, 8])
def test_2d_with_rowstride_leaves_guards(reference, bits):
    rng = np.random.default_rng(200 + bits)
    for (h, w) in [(2, 2), (3, 2), (4, 4), (5, 5), (7, 11), (33, 65), (40, 130), (37, 301)]:
        for filt in range(7):
            for inverse in (False, True):
                buf = _img(rng, h + 1, w + 7, bits, filt % 2 == 1)
                rr, rc, a, b = _same(reference, inverse, buf, filt, kind="2d", image_w=w, image_h=h)
                assert rc == rr and np.array_equal(a, b), (h, w, filt, inverse)
                assert np.array_equal(b[:, w:], buf[:, w:]) and np.array_equal(b[h:], buf[h:])


@pytest.mark.parametrize("bits", [16, 8])
def test_1d_with_stride(reference, bits):
    rng = np.random.default_rng(300 + bits)
    for n in list(range(2, 40)) + [63, 64, 65, 255, 256, 1001, 4096]:
        for filt in range(7):
            for inverse in (False, True):
                stride = 1 + (n % 3)
                buf = _img(rng, 1, n * stride + 5, bits, n % 2 == 0).ravel()
                rr, rc, a, b = _same(reference, inverse, buf, filt, kind="1d", N=n, stride=stride)
                assert rc == rr and np.array_equal(a, b), (n, filt, inverse)
    d = np.arange(8, dtype=np.uint16 if bits == 16 else np.uint8)
    for inverse in (False, True):
        for n in (0, 1):
            assert ours(inverse, d, 0, kind="1d", N=n) == api.ICER_INVALID_INPUT
        assert ours(inverse, d.reshape(2, 4), 0, kind="2d", image_w=1, image_h=2) == api.ICER_INVALID_INPUT
    assert np.array_equal(d, np.arange(8))


@pytest.mark.parametrize("filt", range(7))
def test_4096_six_stages_both_directions(reference, filt):
    rng = np.random.default_rng(400 + filt)
    img = _img(rng, 4096, 4096, 16, False)
    a, b = img.copy(), img.copy()
    assert ref_transform(reference, False, a, filt, stages=6) == api.wavelet_transform(b, filt, stages=6)
    assert np.array_equal(a, b)
    # forward then inverse: equal to the reference's forward then inverse
    assert ref_transform(reference, True, a, filt, stages=6) == decoder.inverse_wavelet_transform(b, filt, stages=6)
    assert np.array_equal(a, b)


def test_roundtrip_equals_reference_roundtrip(reference):
    rng = np.random.default_rng(7)
    for bits in (16, 8):
        for (h, w) in [(31, 47), (64, 100)]:
            for filt in range(7):
                img = _img(rng, h, w, bits, True)
                a, b = img.copy(), img.copy()
                r1 = ref_transform(reference, False, a, filt, stages=3), ref_transform(reference, True, a, filt, stages=3)
                r2 = api.wavelet_transform(b, filt, stages=3), decoder.inverse_wavelet_transform(b, filt, stages=3)
                assert r1 == r2 and np.array_equal(a, b), (bits, h, w, filt)


@pytest.mark.parametrize("bits", [16, 8])
def test_device_batch_on_a_stream_with_per_plane_rcs(reference, bits):
    import torch
    rng = np.random.default_rng(500 + bits)
    h, w, n, stages = 67, 130, 8, 3
    planes = np.stack([_img(rng, h, w, bits, k % 3 == 1) for k in range(n)])
    tdt = torch.int16 if bits == 16 else torch.int8
    s = torch.cuda.Stream()
    for filt in (0, 2, 6):
        want = planes.copy()
        want_fwd = [ref_transform(reference, False, want[k], filt, stages=stages) for k in range(n)]
        fwd = want.copy()
        want_inv = [ref_transform(reference, True, want[k], filt, stages=stages) for k in range(n)]
        d = torch.from_numpy(planes.view(np.int16 if bits == 16 else np.int8).copy()).cuda()
        with torch.cuda.stream(s):
            rf = api.wavelet_forward_torch(d, stages, filt)
            got_fwd = d.clone()
            ri = decoder.wavelet_inverse_torch(d, stages, filt)
        s.synchronize()
        np_dt = np.uint16 if bits == 16 else np.uint8
        assert rf.tolist() == want_fwd and ri.tolist() == want_inv, filt
        assert -1 in want_fwd
        assert np.array_equal(got_fwd.cpu().numpy().view(np_dt), fwd)
        assert np.array_equal(d.cpu().numpy().view(np_dt), want)
        assert d.dtype == tdt
    with pytest.raises(api.IcerHipError):
        api.wavelet_forward_torch(torch.zeros((2, 9, 9), dtype=tdt, device="cuda"), 3, 0)         # ICER_TOO_MANY_STAGES


def test_two_host_threads(reference):
    rng = np.random.default_rng(9)
    jobs = [(_img(rng, 300, 257, 16, True), 2), (_img(rng, 129, 400, 8, True), 5)]
    errors = []

    def run(img, filt):
        try:
            for _ in range(10):
                for inverse in (False, True):
                    rr, rc, a, b = _same(reference, inverse, img, filt, stages=4)
                    assert rc == rr and np.array_equal(a, b)
        except Exception as ex:             # noqa: BLE001 (reported by the main thread)
            errors.append(repr(ex))
    th = [threading.Thread(target=run, args=j) for j in jobs]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_plain_c_program(reference, tmp_path):
    """tests/c_abi/wavelet_dropin.c, compiled with gcc against the product headers and linked with both libraries"""
    from icer_compression_amd.build import build_decoder_library, build_library
    libdir = os.path.dirname(build_library())
    build_decoder_library()
    exe = str(tmp_path / "wavelet_dropin")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi", "wavelet_dropin.c"),
                           "-L", libdir, "-licer_hip", "-licer_hip_dec", "-Wl,-rpath," + libdir, "-o", exe])
    W, H = 61, 37
    rng = np.random.default_rng(11)
    img16 = rng.integers(0, 1 << 16, size=(H, W), dtype=np.int64).astype(np.uint16)
    img16[:, : W // 2] >>= 4
    img8 = rng.integers(0, 256, size=(H, W), dtype=np.int64).astype(np.uint8)
    img8[: H // 2] >>= 3
    (tmp_path / "in.bin").write_bytes(img16.tobytes() + img8.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # the same sequence through the reference
    want = bytearray()

    def put(rc, arr):
        want.extend(np.int32(rc).tobytes() + arr.tobytes())

    def sm(name, arr):
        fn = _ref(reference, name)
        fn(C.c_void_p(arr.ctypes.data), C.c_size_t(arr.size))
        put(0, arr)
    for f in range(7):
        a = img16.copy()
        put(ref_transform(reference, False, a, f, stages=3), a)
        put(ref_transform(reference, True, a, f, stages=3), a)
        put(ref_transform(reference, False, a, f, kind="2d", image_w=W - 4, image_h=H, rowstride=W), a)
        flat = a.ravel()
        put(_ref(reference, "icer_inverse_wavelet_transform_1d_uint16")(C.c_void_p(flat.ctypes.data + 2), C.c_size_t(H - 2), C.c_size_t(W), C.c_int(f)), a)
        sm("icer_to_sign_magnitude_int16", a)
        sm("icer_from_sign_magnitude_int16", a)
        b = img8.copy()
        put(ref_transform(reference, False, b, f, stages=2), b)
        put(ref_transform(reference, True, b, f, stages=2), b)
        flat = b.ravel()
        put(_ref(reference, "icer_wavelet_transform_1d_uint8")(C.c_void_p(flat.ctypes.data + 3), C.c_size_t(W - 6), C.c_size_t(1), C.c_int(f)), b)
        put(ref_transform(reference, True, b, f, kind="2d", image_w=W, image_h=H - 1, rowstride=W), b)
        sm("icer_to_sign_magnitude_int8", b)
        sm("icer_from_sign_magnitude_int8", b)
    a = img16.copy()
    put(ref_transform(reference, False, a, 0, stages=5), a)
    assert (tmp_path / "out.bin").read_bytes() == bytes(want)


def test_device_call_argument_checks():
    import torch
    with pytest.raises(ValueError):
        api.wavelet_forward_torch(torch.zeros(16, dtype=torch.int16, device="cuda"), 1, 0)
    with pytest.raises(ValueError):
        decoder.wavelet_inverse_torch(torch.zeros((3, 0, 8), dtype=torch.int16, device="cuda"), 1, 0)
    lib = api.load_library()
    d = torch.zeros((8, 8), dtype=torch.int16, device="cuda")
    rc = lib.icerx_wavelet_forward_device(C.c_void_p(d.data_ptr()), C.c_int(70000), C.c_size_t(8), C.c_size_t(8), C.c_size_t(0), C.c_int(1),
                                          C.c_int(0), C.c_int(16), C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), None)
    assert rc == api.ICER_INVALID_INPUT                 # more planes than a launch grid takes: rejected, nothing enqueued
