"""CPU checks of the standalone wavelet transform: the line bodies of csrc/wavelet_core.hpp, built for the CPU from
tests/emu/wavelet_emu.cpp and driven in the passes the GPU kernels run, against the reference's own
icer_wavelet_transform_* / icer_inverse_wavelet_transform_* (oracle/_ref), and the host-only sign-magnitude helpers of
the product libraries against the reference's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE_STAGES, MODE_2D, MODE_1D = 0, 1, 2
NAMES = {(MODE_STAGES, False): "icer_wavelet_transform_stages", (MODE_STAGES, True): "icer_inverse_wavelet_transform_stages",
         (MODE_2D, False): "icer_wavelet_transform_2d", (MODE_2D, True): "icer_inverse_wavelet_transform_2d",
         (MODE_1D, False): "icer_wavelet_transform_1d", (MODE_1D, True): "icer_inverse_wavelet_transform_1d"}


@pytest.fixture(scope="module")
def wl(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "emu", "wavelet_emu.cpp")
    so = str(tmp_path_factory.mktemp("wl") / "libwavelet_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-o", so, src])
    L = C.CDLL(so)
    L.wl_emu.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int]
    L.wl_emu_inv_kernels.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int]
    return L


_REF = {}


def _ref_fn(reference, name):
    """the reference's function through a handle of our own (the Reference object declares some of them differently)"""
    if "lib" not in _REF:
        _REF["lib"] = C.CDLL(reference.lib._name, mode=os.RTLD_LOCAL)
    fn = getattr(_REF["lib"], name)
    fn.restype = C.c_int
    return fn


def _ref_call(reference, mode, inv, bits, buf, w, h, stride, stages, filt):
    fn = _ref_fn(reference, NAMES[(mode, inv)] + ("_uint8" if bits == 8 else "_uint16"))
    if mode == MODE_STAGES:
        return fn(C.c_void_p(buf.ctypes.data), C.c_size_t(w), C.c_size_t(h), C.c_uint8(stages), C.c_int(filt))
    if mode == MODE_2D:
        return fn(C.c_void_p(buf.ctypes.data), C.c_size_t(w), C.c_size_t(h), C.c_size_t(stride), C.c_int(filt))
    return fn(C.c_void_p(buf.ctypes.data), C.c_size_t(w), C.c_size_t(stride), C.c_int(filt))


def _both(wl, reference, mode, inv, bits, data, w, h=1, stride=1, stages=0, filt=0):
    a = data.copy()
    b = data.copy()
    rc_ref = _ref_call(reference, mode, inv, bits, a, w, h, stride, stages, filt)
    rc = wl.wl_emu(mode, int(inv), bits, b.ctypes.data, w, h, stride, stages, filt)
    return rc_ref, a, rc, b


def _data(rng, n, bits, small):
    dt = np.uint8 if bits == 8 else np.uint16
    hi = (1 << bits) if not small else (1 << (bits - 3))
    return rng.integers(0, hi, size=n, dtype=np.int64).astype(dt)


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("inv", [False, True])
def test_lines_all_filters_lengths_2_to_70(wl, reference, bits, inv):
    rng = np.random.default_rng(11 + bits + inv)
    for filt in range(7):
        for n in list(range(2, 71)) + [127, 128, 129, 255, 256, 257, 1023, 1024, 1025]:
            for small in (True, False):
                for stride in (1, 3):
                    d = _data(rng, n * stride, bits, small)
                    rc_ref, a, rc, b = _both(wl, reference, MODE_1D, inv, bits, d, n, stride=stride, filt=filt)
                    assert rc == rc_ref and np.array_equal(a, b), (filt, n, small, stride)


def test_lines_overflow_is_flagged_and_wraps(wl, reference):
    rng = np.random.default_rng(5)
    seen = set()
    for bits in (16, 8):
        for inv in (False, True):
            for filt in range(7):
                d = _data(rng, 301, bits, False)
                rc_ref, a, rc, b = _both(wl, reference, MODE_1D, inv, bits, d, 301, filt=filt)
                assert rc == rc_ref and np.array_equal(a, b)
                seen.add(rc)
    assert -1 in seen


def test_short_lines_are_invalid_input(wl):
    for n in (0, 1):
        d = np.arange(4, dtype=np.uint16)
        assert wl.wl_emu(MODE_1D, 0, 16, d.ctypes.data, n, 1, 1, 0, 0) == -11
        assert wl.wl_emu(MODE_2D, 1, 16, d.ctypes.data, n, 2, 2, 0, 0) == -11
        assert np.array_equal(d, np.arange(4, dtype=np.uint16))


@pytest.mark.parametrize("bits", [16, 8])
def test_2d_and_stages(wl, reference, bits):
    rng = np.random.default_rng(bits)
    for filt in range(7):
        for (w, h) in ((2, 2), (4, 5), (5, 5), (7, 12), (33, 17), (70, 9)):
            for inv in (False, True):
                stride = w + 3
                d = _data(rng, h * stride, bits, filt % 2 == 0)
                rc_ref, a, rc, b = _both(wl, reference, MODE_2D, inv, bits, d, w, h, stride, filt=filt)
                assert rc == rc_ref and np.array_equal(a, b), (filt, w, h, inv)
        for (w, h) in ((5, 5), (13, 6), (64, 47), (100, 37), (129, 65)):
            for stages in range(0, 8):
                for inv in (False, True):
                    d = _data(rng, w * h, bits, stages % 2 == 0)
                    rc_ref, a, rc, b = _both(wl, reference, MODE_STAGES, inv, bits, d, w, h, stages=stages, filt=filt)
                    assert rc == rc_ref and np.array_equal(a, b), (filt, w, h, stages, inv)


def test_sign_magnitude_helpers_match_reference(reference):
    from icer_compression_amd import api, decoder
    enc, dec = api.load_library(), decoder.load_library()
    rng = np.random.default_rng(3)
    for bits, ours in ((16, "icer_to_sign_magnitude_int16"), (16, "icer_from_sign_magnitude_int16"),
                       (8, "icer_to_sign_magnitude_int8"), (8, "icer_from_sign_magnitude_int8")):
        lib = enc if "_to_" in ours else dec
        dt = np.uint16 if bits == 16 else np.uint8
        d = rng.integers(0, 1 << bits, size=4099, dtype=np.int64).astype(dt)
        d[:4] = np.array([0, 1 << (bits - 1), (1 << bits) - 1, 1], dt)
        a, b = d.copy(), d.copy()
        ref_fn = _ref_fn(reference, ours)
        ref_fn.argtypes = [C.c_void_p, C.c_size_t]
        getattr(lib, ours).argtypes = [C.c_void_p, C.c_size_t]
        ref_fn(a.ctypes.data, 4000)
        getattr(lib, ours)(b.ctypes.data, 4000)
        assert np.array_equal(a, b), ours


@pytest.mark.parametrize("bits", [16, 8])
def test_inverse_kernel_phases(wl, reference, bits):
    """the inverse as wavelet_inv.hip runs it -- filter A through the tile pass's phases (wavelet_inv.hpp), the others
    through the line bodies: sizes across tile and chunk boundaries (lines of 63 .. 66, 129, 130 samples), odd and even,
    and overflow"""
    rng = np.random.default_rng(40 + bits)
    seen = set()
    for filt in range(7):
        for (w, h) in ((5, 5), (6, 9), (66, 13), (65, 70), (130, 33), (129, 64), (200, 131)):
            for stages in (1, 2, 3):
                for small in (True, False):
                    d = _data(rng, w * h, bits, small)
                    a, b = d.copy(), d.copy()
                    rr = _ref_call(reference, MODE_STAGES, True, bits, a, w, h, w, stages, filt)
                    rc = wl.wl_emu_inv_kernels(MODE_STAGES, bits, b.ctypes.data, w, h, stages, filt)
                    assert rc == rr and np.array_equal(a, b), (filt, w, h, stages, small)
                    seen.add(rc)
    assert {0, -1, -4} <= seen


def test_encoder_tile_pass_is_not_int8_exact_after_overflow(wl, reference):
    """Why the uint8 forward does not run on the encoder's tile pass (dwt_tile.hpp): with the int8 limit it flags the
    same overflows and matches the reference's data while nothing overflows, but it keeps int16 intermediates where the
    reference truncates every lifting step to int8, so after an overflow its data differ."""
    L = wl
    L.wl_emu_tile_u8_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    rng = np.random.default_rng(8)
    w, h = 67, 41
    differs = 0
    for filt in range(7):
        for small in (True, False):
            img = _data(rng, w * h, 8, small)
            a = img.copy()
            rr = _ref_call(reference, MODE_2D, False, 8, a, w, h, w, 1, filt)
            out = np.zeros(w * h, np.uint8)
            rc = L.wl_emu_tile_u8_stage(img.ctypes.data, out.ctypes.data, w, h, filt)
            assert rc == rr
            if rr == 0:
                assert np.array_equal(out, a), filt
            else:
                differs += int(not np.array_equal(out, a))
    assert differs > 0
