"""The decoder's reconstruction option (icerx_decoder_set_reconstruction / icerx_decompress_reconstructed,
include/icer_hip_dec.h) through the decoder's host pipeline and its device planner, with decoder.hip compiled by g++ against
tests/emu/hip_mock_async.h as tests/test_reduced_mock.py builds it.  Expected: the model of tests/recon_model.py (batches of
tests/recon_cases.py), and tests/display_model.py of it for the display calls.  CPU only."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from oracle.binding import Oracle
from tests import recon_cases as rcase
from tests.test_display_mock import DECODER_HIP, MOCK_FLAGS
from tests.test_reduced_mock import check_all, check_planes, plane_call

INVALID = -11
_sz = C.c_size_t


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def mock_lib(tmp_path_factory):
    from icer_compression_amd import decoder
    lib_path = str(tmp_path_factory.mktemp("mock_recon") / "libdecoder_mock_recon.so")
    subprocess.check_call(["g++"] + MOCK_FLAGS + ["-O2", "-fPIC", "-shared", "-o", lib_path, DECODER_HIP])
    return decoder.bind(lib_path)


def _decoder(lib, b, k=None):
    from icer_compression_amd import decoder
    d = decoder.Decoder(b.channels, b.stages, b.filt, b.segments, bits=b.bits, lib=lib, reduce=b.r, reconstruct=b.k if k is None else k)
    assert d.reconstruct == (b.k if k is None else k) and d.reduce == b.r
    return d


@pytest.mark.parametrize("filt", [0, 2, 6], ids=["A", "C", "Q"])
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (1, 8), (3, 8)])
def test_recon_every_entry_point(mock_lib, orc, ch, bits, filt):
    """lossless, lossy and damaged streams in one batch at k = 3 through host, device, async and the three display calls"""
    b = rcase.main_batch(orc, ch, bits, filt, 3)
    assert b.differs(b.at(orc, 0)) == [0, 2, 3, 4, 5], "every lossy frame moves, the lossless one does not"
    d = _decoder(mock_lib, b)
    check_all(d, b, f"ch {ch} bits {bits} filt {filt}")
    d.close()


@pytest.mark.parametrize("k", [1, 4])
def test_recon_other_points(mock_lib, orc, k):
    for ch, bits, filt in ((1, 16, 2), (3, 8, 0)):
        b = rcase.main_batch(orc, ch, bits, filt, k)
        # (the 6-bit data of the 8-bit frames has few coefficients left where many planes are missing: no such condition there)
        assert bits == 8 or (b.differs(b.at(orc, 3)) and b.differs(b.at(orc, 0)))
        d = _decoder(mock_lib, b)
        check_planes(d, b, f"k {k} ch {ch} bits {bits}")
        d.close()


@pytest.mark.parametrize("w,h,stages,segments", [(61, 45, 2, 3), (300, 24, 2, 1), (600, 24, 2, 1)],
                         ids=["odd sides", "one wide segment", "chains wider than a workgroup"])
def test_recon_shapes(mock_lib, orc, w, h, stages, segments):
    b = rcase.main_batch(orc, 1, 16, 0, 3, w, h, stages, segments)
    d = _decoder(mock_lib, b)
    check_planes(d, b, f"{w}x{h}")
    d.close()


@pytest.mark.parametrize("ch,bits,filt", [(1, 16, 0), (3, 8, 2)])
def test_recon_reduced_decoder(mock_lib, orc, ch, bits, filt):
    """reduce = 1: the rule on the chains of the derived stream"""
    b = rcase.main_batch(orc, ch, bits, filt, 3, r=1)
    assert b.differs(b.at(orc, 0))
    d = _decoder(mock_lib, b)
    check_all(d, b, f"reduced ch {ch} bits {bits}")
    d.close()


def test_recon_leaves_a_frame_that_stops_early(mock_lib, orc):
    b = rcase.too_many_segments_batch(orc, 3)
    assert b.differs(b.at(orc, 0)) == [1]
    d = _decoder(mock_lib, b)
    check_planes(d, b, "too many segments")
    d.close()


def test_recon_setting(mock_lib, orc):
    """the setter's range, the getter, and k = 0 after k = 3 on one decoder: a fresh decoder's bytes"""
    b = rcase.main_batch(orc, 1, 16, 0, 0)
    d, fresh = _decoder(mock_lib, b, 3), _decoder(mock_lib, b, 0)
    lib = mock_lib
    for bad in (5, -1, 8, 1 << 20):
        assert lib.icerx_decoder_set_reconstruction(d.handle, bad) == INVALID and lib.icerx_decoder_reconstruction(d.handle) == 3
        with pytest.raises(ValueError):
            d.set_reconstruction(bad)
    assert lib.icerx_decoder_set_reconstruction(None, 3) == INVALID and lib.icerx_decoder_reconstruction(None) == 0
    for k in range(5):
        assert lib.icerx_decoder_set_reconstruction(d.handle, k) == 0 and lib.icerx_decoder_reconstruction(d.handle) == k == d.reconstruct
    d.set_reconstruction(3)
    three = plane_call("sync", d, b.at(orc, 3), b.stride)
    b.at(orc, 3).check(*three[:3], lambda k, c: three[3][(k * b.channels + c) * b.stride:], "k 3")
    d.set_reconstruction(0)
    for kind in ("sync", "async"):
        a, z = plane_call(kind, d, b, b.stride), plane_call(kind, fresh, b, b.stride)
        assert a[:3] == z[:3] and a[3].tobytes() == z[3].tobytes(), kind
    check_planes(d, b, "k 0 after k 3")
    d.close()
    fresh.close()


@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 8)])
def test_decompress_reconstructed_one_shot(mock_lib, orc, ch, bits):
    from icer_compression_amd import decoder
    for r in (0, 1):
        b = rcase.main_batch(orc, ch, bits, 2, 3, r=r)
        for s, (rc, w, h, planes) in zip(b.streams[:4], b.want):
            got = decoder.decompress(s, ch, b.stages, b.filt, b.segments, bufsize=b.stride, bits=bits, lib=mock_lib, reduce=r, reconstruct=3)
            assert got[:3] == (rc, w, h)
            assert all(np.array_equal(g[: w * h], p[: w * h]) for g, p in zip(got[3], planes)), r
    b = rcase.main_batch(orc, ch, bits, 2, 3)
    s = b.streams[0]
    buf = np.frombuffer(s, np.uint8).copy()
    out = [np.zeros(b.stride, np.uint16 if bits == 16 else np.uint8) for _ in range(ch)]
    ptrs = (C.c_void_p * ch)(*[p.ctypes.data for p in out])
    w_, h_ = _sz(0), _sz(0)

    def call(k, planes_p=ptrs, reduce=0):
        return mock_lib.icerx_decompress_reconstructed(planes_p, ch, C.byref(w_), C.byref(h_), b.stride, buf, len(s), b.stages, b.filt,
                                                       b.segments, bits, reduce, k)
    for k in (5, -1):
        assert call(k) == INVALID and not any(p.any() for p in out)
    assert call(3, planes_p=None) == INVALID and call(3, reduce=b.stages) == INVALID
    assert call(0) == 0 and all(np.array_equal(g, p) for g, p in zip(out, b.at(orc, 0).want[0][3]))
    # the display one-shot of the Python layer
    if bits == 16:
        from tests.display_model import display_of
        rc, img = decoder.decompress_display(s, ch, b.stages, b.filt, b.segments, lib=mock_lib, reconstruct=3)
        rc0, w, h, planes = b.want[0]
        assert rc == 0 and np.array_equal(img.reshape(-1), display_of([p[: w * h] for p in planes], ch).reshape(-1))
