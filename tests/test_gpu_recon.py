"""The decoder's reconstruction option on the GPU (icerx_decoder_set_reconstruction / icerx_decompress_reconstructed,
include/icer_hip_dec.h; Decoder(reconstruct=k), decoder.decompress(reconstruct=k)).  Streams come from the encoder oracle; a
decoder set to k eighths must deliver, for every frame, the image of the model in tests/recon_model.py -- equal, sample for
sample -- through the host, device, asynchronous, display and one-shot calls and through a reduced decoder.  (The same batches
run on the CPU mock in tests/test_recon_mock.py.)"""
import ctypes as C

import numpy as np
import pytest

from tests import recon_cases as rcase
from tests.decoder_batch_cases import decode_host
from tests.test_gpu_display import check_display
from tests.test_gpu_reduced import async_call, check_both, check_sync, dec, orc, sync_call, torch       # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

INVALID = -11
_sz = C.c_size_t


def _decoder(dec, b, k=None):
    d = dec.Decoder(b.channels, b.stages, b.filt, b.segments, bits=b.bits, reduce=b.r, reconstruct=b.k if k is None else k)
    assert d.reconstruct == (b.k if k is None else k) and d.reduce == b.r
    return d


# ---------------------------------------------------------------------------------------------- 1. the grid of the issue
@pytest.mark.parametrize("k", [1, 3, 4])
@pytest.mark.parametrize("filt", [0, 2, 6], ids=["A", "C", "Q"])
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (1, 8), (3, 8)])
def test_recon_grid(dec, orc, torch, ch, bits, filt, k):
    """96 x 80, 3 stages, 3 segments: a lossless stream between two lossy ones (the first leaves p >= 2 in every chain of level
    1), then one with a mid-chain packet removed, one with all packets of a segment removed, one with a header flip"""
    b = rcase.main_batch(orc, ch, bits, filt, k)
    if k == 3:
        assert b.differs(b.at(orc, 0)) == [0, 2, 3, 4, 5], "every lossy frame moves, the lossless one does not"
    d = _decoder(dec, b)
    try:
        check_sync(torch, d, b, f"ch{ch} {bits}bit filt{filt} k{k}")
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------- 2. shapes
@pytest.mark.parametrize("w,h,stages,segments", [(61, 45, 2, 3), (300, 24, 2, 1), (600, 24, 2, 1)],
                         ids=["odd sides", "one wide segment", "chains wider than a workgroup"])
def test_recon_shapes(dec, orc, torch, w, h, stages, segments):
    """(600 x 24: the level-1 chains are 300 samples wide, more than reconstruct_kernel's 256 threads)"""
    b = rcase.main_batch(orc, 1, 16, 0, 3, w, h, stages, segments)
    assert b.differs(b.at(orc, 0))
    d = _decoder(dec, b)
    try:
        check_both(torch, d, b, f"{w}x{h}")
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------- 3. every entry point
@pytest.mark.parametrize("ch,bits,filt,r", [(1, 16, 0, 0), (3, 16, 2, 0), (3, 8, 6, 0), (1, 16, 2, 1), (3, 8, 0, 1)])
def test_recon_every_entry_point(dec, orc, torch, ch, bits, filt, r):
    """the same batch through the host, device, async and display calls; r = 1: a reduced decoder, the rule on the chains of
    the derived stream"""
    b = rcase.main_batch(orc, ch, bits, filt, 3, r=r)
    assert b.differs(b.at(orc, 0))
    d = _decoder(dec, b)
    try:
        label = f"ch{ch} {bits}bit filt{filt} r{r}"
        decode_host(d, b, label)
        check_both(torch, d, b, label)
        for kind in ("host", "sync", "async"):
            check_display(torch, d, b, kind, label=label)
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------- 4. a frame that stops early
def test_recon_leaves_a_frame_that_stops_early(dec, orc, torch):
    """a segment count too large for two of the images: they never reach the transform and come back exactly as with k = 0"""
    b = rcase.too_many_segments_batch(orc, 3)
    zero = b.at(orc, 0)
    assert b.differs(zero) == [1]
    d = _decoder(dec, b)
    try:
        check_both(torch, d, b, "too many segments")
        a = sync_call(torch, d, b, b.stride)
        d.set_reconstruction(0)
        z = sync_call(torch, d, zero, b.stride)
        for i in (0, 2):
            assert np.array_equal(a[3](i, 0)[: 24 * 24], z[3](i, 0)[: 24 * 24]), i
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------- 5. the setting
def test_recon_setting(dec, orc, torch):
    """the setter's range, the getter, and k = 0 after k = 3 on one decoder: a fresh decoder's bytes"""
    lib = dec.load_library()
    b = rcase.main_batch(orc, 1, 16, 0, 0)
    three = b.at(orc, 3)
    d, fresh = _decoder(dec, b, 3), _decoder(dec, b, 0)
    try:
        for bad in (5, -1):
            assert lib.icerx_decoder_set_reconstruction(d.handle, bad) == INVALID and lib.icerx_decoder_reconstruction(d.handle) == 3
        assert lib.icerx_decoder_set_reconstruction(None, 3) == INVALID and lib.icerx_decoder_reconstruction(None) == 0
        for k in range(5):
            assert lib.icerx_decoder_set_reconstruction(d.handle, k) == 0 and lib.icerx_decoder_reconstruction(d.handle) == k == d.reconstruct
        d.set_reconstruction(3)
        check_both(torch, d, three, "k 3")
        d.set_reconstruction(0)
        for call in (sync_call, async_call):
            a, z = call(torch, d, b, b.stride), call(torch, fresh, b, b.stride)
            n = len(b.streams) * b.stride
            assert a[:3] == z[:3] and np.array_equal(a[3](0, 0)[:n], z[3](0, 0)[:n]), call.__name__
        check_both(torch, d, b, "k 0 after k 3")
    finally:
        d.close()
        fresh.close()


# ---------------------------------------------------------------------------------------------- 6. the one-shot calls
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 8)])
def test_decompress_reconstructed_one_shot(dec, orc, ch, bits):
    lib = dec.load_library()
    for r in (0, 1):
        b = rcase.main_batch(orc, ch, bits, 2, 3, r=r)
        for s, (rc, w, h, planes) in zip(b.streams[:4], b.want):
            got = dec.decompress(s, ch, b.stages, b.filt, b.segments, bufsize=b.stride, bits=bits, reduce=r, reconstruct=3)
            assert got[:3] == (rc, w, h)
            assert all(np.array_equal(g[: w * h], p[: w * h]) for g, p in zip(got[3], planes)), r
    b = rcase.main_batch(orc, ch, bits, 2, 3)
    s = b.streams[0]
    buf = np.frombuffer(s, np.uint8).copy()
    out = [np.zeros(b.stride, np.uint16 if bits == 16 else np.uint8) for _ in range(ch)]
    ptrs = (C.c_void_p * ch)(*[p.ctypes.data for p in out])
    w_, h_ = _sz(0), _sz(0)
    for k in (5, -1):
        assert lib.icerx_decompress_reconstructed(ptrs, ch, C.byref(w_), C.byref(h_), b.stride, buf, len(s), b.stages, b.filt, b.segments,
                                                  bits, 0, k) == INVALID
        assert not any(p.any() for p in out)
    if bits == 16:
        from tests.display_model import display_of
        rc, img = dec.decompress_display(s, ch, b.stages, b.filt, b.segments, reconstruct=3)
        rc0, w, h, planes = b.want[0]
        assert rc == 0 and np.array_equal(img.reshape(-1), display_of([p[: w * h] for p in planes], ch).reshape(-1))
