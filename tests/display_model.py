"""The 8-bit display conversion of the decoder's *_display entry points (include/icer_hip_dec.h), restated in numpy with
int64 arithmetic: the exact integer value of the formulas for every input 0..65535.  Shared by tests/test_display_mock.py
(CPU) and tests/test_gpu_display.py."""
import numpy as np


def finished(planes):
    """the samples a plain decode call delivers, as the unsigned values the conversion takes: uint16 words or uint8 bytes
    (int16 views of the same memory included) -> int64 arrays"""
    out = []
    for p in planes:
        p = np.asarray(p)
        if p.dtype.kind == "i":
            p = p.view({1: np.uint8, 2: np.uint16}[p.dtype.itemsize])
        assert p.dtype in (np.uint8, np.uint16), p.dtype
        out.append(p.astype(np.int64))
    return out


def display_of(planes, channels):
    """planes: `channels` arrays of one shape (delivered samples) -> uint8 array of that shape (gray8, channels 1) or of that
    shape + (3,) (R, G, B; channels 3)"""
    v = finished(planes)
    assert len(v) == channels and channels in (1, 3)
    if channels == 1:
        return np.minimum(v[0], 255).astype(np.uint8)
    y, cb, cr = v
    r = y + ((91881 * cr) >> 16) - 179
    g = y - ((22544 * cb + 46793 * cr) >> 16) + 135
    b = y + ((116129 * cb) >> 16) - 226
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)
