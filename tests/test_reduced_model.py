"""tests/reduced_model.py -- the definition of the reduced-resolution decode -- held to the decoder oracle everywhere and to the
reference decoder where it is built: the derived stream X_r of a stream X decodes at stages - r with ICER_RESULT_OK to an
image of ceil(w / 2^r) x ceil(h / 2^r), oracle and reference agree on it, and where the full decode clamps nothing it is the
top-left LL_r of the forward transform of the full decode.  CPU only."""
import numpy as np
import pytest

from oracle.binding import Oracle, Reference, have_reference
from tests import reduced_model as rm

FULL = None
# (w, h, channels, stages, filter, segments, quota, bits)
CASES = [
    (61, 47, 1, 3, 0, 1, FULL, 16),
    (61, 47, 1, 3, 1, 2, 900, 16),
    (64, 48, 1, 4, 2, 4, FULL, 16),
    (77, 53, 3, 4, 5, 6, FULL, 16),
    (96, 70, 3, 5, 6, 3, 2500, 16),
    (50, 50, 1, 2, 3, 1, FULL, 16),
    (61, 47, 1, 3, 0, 2, FULL, 8),
    (64, 48, 3, 3, 4, 3, FULL, 8),
]
IDS = [f"{w}x{h}-ch{ch}-S{st}-f{f}-sg{sg}-{'full' if q is None else q}-{bits}bit" for w, h, ch, st, f, sg, q, bits in CASES]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def ref():
    return Reference() if have_reference() else None


def planes_of(case, k):
    w, h, ch, st, filt, sg, quota, bits = case
    if bits == 8:
        return rm.wave_planes(w, h, ch, 100 + k, top=60, amp=20, noise=8, dtype=np.uint8)
    return rm.wave_planes(w, h, ch, 100 + k)


def stream_of(orc, ref, case, k):
    """the reference encoder's stream where the reference is built, else the encoder oracle's"""
    w, h, ch, st, filt, sg, quota, bits = case
    enc = ref or orc
    q = quota if quota is not None else 4 * w * h * ch + 32 * 9 * (3 * st + 1) * sg * ch
    rc, stream, _ = (enc.compress if bits == 16 else enc.compress_u8)(planes_of(case, k), st, filt, sg, q)
    assert stream and rc == (0 if quota is None else -5), (rc, len(stream))
    return stream


def same(a, b):
    n = a[1] * a[2]
    return a[:3] == b[:3] and all(np.array_equal(x[:n], y[:n]) for x, y in zip(a[3], b[3]))


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_derived_streams_decode_to_the_reduced_size(orc, ref, k):
    case = CASES[k]
    w, h, ch, st, filt, sg, quota, bits = case
    x = stream_of(orc, ref, case, k)
    assert rm.derive(x, 0) == x and max(rm.levels_of(x)) == st
    assert quota is not None or set(rm.levels_of(x)) == set(range(1, st + 1))
    for r in range(1, st):
        xr = rm.derive(x, r)
        rw, rh = rm.reduced_size(w, h, r)
        assert [lv - r for lv in rm.levels_of(x) if lv > r] == rm.levels_of(xr)
        assert len(xr) == len(x) - sum(n for o, n in rm.walk(x) if x[o + 4] <= r)
        a = orc.decompress(xr, ch, st - r, filt, sg, bufsize=rw * rh, bits=bits)
        assert a[:3] == (0, rw, rh), (r, a[:3])
        assert a[:3] == rm.expected(orc, x, r, ch, st, filt, sg, rw * rh, bits)[:3]
        if ref is not None:
            b = ref.decompress_raw(xr, ch, st - r, filt, sg, bufsize=rw * rh, bits=bits)
            assert same(a, b), ("oracle != reference", r, a[:3], b[:3])
        # one sample too small a buffer: the plain decode's code
        assert orc.decompress(xr, ch, st - r, filt, sg, bufsize=rw * rh - 1, bits=bits)[0] == -5


@pytest.mark.parametrize("k", [0, 2, 3, 6, 7], ids=[IDS[i] for i in (0, 2, 3, 6, 7)])      # (the uncut streams: they hold level 1)
def test_derived_streams_of_damaged_streams(orc, ref, k):
    """a flipped bit in a level-1 payload (the packet is dropped either way: its damage must not show at r >= 1) and in a
    level-S header (the LL or a deepest subband loses a packet at every r)"""
    case = CASES[k]
    w, h, ch, st, filt, sg, quota, bits = case
    x = stream_of(orc, ref, case, k)
    for level, header in ((1, False), (st, True)):
        y = rm.flip_in_packet(x, level, header, which=1)
        assert len(rm.levels_of(y)) == len(rm.levels_of(x)) - 1
        for r in range(1, st):
            yr = rm.derive(y, r)
            rw, rh = rm.reduced_size(w, h, r)
            assert (yr == rm.derive(x, r)) == (level <= r)
            a = orc.decompress(yr, ch, st - r, filt, sg, bufsize=rw * rh, bits=bits)
            assert a[:3] == (0, rw, rh)
            if ref is not None:
                assert same(a, ref.decompress_raw(yr, ch, st - r, filt, sg, bufsize=rw * rh, bits=bits)), (level, r)
    # a stream cut in the middle of a packet, and one with nothing left above level r
    t = x[: len(x) // 2 + 3]
    assert rm.derive(t, 1) == rm.derive(rm.derive(t, 0), 1)
    only_low = b"".join(x[o: o + n] for o, n in rm.walk(x) if x[o + 4] == 1)
    assert only_low and rm.derive(only_low, 1) == b""


@pytest.mark.parametrize("k", [3, 5], ids=[IDS[3], IDS[5]])
def test_reduced_image_is_the_ll_corner_of_the_forward_transform(orc, ref, k):
    """where the full decode holds no zero sample (nothing was clamped -- asserted, these inputs stay far above zero), the
    reduced image equals the top-left LL_r of the forward transform of the full decode"""
    case = CASES[k]
    w, h, ch, st, filt, sg, quota, bits = case
    x = stream_of(orc, ref, case, k)
    full = (ref.decompress_raw if ref is not None else orc.decompress)(x, ch, st, filt, sg, bufsize=w * h, bits=16)
    assert full[:3] == (0, w, h)
    assert all((p[: w * h] != 0).all() for p in full[3]), "the precondition: no clamped sample in the full decode"
    for r in range(1, st):
        rw, rh = rm.reduced_size(w, h, r)
        red = rm.expected(orc, x, r, ch, st, filt, sg, rw * rh)
        assert red[:3] == (0, rw, rh)
        for c in range(ch):
            img = full[3][c][: w * h].reshape(h, w)
            for who in (orc, ref):
                if who is None:
                    continue
                rc, t = who.dwt(img, r, filt)
                assert rc == 0
                assert np.array_equal(t[:rh, :rw], red[3][c][: rw * rh].reshape(rh, rw)), (who.name, r, c)
