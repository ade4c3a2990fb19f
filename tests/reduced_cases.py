"""Batches for the reduced-resolution decode (include/icer_hip_dec.h, "Decoding at 1/2^r resolution"), shared by the CPU
mock-runtime tests (tests/test_reduced_mock.py) and the GPU tests (tests/test_gpu_reduced.py).  A ReducedBatch is a list of
streams made with `stages` plus what a decoder created with (stages, reduce = r) must deliver for each: the decoder oracle's
plain decode, at stages - r, of the stream's derived stream (tests/reduced_model.py), computed once per distinct stream."""
import numpy as np

from tests import decoder_batch_cases as dbc
from tests import reduced_model as rm


class ReducedBatch:
    """Quacks like decoder_batch_cases.Batch (channels, bits, filt, stages, segments, streams, entries, stride, want, rcs(),
    check()), so that the helpers written for plain batches take it."""

    def __init__(self, orc, channels, bits, filt, stages, segments, streams, r, stride, entries=None):
        self.channels, self.bits, self.filt, self.stages, self.segments, self.r = channels, bits, filt, stages, segments, r
        self.streams = list(streams)
        self.entries = list(entries) if entries is not None else [None] * len(self.streams)
        self.stride = stride
        cache = {}
        self.want = []
        for s in self.streams:
            if s not in cache:
                cache[s] = rm.expected(orc, s, r, channels, stages, filt, segments, stride, bits)
            self.want.append(cache[s])

    rcs = dbc.Batch.rcs
    check = dbc.Batch.check

    def written(self, k):
        rc, w, h, _ = self.want[k]
        return not (rc == -5 or w * h == 0 or w * h > self.stride)


def of_batch(orc, b, r, stride=None):
    """a plain batch's streams at reduction r; default stride: the largest reduced frame that is not a 'big' one, + 13"""
    if stride is None:
        sizes = [(s[1], s[2]) if isinstance(s[0], str) else (s[0], s[1]) for s, q, d in b.entries if s[0] != "big"]
        stride = max(np.prod(rm.reduced_size(w, h, r)) for w, h in sizes) + 13
    return ReducedBatch(orc, b.channels, b.bits, b.filt, b.stages, b.segments, b.streams, r, int(stride), b.entries)


def encode(orc, planes, stages, filt, segments, quota=None, bits=16):
    """the encoder oracle's stream; quota None: room for everything"""
    h, w = planes[0].shape
    ch = len(planes)
    q = quota if quota is not None else 4 * w * h * ch + 32 * 9 * (3 * stages + 1) * segments * ch
    rc, stream, _ = (orc.compress if bits == 16 else orc.compress_u8)(planes, stages, filt, segments, q)
    assert stream and rc == (0 if quota is None else -5), (rc, len(stream))
    return stream


def planes(w, h, channels, seed, bits=16):
    if bits == 8:
        return rm.wave_planes(w, h, channels, seed, top=20, amp=6, noise=4, dtype=np.uint8)      # (int8 storage: no overflow at 5 stages)
    return rm.wave_planes(w, h, channels, seed, top=200, amp=40, noise=30)


def level_quota(orc, pl, stages, filt, segments, level, bits=16):
    """a byte quota that cuts the stream inside `level`: room for every packet before the middle one of that level"""
    x = encode(orc, pl, stages, filt, segments, None, bits)
    at = [o for o, n in rm.walk(x) if x[o + 4] == level]
    return at[len(at) // 2] + 5


# ---- the two grid edge cases
def thin_ll_batch(orc, r=1):
    """16 x 40 decoded at 3 stages: the deepest LL is 2 wide, so the inverse transform is skipped, in the plain decode and
    (8 x 20 at 2 stages: 2 wide again) in the reduced one.  No encoder makes such a stream (ICER_TOO_MANY_STAGES), so these were
    made with 2 stages: the decoder for 3 finds the level-1 and level-2 detail subbands and no LL.  Among frames that are
    transformed."""
    streams = [encode(orc, planes(16, 40, 1, 1), 2, 1, 1), encode(orc, planes(40, 40, 1, 2), 3, 1, 1),
               encode(orc, planes(16, 40, 1, 3), 2, 1, 1, 700), encode(orc, planes(40, 24, 1, 4), 3, 1, 1)]
    b = ReducedBatch(orc, 1, 16, 1, 3, 1, streams, r, 20 * 20 + 3, [(16, 40), (40, 40), (16, 40), (40, 24)])
    assert [w[:3] for w in b.want] == [(0, 8, 20), (0, 20, 20), (0, 8, 20), (0, 20, 12)]
    assert all(b.want[k][3][0][:160].any() for k in (0, 2)), "the thin frames hold decoded samples"
    return b


def too_many_segments_batch(orc, r=1):
    """24 x 24 at 3 stages decoded with 32 segments (encoded with one): the reduced image's level 1 (6 x 6 subbands) takes the
    grid, its level 2 (3 x 3) does not -- ICER_TOO_MANY_SEGMENTS, and the sign-magnitude words decoded so far stay; among
    frames large enough for 32 segments"""
    streams = [encode(orc, planes(24, 24, 1, 5), 3, 0, 1), encode(orc, planes(96, 96, 1, 6), 3, 0, 32),
               encode(orc, planes(24, 24, 1, 7), 3, 0, 1, 600), encode(orc, planes(96, 80, 1, 8), 3, 0, 32)]
    b = ReducedBatch(orc, 1, 16, 0, 3, 32, streams, r, 48 * 48 + 1, [(24, 24), (96, 96), (24, 24), (96, 80)])
    assert [w[:3] for w in b.want] == [(-3, 12, 12), (0, 48, 48), (-3, 12, 12), (0, 48, 40)]
    assert any(w[3][0][:144].any() for w in b.want[::2]), "the frames that stop early hold decoded words"
    return b
