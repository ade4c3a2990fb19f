"""Batches for the decoder's reconstruction option (include/icer_hip_dec.h, "Reconstructing truncated coefficients inside their
interval"), shared by the CPU mock-runtime tests (tests/test_recon_mock.py) and the GPU tests (tests/test_gpu_recon.py).  A
ReconBatch is a list of streams plus what a decoder set to k eighths (and made with reduce = r) must deliver for each: the model of
tests/recon_model.py, computed once per distinct (stream, configuration).  Inputs are the synthetic frames of
icer_compression_amd/synth.py, in which no pixel comes near the clamp at zero: the model asserts at every use that its k = 0
result is the decoder oracle's image."""
import numpy as np

from icer_compression_amd import synth
from tests import decoder_batch_cases as dbc
from tests import recon_model as rmod
from tests import reduced_model as rm

_WANT, _STREAMS = {}, {}


class ReconBatch:
    """Quacks like decoder_batch_cases.Batch (channels, bits, filt, stages, segments, streams, entries, stride, want, rcs(),
    check()), so that the helpers written for plain and reduced batches take it."""

    def __init__(self, orc, channels, bits, filt, stages, segments, streams, k, stride, entries=None, r=0):
        self.channels, self.bits, self.filt, self.stages, self.segments, self.k, self.r = channels, bits, filt, stages, segments, k, r
        self.streams = list(streams)
        self.entries = list(entries) if entries is not None else [None] * len(self.streams)
        self.stride = stride
        self.want = [self._want(orc, s, k) for s in self.streams]

    def _want(self, orc, s, k):
        key = (s, k, self.r, self.channels, self.stages, self.filt, self.segments, self.stride, self.bits)
        if key not in _WANT:
            _WANT[key] = rmod.expected_reduced(orc, s, k, self.r, self.channels, self.stages, self.filt, self.segments, self.stride, self.bits)
        return _WANT[key]

    rcs = dbc.Batch.rcs
    check = dbc.Batch.check

    def at(self, orc, k):
        """the same batch for another k"""
        return ReconBatch(orc, self.channels, self.bits, self.filt, self.stages, self.segments, self.streams, k, self.stride, self.entries, self.r)

    def differs(self, other):
        """frames whose expected image is not the other batch's"""
        return [i for i, (a, b) in enumerate(zip(self.want, other.want)) if any(not np.array_equal(x, y) for x, y in zip(a[3], b[3]))]


def frame(w, h, channels, bits, seed=5):
    if channels == 1:
        return [synth.gray_frame(w, h, seed) if bits == 16 else synth.gray_frame_u8(w, h, seed)]
    return list(synth.color_frame_yuv(w, h, seed) if bits == 16 else synth.color_frame_yuv_u8(w, h, seed))


def encode(orc, planes, stages, filt, segments, quota, bits):
    """the encoder oracle's stream; quota None: room for everything"""
    h, w = planes[0].shape
    q = quota if quota is not None else 4 * w * h * len(planes) + 32 * 9 * (3 * stages + 1) * segments * len(planes)
    rc, stream, _ = (orc.compress if bits == 16 else orc.compress_u8)(planes, stages, filt, segments, q)
    assert stream and rc == (0 if quota is None else -5), (rc, len(stream))
    return stream


def chain_key(stream, o, channels):
    return (stream[o + 7] >> 4 if channels == 3 else 0, stream[o + 4], stream[o + 5], stream[o + 6])


def drop_packets(stream, keep):
    """the accepted packets for which keep(offset) holds, in stream order"""
    return b"".join(stream[o: o + n] for o, n in rm.walk(stream) if keep(o))


def without_mid_chain_packet(stream, channels, planes):
    """one packet out of the middle of a level-1 chain that runs at least three planes: the planes below it no longer run"""
    by = {}
    for o, _ in rm.walk(stream):
        by.setdefault(chain_key(stream, o, channels), []).append(o)
    key = next(k for k in sorted(by) if k[1] == 1 and len(by[k]) >= 3)
    gone = next(o for o in by[key] if (stream[o + 7] & 15) == planes - 2)
    return drop_packets(stream, lambda o: o != gone)


def without_one_segment(stream, channels):
    """every packet of one level-1 segment (the last of its subband) removed: no chain there"""
    key = max((k for k in {chain_key(stream, o, channels) for o, _ in rm.walk(stream)} if k[1] == 1), key=lambda k: (k[3], k))
    return drop_packets(stream, lambda o: chain_key(stream, o, channels) != key)


def main_streams(orc, w, h, channels, bits, filt, stages, segments):
    """one image: two lossy streams with a lossless one between them, then the damaged forms of the first lossy stream"""
    key = (w, h, channels, bits, filt, stages, segments)
    if key not in _STREAMS:
        pl = frame(w, h, channels, bits)
        whole = encode(orc, pl, stages, filt, segments, None, bits)
        # (the 8-bit frames hold 6-bit data: at a quarter of the bytes no non-zero coefficient would be left to move)
        lossy = encode(orc, pl, stages, filt, segments, len(whole) // (4 if bits == 16 else 2), bits)
        milder = encode(orc, pl, stages, filt, segments, len(whole) * (2 if bits == 16 else 3) // 4, bits)
        nplanes = 9 if bits == 16 else 7
        streams = [lossy, whole, milder, without_mid_chain_packet(milder, channels, nplanes), without_one_segment(lossy, channels),
                   rm.flip_in_packet(lossy, stages, True, 1)]
        entries = [(w, h, what) for what in ("lossy", "lossless", "milder", "mid-chain packet removed", "one segment removed", "header flip")]
        _STREAMS[key] = (streams, entries)
    return _STREAMS[key]


def main_batch(orc, channels, bits, filt, k, w=96, h=80, stages=3, segments=3, r=0):
    """the batch every entry point is run with: lossless and lossy streams mixed, and the damage cases.  At the first quota
    every chain of the finest level misses at least two planes."""
    streams, entries = main_streams(orc, w, h, channels, bits, filt, stages, segments)
    rw, rh = rm.reduced_size(w, h, r)
    b = ReconBatch(orc, channels, bits, filt, stages, segments, streams, k, rw * rh + 7, entries, r)
    assert [x[:3] for x in b.want] == [(0, rw, rh)] * len(streams), [x[:3] for x in b.want]
    if r == 0:
        ps = rmod.missing_planes(orc, streams[0], channels, stages, segments, bits)
        assert min(p for lv, p in ps if lv == 1) >= 2, ps
        assert {p for _, p in rmod.missing_planes(orc, streams[1], channels, stages, segments, bits)} == {0}
        assert max(p for _, p in rmod.missing_planes(orc, streams[3], channels, stages, segments, bits)) == (9 if bits == 16 else 7) - 1
    return b


def too_many_segments_batch(orc, k):
    """24 x 24 made with one segment among 96-wide frames made with 32, decoded with 32 segments: the small frames end with
    ICER_TOO_MANY_SEGMENTS at level 3 and keep the sign-magnitude words decoded so far, exactly as with k = 0"""
    key = "too many segments"
    if key not in _STREAMS:
        small, large = frame(24, 24, 1, 16, 7), frame(96, 80, 1, 16, 8)
        whole, whole_small = encode(orc, large, 3, 0, 32, None, 16), encode(orc, small, 3, 0, 1, None, 16)
        _STREAMS[key] = [whole_small, encode(orc, large, 3, 0, 32, len(whole) // 3, 16),
                         encode(orc, small, 3, 0, 1, len(whole_small) * 3 // 4, 16), whole]
    b = ReconBatch(orc, 1, 16, 0, 3, 32, _STREAMS[key], k, 96 * 80 + 1, [(24, 24), (96, 80), (24, 24), (96, 80)])
    assert [x[:3] for x in b.want] == [(-3, 24, 24), (0, 96, 80), (-3, 24, 24), (0, 96, 80)]
    assert all(b.want[i][3][0][:576].any() for i in (0, 2)), "the frames that stop early hold decoded words"
    return b
