"""The definition of the reduced-resolution decode (include/icer_hip_dec.h, "Decoding at 1/2^r resolution") in plain Python:
derive(X, r) builds the derived stream X_r of a stream X, and the reduced decode of X at r IS the plain decode of X_r at
stages - r.  Shared by tests/test_reduced_model.py, test_reduced_plan_device.py, test_reduced_mock.py and test_gpu_reduced.py;
also the specification of the recutter's cuts by resolution.  zlib.crc32 is the reference's CRC.  (One exception, stated in the
header: a chain whose packets do not decode within their own payloads reads on into the bytes that follow in X, which are not
the ones that follow in X_r; tests/sweep_cut_cases.reads_on finds such streams with the decoder oracle.)"""
import zlib

import numpy as np

HEADER = 28


def reduced_size(w, h, r):
    """ceil(w / 2^r), ceil(h / 2^r)"""
    return (w + (1 << r) - 1) >> r, (h + (1 << r) - 1) >> r


def walk(stream):
    """icer_find_packet_in_bytestream's walk: the offsets of the packets a decoder accepts -- preamble, header CRC, payload
    inside the stream, payload CRC; an accepted packet is stepped over whole, anything else byte by byte"""
    stream = bytes(stream)
    off, n = 0, len(stream)
    while off + HEADER <= n:
        hdr = stream[off: off + HEADER]
        if hdr[:2] == b"\x5b\x60" and zlib.crc32(hdr[:24]) == int.from_bytes(hdr[24:28], "little"):
            nbytes = (int.from_bytes(hdr[16:20], "little") + 7) // 8
            if nbytes <= n - off - HEADER and zlib.crc32(stream[off + HEADER: off + HEADER + nbytes]) == int.from_bytes(hdr[20:24], "little"):
                yield off, HEADER + nbytes
                off += HEADER + nbytes
                continue
        off += 1


def derive(stream, r):
    """X -> X_r: the accepted packets of decomp_level > r in stream order, each with decomp_level - r, the size fields
    ceil(. / 2^r) and a fresh header CRC; payload and payload CRC as they are"""
    stream = bytes(stream)
    if r == 0:
        return b"".join(stream[o: o + n] for o, n in walk(stream))
    out = []
    for off, n in walk(stream):
        hdr = bytearray(stream[off: off + HEADER])
        if hdr[4] <= r:
            continue
        hdr[4] -= r
        w, h = reduced_size(int.from_bytes(hdr[8:12], "little"), int.from_bytes(hdr[12:16], "little"), r)
        hdr[8:12] = w.to_bytes(4, "little")
        hdr[12:16] = h.to_bytes(4, "little")
        hdr[24:28] = zlib.crc32(bytes(hdr[:24])).to_bytes(4, "little")
        out.append(bytes(hdr) + stream[off + HEADER: off + n])
    return b"".join(out)


def levels_of(stream):
    """decomp_level of every accepted packet"""
    stream = bytes(stream)
    return [stream[o + 4] for o, _ in walk(stream)]


def flip_in_packet(stream, level, header, which=0, subband=None):
    """one bit flipped in the `which`-th accepted packet of decomp_level `level` (and of `subband`, 0 = LL, if given): in its
    header's segment field (header=True; the header CRC then fails) or in the middle of its payload (the payload CRC fails)"""
    s = bytearray(stream)
    hits = [(o, n) for o, n in walk(stream) if stream[o + 4] == level and (header or n > HEADER) and subband in (None, stream[o + 5])]
    o, n = hits[which]
    s[o + 6 if header else o + HEADER + (n - HEADER) // 2] ^= 0x10
    return bytes(s)


def expected(orc, stream, r, channels, stages, filt, segments, bufsize, bits=16, w0=0, h0=0):
    """(rc, w, h, planes) of the reduced decode: the decoder oracle on the derived stream, with size in-values"""
    from tests.decoder_batch_cases import oracle_decode
    return oracle_decode(orc, derive(stream, r), channels, stages - r, filt, segments, bufsize, bits, w0, h0)


def wave_planes(w, h, channels, seed, top=1000, amp=100, noise=40, dtype=np.uint16):
    """(sin(x / 7 + c) + cos(y / 5)) * amp + top + noise[0, noise): smooth planes far from zero (nothing is clamped)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return [((np.sin(xx / 7.0 + c) + np.cos(yy / 5.0)) * amp + top + rng.integers(0, noise, (h, w))).astype(dtype) for c in range(channels)]
