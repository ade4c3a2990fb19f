"""Batches of streams for the batch decoder (icerx_decode_host / icerx_decode_device, decode_batch in
icer_compression_amd/csrc/decoder.hip) and their expected results, shared by the GPU tests (tests/test_gpu_decoder_batch.py)
and the CPU mock-runtime tests (tests/test_emu_decoder.py).

A batch is a list of entries (image spec, quota, damage).  Every distinct stream is decoded once on the CPU by the decoder
oracle with bufsize = the batch's frame stride; where the reference is built and defined for the stream, the reference decoder
must agree with the oracle; a lossless, undamaged stream whose inverse transform is exact must also give back its input.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import zlib

import numpy as np

from oracle.binding import Reference, have_reference
from tests.test_oracle_decoder import packets

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "icer_compression_amd", "csrc")
EMU_SRC = os.path.join(HERE, "emu", "decoder_emu.cpp")
EMU_LIB = os.path.join(HERE, "emu", "libdecoder_emu.so")
_sz = C.c_size_t

LOSSLESS, CUT = "lossless", "cut"
# damage: None, or one of these
DAMAGES = ("empty", "truncated", "flipped", "reversed", "shuffled", "duplicated")


def build_decoder_emu() -> C.CDLL:
    """tests/emu/decoder_emu.cpp (the decoder's device code built by g++), rebuilt when a source is newer"""
    deps = [EMU_SRC] + [os.path.join(CSRC, f) for f in ("decoder_core.hpp", "decoder_plan.hpp", "decoder_wave.hpp", "decoder_planes.hpp",
                                                        "wave.hpp", "plan.hpp", "icer_tables.hpp")]
    if not os.path.exists(EMU_LIB) or any(os.path.getmtime(d) > os.path.getmtime(EMU_LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-DICER_WAVE_EMU", "-o", EMU_LIB, EMU_SRC])
    return C.CDLL(EMU_LIB)


def pw_lds_bytes(chain_w: int, bits: int) -> int:
    """dynamic LDS of decode_chains_planes_kernel for a chain `chain_w` samples wide (decoder_planes.hpp pw_lds_bytes)"""
    lib = build_decoder_emu()
    lib.emu_pw_lds_bytes.restype = _sz
    lib.emu_pw_lds_bytes.argtypes = [C.c_uint32, C.c_int]
    return int(lib.emu_pw_lds_bytes(chain_w, 9 if bits == 16 else 7))


def dim_low(n, lv):
    return (n + (1 << lv) - 1) >> lv


def widest_segment(orc, w, h, stages, segments):
    """the widest segment (= chain) of any subband of a w x h image (the segment grid of orc_partition_make)"""
    best = 0
    for lv in range(1, stages + 1):
        lw, lh = dim_low(w, lv), dim_low(h, lv)
        hw, hh = dim_low(w, lv - 1) - lw, dim_low(h, lv - 1) - lh
        for sw, sh in ((hw, lh), (lw, hh), (hw, hh)) + (((lw, lh),) if lv == stages else ()):
            rc, p = orc.partition(sw, sh, segments)
            assert rc == 0, (sw, sh, segments)
            r, c, r_t, x_t, c_t0 = p[2], p[3], p[4], p[6], p[7]          # (orc_partition's field order)
            best = max(best, x_t + (1 if c_t0 < c else 0))
            if r_t < r:
                x_b, c_b0 = p[10], p[11]
                best = max(best, x_b + (1 if c_b0 < c + 1 else 0))
    return best


def chains_in(stream, channels):
    """chains a stream asks the decoder for: one per (channel, level, subband, segment) that has packets"""
    return len({(p[7] >> 4 if channels == 3 else 0, p[4], p[5], p[6]) for p in packets(stream)})


def image(spec, channels, bits):
    """spec = (w, h, kind, seed); kind: noise / smooth / flat (values inside the coded planes: the lossless streams decode
    exactly) or wild (16-bit values far above them: the decoder derails, identically)"""
    w, h, kind, seed = spec
    rng = np.random.default_rng(seed)
    top = 60 if bits == 16 else 24
    out = []
    for c in range(channels):
        if kind == "noise":
            p = rng.integers(0, top, (h, w))
        elif kind == "smooth":
            yy, xx = np.mgrid[0:h, 0:w]
            p = (np.sin(xx / 7.0 + c) + np.cos(yy / 11.0)) * (top / 5) + top / 2 + rng.integers(0, 4, (h, w))
        elif kind == "flat":
            p = np.full((h, w), int(rng.integers(0, top)))
        elif kind == "wild":
            p = rng.integers(0, 4096 if bits == 16 else 128, (h, w))
        else:
            raise ValueError(kind)
        out.append(np.clip(p, 0, 65535 if bits == 16 else 127).astype(np.uint16 if bits == 16 else np.uint8))
    return out


def exact_inverse(filt, bits, w, h, stages):
    """the oracle's round trip gives back the input (test_decoder_round_trip_is_lossless_when_the_planes_are_all_coded):
    every filter but C; uint8 only with even sides at every level"""
    if filt == 2:
        return False
    return bits == 16 or all(dim_low(w, lv) % 2 == 0 and dim_low(h, lv) % 2 == 0 for lv in range(stages))


def damage(stream, how, rng):
    pk = packets(stream)
    if how == "empty":
        return b""
    if how == "truncated":
        return stream[: len(stream) // 2 + 3]
    if how == "flipped":                        # one payload byte of one packet: the CRC scan drops that packet
        big = [i for i, p in enumerate(pk) if len(p) > 29]
        i = big[int(rng.integers(0, len(big)))]
        p = bytearray(pk[i])
        p[28 + int(rng.integers(0, len(p) - 28))] ^= 1 << int(rng.integers(0, 8))
        return b"".join(pk[:i]) + bytes(p) + b"".join(pk[i + 1:])
    if how == "reversed":
        return b"".join(reversed(pk))
    if how == "shuffled":
        order = rng.permutation(len(pk))
        return b"".join(pk[i] for i in order[: max(1, 3 * len(pk) // 4)])
    if how == "duplicated":
        return b"".join(pk + pk[:7])
    raise ValueError(how)


def oracle_decode(orc, stream, channels, stages, filt, segments, bufsize, bits, w0=0, h0=0):
    """Oracle.decompress, with in-values for w / h (kept for a stream that holds no valid packet)"""
    buf = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, np.uint8)
    w, h = _sz(w0), _sz(h0)
    dt = np.uint16 if bits == 16 else np.uint8
    planes = [np.zeros(max(bufsize, 1), dt) for _ in range(channels)]
    ptrs = (C.c_void_p * channels)(*[p.ctypes.data for p in planes])
    fn = orc.lib.orc_decompress_u16 if bits == 16 else orc.lib.orc_decompress_u8
    fn.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(_sz), C.POINTER(_sz), _sz, C.c_void_p, _sz, C.c_int, C.c_int, C.c_uint]
    rc = fn(ptrs, channels, C.byref(w), C.byref(h), bufsize, buf.ctypes.data, len(stream), stages, filt, segments)
    return rc, w.value, h.value, planes


class Batch:
    """A batch of one decoder configuration.  entries: (spec, quota, damage) with quota LOSSLESS or CUT, damage None or one
    of DAMAGES; spec may also be ("small", w, h, seed): encoded with one segment, too small for the batch's segment count
    (rc -3), or ("big", w, h, seed): left out of the default stride, so that it comes back with rc -5."""

    def __init__(self, orc, channels, bits, filt, stages, segments, entries, stride=None, seed=0, check_reference=True):
        self.channels, self.bits, self.filt, self.stages, self.segments = channels, bits, filt, stages, segments
        self.entries = list(entries)
        rng = np.random.default_rng(seed)
        comp = orc.compress if bits == 16 else orc.compress_u8
        encoded = {}
        self.streams, self.inputs = [], []
        for spec, quota, dmg in self.entries:
            tag = spec[0] if isinstance(spec[0], str) else None
            key = (spec, quota)
            if key not in encoded:
                w, h = spec[1:3] if tag else spec[:2]
                planes = image((w, h, "noise", spec[3]) if tag else spec, channels, bits)
                # (lossless: room for every packet's 28-byte header besides the data)
                q = 4 * w * h * channels + 32 * 9 * (3 * stages + 1) * segments * channels if quota == LOSSLESS else w * h * channels // 3 + 100
                rc, stream, _ = comp(planes, stages, filt, 1 if tag == "small" else segments, q)
                assert stream, (spec, quota, rc)
                encoded[key] = (stream, planes, rc == 0 and quota == LOSSLESS and tag is None and spec[2] != "wild")
            stream, planes, whole = encoded[key]
            if dmg is not None:
                stream = damage(stream, dmg, rng)
            self.streams.append(stream)
            self.inputs.append(planes if whole and dmg is None else None)
        self.stride = stride if stride is not None else max(s[1] * s[2] if s[0] == "small" else s[0] * s[1]
                                                             for s, q, d in self.entries if s[0] != "big") + 13
        self.want = self._expected(orc, check_reference)

    def _expected(self, orc, check_reference):
        ref = Reference() if check_reference and have_reference() else None
        cache, want = {}, []
        for k, s in enumerate(self.streams):
            if s not in cache:
                a = oracle_decode(orc, s, self.channels, self.stages, self.filt, self.segments, self.stride, self.bits)
                if ref is not None and s and (self.channels == 1 or len({s[o + 7] >> 4 for o in packets_valid(s)}) == 3):
                    b = ref.decompress_raw(s, self.channels, self.stages, self.filt, self.segments, bufsize=self.stride, bits=self.bits)
                    assert a[:3] == b[:3] and all(np.array_equal(x, y) for x, y in zip(a[3], b[3])), ("oracle != reference", k, a[:3], b[:3])
                cache[s] = a
            want.append(cache[s])
            inp = self.inputs[k]
            if inp is not None:
                h, w = inp[0].shape
                assert want[k][:3] == (0, w, h), (k, want[k][:3])
                if exact_inverse(self.filt, self.bits, w, h, self.stages):
                    assert all(np.array_equal(x[: w * h].reshape(h, w), p) for x, p in zip(want[k][3], inp)), ("not lossless", k)
        return want

    def rcs(self):
        return [w[0] for w in self.want]

    def groups(self):
        """frames of one size that decode with a transform: {(w, h): [positions]}"""
        out = {}
        for k, (rc, w, h, _) in enumerate(self.want):
            if rc == 0 and w * h <= self.stride:
                out.setdefault((w, h), []).append(k)
        return out

    def check(self, rcs, ws, hs, frame, label=""):
        """frame(k, c) -> channel c of frame k as decoded (at least w * h samples)"""
        assert list(rcs) == self.rcs(), (label, list(rcs), self.rcs())
        for k, (rc, w, h, planes) in enumerate(self.want):
            assert (ws[k], hs[k]) == (w, h), (label, k, ws[k], hs[k], w, h)
            if rc == -5 or w * h == 0 or w * h > self.stride:
                continue
            for c in range(self.channels):
                got = np.asarray(frame(k, c))[: w * h]
                if not np.array_equal(got, planes[c][: w * h]):
                    bad = np.flatnonzero(got != planes[c][: w * h])
                    raise AssertionError(f"{label}: frame {k} {self.entries[k]} channel {c}: {bad.size} samples differ, "
                                         f"first at {bad[0]} ({got[bad[0]]} != {planes[c][bad[0]]})")


def decode_host(dec, batch, label=""):
    rc, res = dec.decode_host(batch.streams, batch.stride)
    assert rc == 0, (label, rc)
    batch.check([r[0] for r in res], [r[1] for r in res], [r[2] for r in res], lambda k, c: res[k][3][c], label + " host")


def decode_device(dec, batch, to_dev, from_dev, label="", junk=0xA5):
    """icerx_decode_device with the streams packed into one device blob, into a device buffer filled with junk first
    (to_dev(numpy array) -> (device pointer, handle), from_dev(handle) -> numpy array)"""
    blob, offs, lens = dec._pack(batch.streams)
    n, ch, stride = len(batch.streams), batch.channels, batch.stride
    dt = np.uint16 if batch.bits == 16 else np.uint8
    p_blob, h_blob = to_dev(blob)
    p_out, h_out = to_dev(np.full(n * ch * stride, junk, dt))
    rc, rcs, ws, hs = dec.decode_device(n, p_blob, offs, lens, p_out, stride)
    assert rc == 0, (label, rc)
    out = from_dev(h_out).view(dt)
    batch.check(rcs, ws, hs, lambda k, c: out[(k * ch + c) * stride:], label + " device")


def spread(specs, reps):
    """each spec `reps` times, round-robin: equal sizes never sit next to each other (for more than one spec)"""
    return [s for _ in range(reps) for s in specs]


def mixed_entries(sizes, kinds=("noise", "smooth"), reps=2, seed=0, wild=False, early_stops=True, big=None, small=None):
    """case 1 / 2: every size `reps` times at non-adjacent positions, lossless and quota-cut streams, then streams that stop
    early (damaged, empty, a frame larger than the stride, a frame too small for the segment grid) in between"""
    entries = []
    for r in range(reps):
        for i, (w, h) in enumerate(sizes):
            kind = kinds[(i + r) % len(kinds)]
            entries.append(((w, h, kind, seed + i), LOSSLESS if (i + r) % 2 == 0 else CUT, None))
    if wild:
        entries.insert(3, ((sizes[0][0], sizes[0][1], "wild", seed + 50), LOSSLESS, None))
    if early_stops:
        w, h = sizes[0]
        stops = [((w, h, "noise", seed), LOSSLESS, d) for d in DAMAGES]
        if big is not None:
            stops.append((("big", big[0], big[1], seed + 90), LOSSLESS, None))
        if small is not None:
            stops.append((("small", small[0], small[1], seed + 91), LOSSLESS, None))
        for j, e in enumerate(stops):                                   # (spread over the batch)
            entries.insert(min(len(entries), 1 + j * 2), e)
    return entries


def raw_call(dec, device, n, data_ptr, offsets, lens, out, stride, w_in, h_in):
    """icerx_decode_host (out = list of host plane pointers) / icerx_decode_device (out = a device pointer) with the
    caller's offsets, lengths and ws / hs in-values -> (rc, rcs, ws, hs)"""
    offs = (_sz * n)(*[int(o) for o in offsets])
    ln = (_sz * n)(*[int(x) for x in lens])
    rcs, ws, hs = (C.c_int * n)(), (_sz * n)(*w_in), (_sz * n)(*h_in)
    if device:
        rc = dec.lib.icerx_decode_device(dec.handle, n, data_ptr, offs, ln, out, stride, rcs, ws, hs)
    else:
        ptrs = (C.c_void_p * len(out))(*out)
        rc = dec.lib.icerx_decode_host(dec.handle, n, data_ptr, offs, ln, ptrs, stride, rcs, ws, hs)
    return rc, list(rcs), list(ws), list(hs)


class Layout:
    """case 7: streams in one blob the way a caller may hand them over -- junk before the first stream and between streams,
    offsets out of order, two entries naming the same bytes, a zero-length entry pointing into another stream -- with
    non-zero ws / hs in-values.  Expected: the oracle on each entry's bytes with the same in-values."""

    def __init__(self, orc, batch, seed=3):
        rng = np.random.default_rng(seed)
        streams = [s for s in batch.streams if s]
        blob, where = bytearray(rng.integers(0, 256, 37).astype(np.uint8).tobytes()), []
        for s in reversed(streams):                      # (laid out back to front: the offsets come out decreasing)
            where.append((len(blob), len(s)))
            blob += s + rng.integers(0, 256, int(rng.integers(1, 90))).astype(np.uint8).tobytes()
        where.reverse()
        entries = list(where)
        entries.insert(2, where[0])                      # the same bytes twice
        entries.insert(4, (where[1][0] + 5, 0))          # zero length, inside another stream
        entries.append((0, 0))
        entries.append((3, 20))                          # junk only
        self.blob = np.frombuffer(bytes(blob), np.uint8).copy()
        self.offsets, self.lens = [e[0] for e in entries], [e[1] for e in entries]
        self.n = len(entries)
        self.batch = batch
        # in-values: some that fit the stride, some that do not
        self.w_in = [int(rng.integers(1, 40)) for _ in range(self.n)]
        self.h_in = [int(rng.integers(1, 40)) for _ in range(self.n)]
        self.w_in[-1], self.h_in[-1] = 4000, 4000
        self.want = []
        for (o, n_), w0, h0 in zip(entries, self.w_in, self.h_in):
            s = bytes(self.blob[o: o + n_])
            self.want.append(oracle_decode(orc, s, batch.channels, batch.stages, batch.filt, batch.segments, batch.stride, batch.bits, w0, h0))
        self.kept = [not any(True for _ in packets_valid(bytes(self.blob[o: o + n_]))) for o, n_ in entries]
        assert sum(self.kept) >= 3 and sum(not k for k in self.kept) >= 4

    def check(self, rcs, ws, hs, frame, label=""):
        b = self.batch
        assert rcs == [w[0] for w in self.want], (label, rcs, [w[0] for w in self.want])
        for k, (rc, w, h, planes) in enumerate(self.want):
            assert (ws[k], hs[k]) == (w, h), (label, k)
            if self.kept[k]:
                assert (ws[k], hs[k]) == (self.w_in[k], self.h_in[k]), (label, k)
            else:
                assert (ws[k], hs[k]) != (self.w_in[k], self.h_in[k]), (label, k)
            if rc in (-5, -4, -1) or w * h == 0 or w * h > b.stride:
                continue
            for c in range(b.channels):
                assert np.array_equal(np.asarray(frame(k, c))[: w * h], planes[c][: w * h]), (label, k, c)


def packets_valid(stream):
    """the packets of a stream whose header and payload CRCs hold (what the decoder's scan accepts), at any offset"""
    off = 0
    while off + 28 <= len(stream):
        hdr = stream[off: off + 28]
        if hdr[:2] == b"\x5b\x60" and zlib.crc32(hdr[:24]) == int.from_bytes(hdr[24:28], "little"):
            n = (int.from_bytes(hdr[16:20], "little") + 7) // 8
            if off + 28 + n <= len(stream) and zlib.crc32(stream[off + 28: off + 28 + n]) == int.from_bytes(hdr[20:24], "little"):
                yield off
        off += 1


# ------------------------------------------------------------------------------------------ the cases
# (the GPU file runs them at the sizes below; the CPU mock-runtime build of decoder.hip runs them at MOCK sizes)
SIZES = {"gpu": [(67, 45), (67, 70), (96, 33), (40, 58)], "mock": [(21, 19), (21, 26), (34, 17)]}
GRID = {"gpu": (3, 6), "mock": (3, 5)}                   # stages, segments
BIG = {"gpu": (120, 90), "mock": (40, 40)}                # larger than the stride: rc -5
SMALL = {"gpu": (17, 17), "mock": (17, 17)}               # a subband with fewer samples than segments: rc -3


def mixed_batch(orc, channels, bits, filt, scale="gpu", seed=0, sizes=None, reps=3):
    """case 1 + 2: one configuration's batch of every size at non-adjacent positions, lossless and quota-cut, with the
    streams that stop early in between"""
    stages, segments = GRID[scale]
    sizes = sizes or SIZES[scale]
    b = Batch(orc, channels, bits, filt, stages, segments,
              mixed_entries(sizes, reps=reps, seed=seed + 100 * filt + channels + bits, wild=bits == 16, big=BIG[scale],
                            small=SMALL[scale]), seed=seed)
    rcs = b.rcs()
    assert {0, -3, -5} <= set(rcs), rcs
    assert rcs[[k for k, (s, q, d) in enumerate(b.entries) if s[0] == "small"][0]] == -3
    # the size groups of the inverse transform: several frames each, not next to each other, and two sizes of one width
    groups = b.groups()
    assert sum(1 for g in groups.values() if len(g) >= 2 and any(j - i > 1 for i, j in zip(g, g[1:]))) >= 3, groups
    assert len({w for (w, h) in groups}) < len(groups), groups
    return b


def header_pass_batch(orc, channels=1, bits=16, filt=1, frames=4, side=64):
    """case 5: flat frames with many stages and segments, whose packets are little more than their 28-byte header: more
    packets than count_headers_kernel's first capacity (total_len / 64 + 1024)"""
    entries = [((side + (k % 2), side, "flat", k), LOSSLESS, None) for k in range(frames)]
    b = Batch(orc, channels, bits, filt, 3, 16, entries)
    total = sum(len(s) for s in b.streams)
    n_packets = sum(len(packets(s)) for s in b.streams)
    assert n_packets > total // 64 + 1024, (n_packets, total)
    assert set(b.rcs()) == {0}
    return b


def reuse_batches(orc, bits, scale="gpu"):
    """case 6: a large batch, then a smaller one of other content and sizes (and a smaller stride), for one decoder"""
    large = mixed_batch(orc, 1, bits, 3, scale, seed=7)
    w0, h0 = SIZES[scale][0]
    sizes = [(w0 - 3, h0 + 2), (w0 + 5, h0 - 1)]
    small = Batch(orc, 1, bits, 3, *GRID[scale], [((w, h, "smooth", 60 + i), CUT if i % 2 else LOSSLESS, None)
                                                 for i, (w, h) in enumerate(sizes * 2)], seed=8)
    assert small.stride < large.stride and set(small.rcs()) == {0}
    return large, small


def layout_call(dec, layout, device, to_dev, from_dev, label=""):
    """case 7 through icerx_decode_device (device=True: blob and output in device memory, the output filled with junk) or
    icerx_decode_host"""
    b, n = layout.batch, layout.n
    dt = np.uint16 if b.bits == 16 else np.uint8
    p_blob, h_blob = to_dev(layout.blob)
    if device:
        p_out, h_out = to_dev(np.full(n * b.channels * b.stride, 0x5A, dt))
        rc, rcs, ws, hs = raw_call(dec, True, n, p_blob, layout.offsets, layout.lens, p_out, b.stride, layout.w_in, layout.h_in)
        out = from_dev(h_out).view(dt)
        frame = lambda k, c: out[(k * b.channels + c) * b.stride:]            # noqa: E731
    else:
        planes = [np.full(b.stride, 0x5A, dt) for _ in range(n * b.channels)]
        rc, rcs, ws, hs = raw_call(dec, False, n, layout.blob.ctypes.data, layout.offsets, layout.lens,
                                   [p.ctypes.data for p in planes], b.stride, layout.w_in, layout.h_in)
        frame = lambda k, c: planes[k * b.channels + c]                       # noqa: E731
    assert rc == 0, (label, rc)
    layout.check(rcs, ws, hs, frame, label)
