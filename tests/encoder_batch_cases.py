"""Frames of many kinds for the encoder's batch entry points (icerx_encode_host / _device / _async / _u8 / _rgb8 / _s8,
icerx_compress_batch_uint16_devices) and their expected results, shared by the GPU tests (tests/test_gpu_encoder_batch.py) and
the CPU checks that every kind reaches the path its name promises (tests/test_encoder_batch_cases.py).

A frame is named by a spec (kind, seed): the kind decides the content, the seed varies it.  For a 3-channel geometry the
kind may be a tuple of three kinds, one per channel (a single kind: the same kind in every channel, a seed per channel).
Every distinct (geometry, spec, quota) is coded once by the oracle (oracle/icer_oracle.c) and remembered.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from icer_compression_amd import synth

# 16-bit samples (icer_compress_image_[yuv_]uint16 and the 16-bit encoders)
KINDS16 = ("blank", "flat", "smooth", "noise8", "sparse", "wide", "dot", "overflow", "mean")
CODED16 = ("blank", "flat", "smooth", "noise8", "sparse", "wide", "dot")     # the kinds whose frames are coded (rc 0 or -5)
ABORTED16 = ("overflow", "mean")                                            # the kinds whose frames return ICER_INTEGER_OVERFLOW
# uint8 twins, int8 storage (icer_compress_image_[yuv_]uint8, encoders of sample_bits 8)
KINDS8 = ("blank8", "noise6", "smooth6", "full8")
# raw inputs of the front ends: 8-bit gray (icerx_encode_device_u8) and packed RGB888 (icerx_encode_device_rgb8)
RAW_GRAY = ("blank", "white", "noise", "smooth")
RAW_RGB = ("black", "white", "noise", "ramp")

QUOTA_CLASSES = ("lossless", "cut", "progressive", "tiny27", "tiny28", "tiny60")


class Geometry(NamedTuple):
    w: int
    h: int
    channels: int = 1
    stages: int = 3
    filt: int = 0
    segments: int = 6
    bits: int = 16                  # 16, or 8 for the uint8 twins
    raw: str = ""                   # "", "gray8" (icerx_encode_device_u8) or "rgb8" (icerx_encode_device_rgb8): what the batch holds

    @property
    def samples(self) -> int:
        return self.w * self.h * self.channels


def quota(g: Geometry, cls: str) -> int:
    """lossless: room for any stream (two bytes per sample, and a header and a few bytes per coding unit for small frames);
    cut: above half a byte per sample (not progressive mode) and below the lossless size of dense frames; progressive: below
    half a byte per sample; tinyN: N bytes (one packet header is 28)"""
    S = g.samples
    if cls == "lossless":
        return 2 * S + 40 * (3 * g.stages + 1) * g.segments * 9 * g.channels
    if cls == "cut":
        return S // 2 + S // 8
    if cls == "progressive":
        return S // 8
    if cls.startswith("tiny"):
        return int(cls[4:])
    raise ValueError(cls)


def plane16(kind: str, w: int, h: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(0x1CE5 + 7919 * seed + 104729 * KINDS16.index(kind))
    if kind == "blank":
        return np.zeros((h, w), np.uint16)
    if kind == "flat":
        return np.full((h, w), 1 + (211 * seed + 37) % 4000, np.uint16)
    if kind == "smooth":
        return synth.gray_frame(w, h, 1000 + seed, 1)
    if kind == "noise8":
        return synth.gray_frame(w, h, 2000 + seed, 0)
    if kind == "sparse":                 # about 10 % nonzero samples
        return np.where(rng.random((h, w)) < 0.1, rng.integers(1, 256, (h, w)), 0).astype(np.uint16)
    if kind == "wide":                   # 12-bit noise: more than the nine coded planes of content
        return synth.gray_frame(w, h, 3000 + seed, 2)
    if kind == "dot":                    # one bright sample on blank
        p = np.zeros((h, w), np.uint16)
        p[int(rng.integers(0, h)), int(rng.integers(0, w))] = 255
        return p
    if kind == "overflow":               # full range: the transform leaves int16
        return rng.integers(0, 65536, (h, w)).astype(np.uint16)
    if kind == "mean":                   # the transform is fine, the LL mean is above INT16_MAX
        return np.full((h, w), 40000 + 1000 * (seed % 5), np.uint16)
    raise ValueError(kind)


def plane8(kind: str, w: int, h: int, seed: int) -> np.ndarray:
    if kind == "blank8":
        return np.zeros((h, w), np.uint8)
    if kind == "noise6":                 # (coded under filter A; the other filters take 6-bit noise out of int8)
        return synth.gray_frame_u8(w, h, 4000 + seed, 0)
    if kind == "smooth6":
        return synth.gray_frame_u8(w, h, 5000 + seed, 1)
    if kind == "full8":                  # full 8-bit range in int8 storage: the transform leaves int8
        return np.random.default_rng(6000 + seed).integers(0, 256, (h, w)).astype(np.uint8)
    raise ValueError(kind)


def raw_gray(kind: str, w: int, h: int, seed: int) -> np.ndarray:
    """(h, w) uint8, as icerx_encode_device_u8 takes it"""
    if kind == "blank":
        return np.zeros((h, w), np.uint8)
    if kind == "white":
        return np.full((h, w), 255, np.uint8)
    if kind == "noise":
        return np.random.default_rng(7000 + seed).integers(0, 256, (h, w)).astype(np.uint8)
    if kind == "smooth":
        return synth.gray_frame(w, h, 8000 + seed, 1).astype(np.uint8)
    raise ValueError(kind)


def raw_rgb(kind: str, w: int, h: int, seed: int) -> np.ndarray:
    """(h, w, 3) uint8 packed RGB888, as icerx_encode_device_rgb8 takes it"""
    if kind == "black":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "noise":
        return np.random.default_rng(9000 + seed).integers(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "ramp":                   # a horizontal ramp in R, a vertical one in G, their mix in B
        x = np.linspace(0, 255, w)[None, :] * np.ones((h, 1))
        y = np.linspace(0, 255, h)[:, None] * np.ones((1, w))
        return np.stack([x, y, (x + y + 8 * seed) / 2 % 256], axis=-1).astype(np.uint8)
    raise ValueError(kind)


def ycbcr(rgb: np.ndarray):
    """packed RGB888 -> Y, Cb, Cr planes (uint16) with the integer formulas the reference's example callers apply before the
    YUV encoder (the same restatement as tests/test_gpu_parity.py test_frontend_fusion_u8_and_rgb8)"""
    r, g, b = (rgb[:, :, c].astype(np.int64) for c in range(3))
    clip = lambda v: np.clip(v, 0, 255)
    y = clip((19595 * r + 38470 * g + 7471 * b) >> 16)
    cb = clip(((36962 * (b - y)) >> 16) + 128)
    cr = clip(((46727 * (r - y)) >> 16) + 128)
    return [p.astype(np.uint16) for p in (y, cb, cr)]


def channel_kinds(g: Geometry, kind):
    return tuple(kind) if isinstance(kind, tuple) else (kind,) * g.channels


def raw_input(g: Geometry, spec) -> np.ndarray:
    """the frame as the batch holds it: (C, h, w) samples, or (h, w) / (h, w, 3) bytes for the front ends"""
    kind, seed = spec
    if g.raw == "gray8":
        return raw_gray(kind, g.w, g.h, seed)
    if g.raw == "rgb8":
        return raw_rgb(kind, g.w, g.h, seed)
    make = plane16 if g.bits == 16 else plane8
    return np.stack([make(k, g.w, g.h, 3 * seed + c) for c, k in enumerate(channel_kinds(g, kind))])


def oracle_planes(g: Geometry, spec):
    """the planes the oracle codes for this frame: a front end's input converted as the reference's callers convert it"""
    x = raw_input(g, spec)
    if g.raw == "gray8":
        return [x.astype(np.uint16)]
    if g.raw == "rgb8":
        return ycbcr(x)
    return list(x)


def batch(g: Geometry, specs) -> np.ndarray:
    """(n, C, h, w) uint16 / uint8, or (n, h, w) / (n, h, w, 3) uint8 for the front ends: C-contiguous"""
    return np.ascontiguousarray(np.stack([raw_input(g, s) for s in specs]))


class Expected:
    """The oracle's (rc, stream, planes left) per (geometry, spec, quota), computed once."""

    def __init__(self, orc):
        self.orc = orc
        self.memo = {}

    def __call__(self, g: Geometry, spec, q: int):
        key = (g, spec, q)
        if key not in self.memo:
            planes = oracle_planes(g, spec)
            fn = self.orc.compress_u8 if g.bits == 8 else self.orc.compress
            self.memo[key] = fn(planes, g.stages, g.filt, g.segments, q)
        return self.memo[key]


def first_difference(a: bytes, b: bytes) -> int:
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i
    return min(len(a), len(b)) if len(a) != len(b) else -1


def check_frame(got_rc: int, got: bytes, want, what="") -> None:
    """rc, size and bytes of one frame against the oracle's"""
    rc, stream = want[0], want[1]
    assert got_rc == rc and got == stream, \
        f"{what}: rc {got_rc} (oracle {rc}), {len(got)} bytes (oracle {len(stream)}), first difference at byte {first_difference(got, stream)}"


def coefficients_comparable(want) -> bool:
    """the drop-in entry points give back the reference's planes for every frame; the batch encoders keep a frame's sign-magnitude
    planes on the device, which are the reference's for every frame that was coded (an aborted frame leaves partly transformed data
    in the reference's planes, which the batch API does not restate)"""
    return want[0] in (0, -5)


def check_coefficients(g: Geometry, got_words, want, what="") -> None:
    """got_words: the encoder's coefficient planes of one frame (icerx_get_coefficients, one (h, w) uint16 per channel); the uint8
    twins keep 16-bit sign-magnitude words, the reference int8 sign-magnitude bytes"""
    for c, (got, ref) in enumerate(zip(got_words, want[2])):
        if g.bits == 8:
            got = (((got >> 8) & 0x80) | (got & 0x7F)).astype(np.uint8)
        assert np.array_equal(got, ref), f"{what}: coefficient plane {c} differs at {np.argwhere(got != ref)[:4].tolist()}"
