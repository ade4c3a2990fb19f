"""The cases of the region-of-interest encode on the GPU (icerx_encode_device_roi), shared by tests/test_gpu_roi.py and
tests/golden/make_roi_golden.py: five geometries chosen so that roi_rank_kernel can still go wrong, two batches each (3 frames
for an encoder of max_frames 4, 5 frames for one of max_frames 8: the two-part enqueue), a different rectangle per frame,
five shifts and six quotas per call."""
from __future__ import annotations

from tests import encoder_batch_cases as ebc
from tests import roi_model as rm
from tests import target_model as tm

#        geometry                                     units   why
GEOMETRIES = {
    "G1": ebc.Geometry(96, 80, 1, 3, 0, 6),           # 540    more than one workgroup's worth of threads, not a multiple of 64
    "G2": ebc.Geometry(72, 56, 3, 2, 1, 4),           # 756    the YUV priorities of quirk D4
    "G3": ebc.Geometry(64, 64, 3, 2, 6, 3, bits=8),   # 441    7 planes, the upward final order; one frame leaves int8: no stream
    "G4": ebc.Geometry(256, 192, 1, 4, 0, 32),        # 3 744  the largest unit count
    "G5": ebc.Geometry(40, 40, 1, 1, 0, 1),           # 36     under one wave, everything foreground
}
UNITS = {"G1": 540, "G2": 756, "G3": 441, "G4": 3744, "G5": 36}

# (frames of the batch, max_frames of its encoder, first rectangle kind)
BATCHES = {
    "G1": ([("noise8", 0), ("smooth", 1), ("sparse", 2)], [("wide", 0), ("noise8", 3), ("dot", 1), ("smooth", 4), ("blank", 0)]),
    "G2": ([("noise8", 0), ("smooth", 1), (("smooth", "noise8", "sparse"), 2)],
           [("wide", 0), ("noise8", 3), (("noise8", "smooth", "smooth"), 1), ("smooth", 4), ("sparse", 0)]),
    "G3": ([("smooth6", 0), ("full8", 1), ("smooth6", 2)], [("smooth6", 3), ("blank8", 0), ("smooth6", 4), ("full8", 2), ("smooth6", 5)]),
    "G4": ([("noise8", 0), ("smooth", 1), ("sparse", 2)], [("wide", 0), ("noise8", 3), ("dot", 1), ("smooth", 4), ("noise8", 5)]),
    "G5": ([("noise8", 0), ("smooth", 1), ("sparse", 2)], [("wide", 0), ("noise8", 3), ("dot", 1), ("smooth", 4), ("blank", 0)]),
}
MAX_FRAMES = (4, 8)
SHIFTS = (0, 1, 3, 9, 16)
RECT_KINDS = ("empty", "full", "segment", "border", "last", "outside")
NO_STREAM = ("full8", "overflow", "mean")


def model(name: str) -> tm.Model:
    g = GEOMETRIES[name]
    m = tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments, g.bits)
    assert m.n_units == UNITS[name], (name, m.n_units)
    return m


def rectangle(m: tm.Model, kind: str):
    """(x, y, w, h): empty, the full frame, one inside a single segment (the middle segment of the finest HH subband), one crossing
    the right and bottom border, the last pixel, one with x >= w"""
    w, h = m.w, m.h
    if kind == "empty":
        return (w // 3, h // 3, 0, 11)
    if kind == "full":
        return (0, 0, w, h)
    if kind == "segment":
        k = next(i for i, u in enumerate(m.units) if u[1] == 1 and u[2] == tm.HH and u[4] == (m.units[-1][4] + 1) // 2)
        sx, sy, sw, sh = rm.local_rect(m, k)
        return (2 * sx + sw // 2, 2 * sy + sh // 2, max(1, sw), max(1, sh))
    if kind == "border":
        return (w - w // 4, h - h // 5, w, h)
    if kind == "last":
        return (w - 1, h - 1, 1, 1)
    if kind == "outside":
        return (w, h // 2, 9, 9)
    raise ValueError(kind)


def rectangles(name: str, b: int):
    """the rectangle of every frame of batch b: a different kind per frame, all six kinds over the two batches"""
    m = model(name)
    first = (0, 3)[b]
    return [rectangle(m, RECT_KINDS[(first + f) % len(RECT_KINDS)]) for f in range(len(BATCHES[name][b]))]


def quotas(name: str):
    """one that keeps everything, one below w * h * channels / 2 (where a ladder call turns progressive), one in between, 28, 0,
    and a repeat"""
    g = GEOMETRIES[name]
    S = g.samples
    return [ebc.quota(g, "lossless"), S // 4, S // 2 + S // 8, 28, 0, S // 4]


def has_stream(spec) -> bool:
    kinds = spec[0] if isinstance(spec[0], tuple) else (spec[0],)
    return not any(k in NO_STREAM for k in kinds)


def golden_key(name: str, b: int, shift: int) -> str:
    return f"{name}/batch{b}/shift{shift}"
